"""Plain RNN layers (nnType "RNN": BaseLayer with bRecurrent, Network/Builder.cpp:76-81, Layer_Base.h:64-113) of 257 .. 1024 cells, all
multiples of 16: training and acting windows time-step-major on the MFMA (rectm.hip: rnn_tm_fwd_kernel / rnn_tm_bwd_kernel).  Against a
fixture recorded from the compiled reference (tests/golden/make_rnn_wide.sh) and against the oracle on minibatches the library draws
itself; bodies and tolerances are those of the LSTM / MGU tests of test_hip_a22.py / test_hip_r5.py."""
import numpy as np
import pytest

import test_hip_a22
import test_hip_r5
from smarties_amd import capi
from oracle_api import synth_cfg, fill_synth
from parity import relinf
from test_hip_parity import _pair, _compare_step, TOL32

pytestmark = pytest.mark.gpu


def test_steps_follow_reference_fixture(hip_api, monkeypatch):
    monkeypatch.setitem(test_hip_a22.A22_FIXTURES, "rnn_wide.bin", ("Tanh", False))
    test_hip_a22.test_steps_follow_reference_fixture_a22(hip_api, "rnn_wide.bin")


SHAPES = [  # (hidden, dimS, nAppendedObs, bptt, batch, nnFunc)
    ((272,), 7, 0, 3, 6, "Tanh"),              # one layer just above the limit: 17 tiles of 16 cells (an odd number), fewer than 16 samples
    ((320, 272), 9, 2, 4, 12, "Tanh"),         # two layers, parametric residual, appended observations in front of the window
    ((272, 320), 5, 0, 3, 20, "SoftSign"),     # a residual narrower than its layer, a partial second block of 16 samples, a derivative that is not tanh's
    ((272, 96, 80), 6, 0, 5, 20, "SoftSign"),  # three layers, wide and narrow mixed: the middle layer's deltas have both producers on one diagonal
    ((272, 272), 5, 0, 16, 40, "Tanh"),        # the window length the shipped preset uses, three sample blocks
    ((1024, 1024), 5, 0, 2, 4, "Tanh"),        # the upper bound: the largest staged A tile the predicate admits (2048 + pad floats x 16 rows)
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "%s-dS%d-app%d-%s" % ("x".join(map(str, sh[0])), sh[1], sh[2], sh[5]))
def test_wide_rnn_layers_match_oracle(hip_api, shape):
    """test_hip_a22.test_wide_and_appended_recurrent_layers_match_oracle for nnType "RNN": three eager steps tap by tap, ten more with equal
    sample indices and generator state and weights within 2 TOL32, acting on windows of 1, 2, bptt + 1 and bptt + 1 + nApp states, a longer
    window refused."""
    hidden, dS, nApp, bptt, batch, func = shape
    kw = dict(dimS=dS, dimA=2, bounded=[1, 0], hidden=hidden, nnFunc=func, batchSize=batch, maxTotObsNum=8000, randSeed=5,
              nn_type=capi.NN_RNN, adv_kind=capi.ADV_GAUSSIAN, nnBPTTseq=bptt, nAppendedObs=nApp)
    G, O = _pair(hip_api, kw, synth_cfg(seed=21, dimS=dS, dimA=2, lenMin=2, lenMax=30, pTerm=0.5), 60)
    for _ in range(3):
        G.step(1); O.step(1)
        _compare_step(G, O)
    G.step(10); O.step(10)
    assert np.array_equal(G.readback(capi.TAP_FLAT), O.readback(capi.TAP_FLAT))
    assert np.array_equal(G.get_rng_state(), O.get_rng_state())
    assert relinf(G.get_params()[0], O.get_params()[0]) < 2 * TOL32
    rng = np.random.default_rng(5)
    for n in sorted({1, 2, bptt + 1, bptt + 1 + nApp}):
        S = rng.normal(size=(n, dS)).astype(np.float32)
        assert relinf(G.forward_sequence(S), O.forward_sequence(S)) < TOL32, n
    with pytest.raises(capi.HlError):
        G.forward_sequence(rng.normal(size=(bptt + 2 + nApp, dS)).astype(np.float32))


def test_wide_rnn_at_a_large_local_batch_matches_oracle(hip_api):
    test_hip_r5.test_recurrent_nets_at_large_local_batches_match_oracle(hip_api, capi.NN_RNN, (272,), 1040, 2)


def test_backward_by_diagonals_is_deterministic(hip_api):
    """test_hip_r5.test_time_step_major_backward_by_diagonals_is_deterministic for three RNN layers: whichever producer of a tile of deltas
    arrives second forms them from the same two inputs, so two runs end bit-identical (weights, generator, beta)."""
    sc = synth_cfg(seed=7, dimS=6, dimA=2, lenMin=5, lenMax=60, pTerm=0.4)

    def run():
        L = capi.Learner(hip_api, capi.make_config(dimS=6, dimA=2, bounded=[1, 0], hidden=(288, 272, 272), nnFunc="Tanh", batchSize=72, maxTotObsNum=50000, randSeed=3,
                                                   nn_type=capi.NN_RNN, adv_kind=capi.ADV_GAUSSIAN, nnBPTTseq=9))
        L.init_weights(); fill_synth(L, sc, 200); L.initialize()
        for n in (1, 5, 30):
            L.step(n)
        L.sync()
        out = (L.get_params()[0].copy(), L.get_rng_state().copy(), L.scalars().beta)
        L.close()
        return out
    a, b = run(), run()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_batched_acting_equals_window_by_window(hip_api):
    """hl_forward_sequences loops nets with layers above 256 cells agent by agent (include/smarties_hip_act.h): bit-identical to
    hl_forward_sequence per window."""
    L = capi.Learner(hip_api, capi.make_config(dimS=9, dimA=2, bounded=[1, 0], hidden=(320, 272), nnFunc="Tanh", batchSize=12, maxTotObsNum=8000, randSeed=5,
                                               nn_type=capi.NN_RNN, adv_kind=capi.ADV_GAUSSIAN, nnBPTTseq=4))
    L.init_weights(); fill_synth(L, synth_cfg(seed=21, dimS=9, dimA=2, lenMin=2, lenMax=30, pTerm=0.5), 60); L.initialize()
    rng = np.random.default_rng(11)
    wins = [rng.normal(size=(n, 9)).astype(np.float32) for n in (1, 3, 5)]
    out = L.forward_sequences(wins)
    for i, w in enumerate(wins):
        assert np.array_equal(out[i], L.forward_sequence(w)), i
    L.close()


@pytest.mark.parametrize("hidden", [(260,), (1040,)], ids=["260", "1040"])
def test_still_refused_on_the_device(hip_api, hidden):
    with pytest.raises(capi.HlError) as e:
        capi.Learner(hip_api, capi.make_config(dimS=5, dimA=2, bounded=[1, 0], hidden=hidden, nnFunc="Tanh", batchSize=8, maxTotObsNum=2000,
                                               nn_type=capi.NN_RNN, adv_kind=capi.ADV_GAUSSIAN, nnBPTTseq=3))
    assert e.value.status == 8
