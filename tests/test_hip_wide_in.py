"""Recurrent nets on wide inputs: LSTM / MGU / RNN layers (multiples of 16 cells, no convolutions or encoder layers in front) over a state
beyond 256 components or a stacked input beyond 1024, up to 8192.  They run time-step-major whatever their cell count, the first layer's
input product of all window rows as one launch (rectm.hip: tm_win_product_kernel), its forward tiles over the recurrent part alone
(tm_win_lstm_fwd_kernel / tm_win_mgu_fwd_kernel / tm_win_rnn_fwd_kernel).  Against two fixtures recorded from the compiled reference
(tests/golden/make_wide_in.sh) and against the oracle on minibatches the library draws itself; bodies and tolerances are those of
test_hip_a22.py."""
import numpy as np
import pytest

import test_hip_a22
from smarties_amd import capi
from oracle_api import synth_cfg, fill_synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,restricted", [("lstm_wide_in.bin", False), ("mgu_wide_in.bin", True)], ids=["lstm_wide_in", "mgu_wide_in"])
def test_steps_follow_reference_fixture(hip_api, monkeypatch, name, restricted):
    monkeypatch.setitem(test_hip_a22.A22_FIXTURES, name, ("Tanh", restricted))
    test_hip_a22.test_steps_follow_reference_fixture_a22(hip_api, name)


SHAPES = [  # (layer type, hidden, dimS, nAppendedObs, bptt, batch)
    ("lstm", (32, 16), 257, 0, 3, 6),       # one component above the old limit; fewer than 16 samples; 24 product rows
    ("rnn", (272,), 1027, 0, 3, 6),         # a reduction that is no multiple of 4; 272 columns; 17 cell tiles
    ("mgu", (64, 32), 300, 4, 4, 20),       # 1500 inputs from appended observations; windows that begin before the episode's start; a partial second block of 16 samples; both MGU phases
    ("lstm", (48, 48), 1030, 0, 16, 40),    # the shipped window length; three sample blocks; parametric residual on layer 2
    ("lstm", (16,), 8192, 0, 2, 4),         # the upper bound
]
_IDS = ["%s-%s-dS%d-app%d" % (sh[0], "x".join(map(str, sh[1])), sh[2], sh[3]) for sh in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_wide_inputs_match_oracle(hip_api, shape):
    """test_hip_a22.test_wide_and_appended_recurrent_layers_match_oracle on these shapes: three eager steps tap by tap within TOL32, ten
    replayed ones (the captured graph) with equal sample indices and generator state and weights within 2 TOL32, acting on windows of 1, 2,
    bptt + 1 and bptt + 1 + nApp states within TOL32, a longer window refused."""
    test_hip_a22.test_wide_and_appended_recurrent_layers_match_oracle(hip_api, shape)


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[1]], ids=[_IDS[2], _IDS[1]])
def test_batched_acting_equals_window_by_window(hip_api, shape):
    """hl_forward_sequences runs these nets' agents as the samples of one chain per chunk of min(local batch, what the staging holds): 13
    agents at a local batch of 6 are three chunks, windows of 1, 3 and bptt + 1 + nApp states mixed in each.  The same kernels on the same
    rows in the same order as hl_forward_sequence: bit-identical window by window."""
    kind, hidden, dS, nApp, bptt, _ = shape
    nnt = {"lstm": capi.NN_LSTM, "mgu": capi.NN_MGU, "rnn": capi.NN_RNN}[kind]
    L = capi.Learner(hip_api, capi.make_config(dimS=dS, dimA=2, bounded=[1, 0], hidden=hidden, nnFunc="Tanh", batchSize=6, maxTotObsNum=8000, randSeed=5,
                                               nn_type=nnt, adv_kind=capi.ADV_GAUSSIAN, nnBPTTseq=bptt, nAppendedObs=nApp))
    L.init_weights(); fill_synth(L, synth_cfg(seed=21, dimS=dS, dimA=2, lenMin=2, lenMax=30, pTerm=0.5), 60); L.initialize()
    rng = np.random.default_rng(11)
    lens = [(1, 3, bptt + 1 + nApp)[i % 3] for i in range(13)]
    wins = [rng.normal(size=(n, dS)).astype(np.float32) for n in lens]
    out = L.forward_sequences(wins)
    for i, w in enumerate(wins):
        assert np.array_equal(out[i], L.forward_sequence(w)), (i, lens[i])
    L.close()


def test_window_rows_beyond_the_launches_offsets_are_refused_with_a_message(hip_api):
    """16384 samples x 18 window rows x (8192 + 16 + 1 -> 8224) floats of the first layer's operand rows reach 2^31 floats: refused at
    hl_create, before anything of that size is allocated, and hl_last_error says which bound."""
    with pytest.raises(capi.HlError) as e:
        capi.Learner(hip_api, capi.make_config(dimS=8192, dimA=2, bounded=[1, 0], hidden=(16,), nnFunc="Tanh", batchSize=16384, maxTotObsNum=20000,
                                               nn_type=capi.NN_LSTM, adv_kind=capi.ADV_GAUSSIAN, nnBPTTseq=16))
    assert e.value.status == 8 and "2^31" in str(e.value)


def test_two_runs_end_bit_identical(hip_api):
    """1 + 5 + 30 steps (eager and replayed) of three LSTM layers on 1100 states, twice: the product's elements are one chain of MFMAs each
    and the backward diagonals join their producers' values in a fixed order, so weights, generator state and beta end bit-identical."""
    sc = synth_cfg(seed=7, dimS=1100, dimA=2, lenMin=5, lenMax=60, pTerm=0.4)

    def run():
        L = capi.Learner(hip_api, capi.make_config(dimS=1100, dimA=2, bounded=[1, 0], hidden=(32, 16, 16), nnFunc="Tanh", batchSize=24, maxTotObsNum=50000, randSeed=3,
                                                   nn_type=capi.NN_LSTM, adv_kind=capi.ADV_GAUSSIAN, nnBPTTseq=5))
        L.init_weights(); fill_synth(L, sc, 100); L.initialize()
        for n in (1, 5, 30):
            L.step(n)
        L.sync()
        out = (L.get_params()[0].copy(), L.get_rng_state().copy(), L.scalars().beta)
        L.close()
        return out
    a, b = run(), run()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
