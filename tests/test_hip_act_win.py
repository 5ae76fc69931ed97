"""hl_forward_sequences for the recurrent nets neither the batched window kernel nor the time-step-major chain serves
(include/smarties_hip_act.h): recurrent layers behind convolutions, RNN encoder layers under MGU layers, nets of at most 256 cells whose
window exceeds the batched kernel's 64 KB.  The agents of a chunk are the samples of ONE chain of hl_forward_sequence's own launches
(smarties_amd/csrc/learner_act.h: actWinChain): workgroup b of the window kernels (smarties_amd/csrc/rec.hip) walks agent b's window,
taken from a per-agent table; a chunk holds min(batchSize, ACT_SEQ_CHUNK) agents.

GPU suite: every agent bit for bit against the library's own single-agent hl_forward_sequence and within TOL32 of the CPU oracle, in any
order of the agents; rows left by a longer window of the call before; one chain per chunk; training untouched; refusals.
CPU suite (the last test): the four extended forward kernels use no scratch memory and spill no vector register, in any instantiation.

The shapes are the smallest at which each piece can go wrong."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from acting import FALLBACK, TOL32, _compare_step, _pair, _ragged as _windows
from oracle_api import synth_cfg, fill_synth
from parity import relinf
from smarties_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW_KERNELS = ("rnn_forward_kernel", "mgu_forward_kernel", "rec_forward_kernel", "lstm_forward_lds_kernel")
CONV_EXTRA = [(8, 8, 12, 32, 4, 1), (5, 5, 32, 64, 3, 1)]      # an 8 x 8 x 12 image of 1 + 2 stacked states of 256 + 2 components: 6 beside it

GAUSS = dict(dimA=2, bounded=[1, 0], adv_kind=capi.ADV_GAUSSIAN)
DISCRETE = dict(dimA=1, adv_kind=capi.ADV_DISCRETE)
SHAPES = {  # name: (configuration, agents)
    # two segments (the RNN encoder layer's rows are the MGU layers' input), chunks of 6, 6, 6, 2
    "rnn-enc-mgu": (dict(GAUSS, dimS=5, hidden=(16, 16), encoder=[24], encoder_rnn=1, nn_type=capi.NN_MGU, nnBPTTseq=5, batchSize=6,
                         maxTotObsNum=2000, randSeed=5), 20),
    # per-agent context states feeding the lower segment
    "rnn-enc-mgu-app2": (dict(GAUSS, dimS=5, hidden=(16,), encoder=[24], encoder_rnn=1, nn_type=capi.NN_MGU, nnBPTTseq=4, nAppendedObs=2,
                              batchSize=12, maxTotObsNum=2000, randSeed=5), 30),
    # convolutional front, appended observations, discrete head, chunks of 6, 6, 2
    "conv-lstm": (dict(FALLBACK["conv-lstm"][0], batchSize=6), 14),
    # the surplus state joining the conv outputs
    "conv-mgu-extra": (dict(DISCRETE, dimS=258, n_options=5, nAppendedObs=2, conv=CONV_EXTRA, hidden=(16,), nn_type=capi.NN_MGU, nnBPTTseq=3,
                            batchSize=4, maxTotObsNum=2000, randSeed=3), 9),
    # 65 x 256 floats = 66 560 B of window, just over the batched kernel's 64 KB
    "lstm-long-window": (dict(GAUSS, dimS=256, hidden=(16,), nn_type=capi.NN_LSTM, nnBPTTseq=64, batchSize=4, maxTotObsNum=8000,
                              randSeed=5), 6),
}


def _cfg(name):
    return dict(SHAPES[name][0], nnFunc="Tanh")


def _dims(name):
    """dimS, nAppendedObs, nnBPTTseq, batchSize, agents"""
    kw, agents = SHAPES[name]
    return kw["dimS"], kw.get("nAppendedObs", 0), kw["nnBPTTseq"], kw["batchSize"], agents


def _synth(name):
    if name in FALLBACK:
        return synth_cfg(**FALLBACK[name][1])
    kw = SHAPES[name][0]
    return synth_cfg(seed=21, dimS=kw["dimS"], dimA=kw["dimA"], lenMin=5, lenMax=40, pTerm=0.5)


def _ragged_lengths(name):
    _, nApp, bptt, _, _ = _dims(name)
    return [1, 2, bptt + 1, 3] + ([bptt + 1 + nApp, bptt + 2] if nApp else [])


@pytest.fixture(scope="module")
def nets(hip_api):
    """name -> (G, O) after three training steps (the weights are not the initial ones), built once; the tests that share a pair only act"""
    made = {}

    def get(name):
        if name not in made:
            G, O = _pair(hip_api, _cfg(name), _synth(name), 40)
            G.step(3); O.step(3)
            made[name] = (G, O)
        return made[name]
    yield get
    for G, O in made.values():
        G.close(); O.close()


def _assert_single_agent_bits(G, wins, out, what):
    assert out.shape == (len(wins), G.nOut)
    for i, w in enumerate(wins):
        assert np.array_equal(out[i], G.forward_sequence(w)), (what, i, w.shape[0])


# ---- 1. per agent, against both references ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_agent_equals_the_single_agent_call_and_the_oracle(nets, name):
    G, O = nets(name)
    dS, _, _, _, agents = _dims(name)
    rng = np.random.default_rng(11)
    wins = _windows(rng, agents, dS, _ragged_lengths(name))
    out = G.forward_sequences(wins)
    one = [G.forward_sequence(w) for w in wins]
    assert out.shape == (agents, G.nOut)
    for i, w in enumerate(wins):
        assert np.array_equal(out[i], one[i]), (name, i, w.shape[0], out[i], one[i])
        assert relinf(out[i], O.forward_sequence(w)) < TOL32, (name, i, w.shape[0])
    # the windows in another order: an agent's place, chunk and neighbours do not matter
    perm = rng.permutation(agents)
    out2 = G.forward_sequences([wins[i] for i in perm])
    for q, i in enumerate(perm):
        assert np.array_equal(out2[q], one[i]), (name, q, i)


# ---- 2. rows left by the call before ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rnn-enc-mgu", "conv-lstm"])
def test_a_longer_window_of_the_call_before_does_not_leak(nets, name):
    """rows b K + k of the lower segment's outputs / of the conv outputs outlive a call: a shorter window must not read them"""
    G, _ = nets(name)
    dS, _, bptt, _, agents = _dims(name)
    rng = np.random.default_rng(12)
    for what, lengths in (("full", [bptt + 1]), ("one state", [1]), ("mixed", [2, bptt + 1, 1, 4])):
        wins = _windows(rng, agents, dS, lengths)
        _assert_single_agent_bits(G, wins, G.forward_sequences(wins), what)


# ---- 3. one chain per chunk -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_chain_of_launches_per_chunk(nets):
    name = "rnn-enc-mgu"
    G, _ = nets(name)
    dS, _, _, batch, agents = _dims(name)
    rng = np.random.default_rng(13)
    wins = _windows(rng, agents, dS, _ragged_lengths(name))
    G.forward_sequences(wins[:2])
    G.timing_enable(True)
    try:
        s0 = G.timing_get("act_seq")[1]
        t0 = G.timing_get("act_tm_chain")[1]
        n0 = G.timing_get("act_win_chain")[1]
        G.forward_sequences(wins[:batch])
        n1 = G.timing_get("act_win_chain")[1]
        assert n1 - n0 == 1
        G.forward_sequences(wins)
        n2 = G.timing_get("act_win_chain")[1]
        assert n2 - n1 == -(-agents // batch) == 4
        assert G.timing_get("act_seq")[1] == s0
        assert G.timing_get("act_tm_chain")[1] == t0
    finally:
        G.timing_enable(False)


# ---- 4. training untouched ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rnn-enc-mgu", "conv-lstm"])
def test_batched_acting_leaves_training_untouched(hip_api, name):
    """The body of test_hip_act_tm.test_batched_acting_leaves_training_untouched: the chain borrows the training rows of the chunk's
    agents, a minibatch drawn ahead must stay as it is -- eager steps and the prepared-graph form."""
    dS, _, bptt, batch, _ = _dims(name)
    G, O = _pair(hip_api, _cfg(name), _synth(name), 40)
    rng = np.random.default_rng(2)
    wins = _windows(rng, 2 * batch + 5, dS, [1, 2, bptt + 1])      # more agents than one chunk holds
    for _ in range(3):
        G.step(1); O.step(1)
        _compare_step(G, O)
        out = G.forward_sequences(wins)
        assert relinf(out[-1], O.forward_sequence(wins[-1])) < TOL32
    G.step(4); O.step(4)
    _compare_step(G, O)
    G.prepare_steps(3)
    for _ in range(2):
        G.step(3); O.step(3)
        _compare_step(G, O)
        out = G.forward_sequences(wins)
        assert relinf(out[0], O.forward_sequence(wins[0])) < TOL32
    G.step(3); O.step(3)
    _compare_step(G, O)
    assert np.array_equal(G.get_rng_state(), O.get_rng_state())
    assert relinf(G.get_params()[0], O.get_params()[0]) < 2 * TOL32
    G.close(); O.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(hip_api):
    name = "rnn-enc-mgu-app2"
    dS, nApp, bptt, _, agents = _dims(name)
    G = capi.Learner(hip_api, capi.make_config(**_cfg(name)))
    G.init_weights(); fill_synth(G, _synth(name), 40); G.initialize()
    G.step(2)
    rng = np.random.default_rng(4)
    wins = _windows(rng, agents, dS, _ragged_lengths(name))
    assert G.forward_sequences([]).shape == (0, G.nOut)                        # n = 0: HL_OK
    assert np.isfinite(G.forward_sequences(wins)).all()
    wins[agents // 2] = rng.normal(size=(bptt + 2 + nApp, dS)).astype(np.float32)      # one window too long, in the middle of the batch
    out = np.full((agents, G.nOut), -7.25)
    with pytest.raises(capi.HlError) as e:
        G.forward_sequences(wins, out=out)
    assert e.value.status == 1                                                 # HL_ERR_BAD_ARG
    assert (out == -7.25).all()                                                # nothing written
    n_steps = np.array([3, 0], np.int32); st = np.zeros((3, dS), np.float32)
    rc = hip_api.fn("forward_sequences")(G.h, 2, n_steps.ctypes.data_as(C.POINTER(C.c_int32)), st.ctypes.data_as(C.POINTER(C.c_float)),
                                         out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 1 and (out == -7.25).all()                                    # a window without a state
    G.step_begin()
    with pytest.raises(capi.HlError) as e:
        G.forward_sequences(wins[:2])
    assert e.value.status == 4                                                 # HL_ERR_STATE
    G.step_end()
    assert np.array_equal(G.forward_sequences(wins[:4]), G.forward_sequences(wins[:4]))
    G.close()


# ---- 6. the window kernels' resources (no GPU) ------------------------------------------------------------------------------------------
def test_no_scratch_and_no_spill_in_the_window_forward_kernels():
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = [k for k in resource_usage.kernels().get("rec.hip", []) if k["name"].split("<")[0] in WINDOW_KERNELS]
    for kernel in WINDOW_KERNELS:      # the form with the per-agent tables and the one without, at least
        assert sum(k["name"].split("<")[0] == kernel for k in rows) >= 2, "no resource remarks of %s beside the objects" % kernel
    for k in rows:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
