"""hl_forward_sequences for nets with recurrent layers wider than 256 cells (include/smarties_hip_act.h): the agents of a chunk are the
sample rows of ONE chain of time-step-major launches (smarties_amd/csrc/rectm.hip: lstm_tm_prepare_acts_kernel, the forward diagonals,
act_output_kernel), a chunk holding min(batchSize, ACT_SEQ_CHUNK) agents.

GPU suite: every agent bit for bit against the library's own single-agent hl_forward_sequence and within TOL32 of the CPU oracle, in any
order of the agents; rows left by a longer window of the chunk before; one chain per chunk; training untouched; refusals.
CPU suite (the last test): the prepare kernel exists and uses no scratch memory.

The shapes are the smallest at which each piece can go wrong (nets built as in test_hip_rnn_wide.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from acting import TOL32, _compare_step, _pair, _ragged as _windows
from oracle_api import synth_cfg, fill_synth
from parity import COL_ROWS, assert_columns, relinf, twin64
from smarties_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREPARE_KERNEL = "lstm_tm_prepare_acts_kernel"

SHAPES = {  # name: (nnType, hidden, dimS, nAppendedObs, nnBPTTseq, batchSize, agents)
    # a chunk smaller than a 16-row tile, four chunks with the last one partial (6, 6, 6, 2), an odd number of cell tiles
    "lstm-272": (capi.NN_LSTM, (272,), 7, 0, 3, 6, 20),
    # per-agent context states for appended observations, parametric residual, two-tile workgroups
    "rnn-320x272-app2": (capi.NN_RNN, (320, 272), 9, 2, 4, 12, 30),
    # both MGU phases, a partial second row block (16 + 4), chunks of 20, 20 and 5, wide and narrow layers mixed
    "mgu-272x96": (capi.NN_MGU, (272, 96), 6, 0, 5, 20, 45),
    # one chunk, three row blocks (16, 16, 8)
    "lstm-512": (capi.NN_LSTM, (512,), 7, 0, 3, 40, 40),
    # the largest staged A tile the predicate admits
    "rnn-2x1024": (capi.NN_RNN, (1024, 1024), 5, 0, 2, 4, 9),
}


def _cfg(name):
    kind, hidden, dS, nApp, bptt, batch, _ = SHAPES[name]
    return dict(dimS=dS, dimA=2, bounded=[1, 0], hidden=hidden, nnFunc="Tanh", batchSize=batch, maxTotObsNum=8000, randSeed=5,
                nn_type=kind, adv_kind=capi.ADV_GAUSSIAN, nnBPTTseq=bptt, nAppendedObs=nApp)


def _synth(name):
    return synth_cfg(seed=21, dimS=SHAPES[name][2], dimA=2, lenMin=2, lenMax=30, pTerm=0.5)


def _ragged_lengths(name):
    _, _, _, nApp, bptt, _, _ = SHAPES[name]
    return [1, 2, bptt + 1, 3] + ([bptt + 1 + nApp, bptt + 2] if nApp else [])


@pytest.fixture(scope="module")
def nets(hip_api):
    """name -> (G, O) after three training steps (the weights are not the initial ones), built once; the tests that share a pair only act"""
    made = {}

    def get(name):
        if name not in made:
            G, O = _pair(hip_api, _cfg(name), _synth(name), 60)
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
    dS, agents = SHAPES[name][2], SHAPES[name][6]
    rng = np.random.default_rng(11)
    wins = _windows(rng, agents, dS, _ragged_lengths(name))
    out = G.forward_sequences(wins)
    one = [G.forward_sequence(w) for w in wins]
    assert out.shape == (agents, G.nOut)
    for i, w in enumerate(wins):
        assert np.array_equal(out[i], one[i]), (name, i, w.shape[0], out[i], one[i])
        assert relinf(out[i], O.forward_sequence(w)) < TOL32, (name, i, w.shape[0])
    if agents >= COL_ROWS:
        T = twin64(O)
        assert_columns(out, np.stack([T.forward_sequence(w) for w in wins]), TOL32, name)
    # the windows in another order: an agent's place, chunk and row block do not matter
    perm = rng.permutation(agents)
    out2 = G.forward_sequences([wins[i] for i in perm])
    for q, i in enumerate(perm):
        assert np.array_equal(out2[q], one[i]), (name, q, i)


# ---- 2. rows left by the chunk before -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_longer_window_of_the_call_before_does_not_leak(nets):
    name = "mgu-272x96"
    G, _ = nets(name)
    _, _, dS, _, bptt, _, agents = SHAPES[name]
    rng = np.random.default_rng(12)
    for what, lengths in (("full", [bptt + 1]), ("one state", [1]), ("mixed", [2, bptt + 1, 1, 4])):
        wins = _windows(rng, agents, dS, lengths)
        _assert_single_agent_bits(G, wins, G.forward_sequences(wins), what)


# ---- 3. one chain per chunk -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_chain_of_launches_per_chunk(nets):
    name = "lstm-272"
    G, _ = nets(name)
    _, _, dS, _, _, batch, agents = SHAPES[name]
    rng = np.random.default_rng(13)
    wins = _windows(rng, agents, dS, _ragged_lengths(name))
    G.forward_sequences(wins[:2])
    G.timing_enable(True)
    try:
        s0 = G.timing_get("act_seq")[1]
        n0 = G.timing_get("act_tm_chain")[1]
        G.forward_sequences(wins[:batch])
        n1 = G.timing_get("act_tm_chain")[1]
        assert n1 - n0 == 1
        G.forward_sequences(wins)
        n2 = G.timing_get("act_tm_chain")[1]
        assert n2 - n1 == -(-agents // batch) == 4
        assert G.timing_get("act_seq")[1] == s0
    finally:
        G.timing_enable(False)


# ---- 4. training untouched ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lstm-512", "mgu-272x96"])
def test_batched_acting_leaves_training_untouched(hip_api, name):
    """The body of test_hip_act_batch.test_batched_acting_leaves_training_untouched: the chain borrows the training rows of the chunk's
    agents, a minibatch drawn ahead must stay as it is -- eager steps and the replayed-graph form."""
    _, _, dS, _, bptt, batch, _ = SHAPES[name]
    G, O = _pair(hip_api, _cfg(name), _synth(name), 60)
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
    name = "rnn-320x272-app2"
    _, _, dS, nApp, bptt, _, agents = SHAPES[name]
    G = capi.Learner(hip_api, capi.make_config(**_cfg(name)))
    G.init_weights(); fill_synth(G, _synth(name), 60); G.initialize()
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


# ---- 6. the prepare kernel's resources (no GPU) ------------------------------------------------------------------------------------------
def test_no_scratch_in_the_prepare_kernel():
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = [k for k in resource_usage.kernels().get("rectm.hip", []) if k["name"] == PREPARE_KERNEL]
    assert len(rows) == 1, "no resource remarks of %s beside the objects" % PREPARE_KERNEL
    assert rows[0]["scratch"] == 0 and rows[0]["vgpr_spill"] == 0, rows[0]
