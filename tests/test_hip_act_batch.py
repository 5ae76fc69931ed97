"""hl_forward_sequences (include/smarties_hip_act.h): the network evaluated for many agents' windows in one call.

GPU suite: every agent's outputs against the CPU oracle's ol_forward_sequence on that agent's window (and against the library's own
single-agent hl_forward_sequence), for the shapes the batched kernel (smarties_amd/csrc/actseq.hip) serves and for those that go
through the single-agent routes; the training path left untouched; refusals; one launch per chunk.
CPU suite (the last two tests): the exported symbol and the kernel's resource remarks."""
import os
import re
import sys

import numpy as np
import pytest

from acting import FALLBACK, TOL32, _compare_step, _pair, _ragged, _rec_cfg
from oracle_api import synth_cfg
from parity import COL_ROWS, assert_columns, relinf, twin64
from smarties_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


BATCHED = [(capi.NN_LSTM, (32, 32), 0), (capi.NN_MGU, (32, 32), 0), (capi.NN_LSTM, (24, 16), 0), (capi.NN_MGU, (24, 16, 8), 0),
           (capi.NN_RNN, (24, 16), 0), (capi.NN_LSTM, (32, 32), 2), (capi.NN_LSTM, (128, 32), 0)]


# ---- 1. parity with the oracle, agent by agent ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,hidden,nApp", BATCHED,
                         ids=["lstm-2x32", "mgu-2x32", "lstm-24x16", "mgu-24x16x8", "rnn-24x16", "lstm-2x32-app2", "lstm-128x32"])
def test_batched_acting_matches_oracle_per_agent(hip_api, kind, hidden, nApp):
    bptt = 8
    G, O = _pair(hip_api, _rec_cfg(kind, hidden, nApp, bptt), synth_cfg(seed=43, dimS=6, dimA=2, lenMin=5, lenMax=40, pTerm=0.5), 40)
    G.step(5); O.step(5)
    rng = np.random.default_rng(11)
    lengths = [1, 2, bptt + 1, 5] + ([bptt + 1 + nApp, bptt + 2] if nApp else [])
    wins = _ragged(rng, 300, 6, lengths)                    # 300 agents: more than the device has compute units
    ref = np.stack([O.forward_sequence(w) for w in wins])
    T = twin64(O)
    ref64 = np.stack([T.forward_sequence(w) for w in wins])
    one = np.stack([G.forward_sequence(w) for w in wins])
    for i in range(len(wins)):
        assert relinf(one[i], ref[i]) < TOL32, ("single-agent call", i, wins[i].shape[0])
    assert_columns(one, ref64, TOL32, "single-agent calls", ref)
    for n in (1, 3, 64, 300):
        out = G.forward_sequences(wins[:n])
        assert out.shape == (n, G.nOut)
        for i in range(n):
            assert relinf(out[i], ref[i]) < TOL32, (n, i, wins[i].shape[0], out[i], ref[i])
        if n >= COL_ROWS:
            assert_columns(out, ref64[:n], TOL32, n, ref[:n])
    # windows in another order: an agent's result does not depend on its place in the batch
    perm = rng.permutation(300)
    out = G.forward_sequences([wins[i] for i in perm])
    for q, i in enumerate(perm):
        assert relinf(out[q], ref[i]) < TOL32, (q, i)
    assert_columns(out, ref64[perm], TOL32, "permuted", ref[perm])


# ---- 2. shapes that go through the single-agent routes ------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FALLBACK))
def test_other_shapes_give_the_single_agent_answers(hip_api, name):
    kw, sc_kw = FALLBACK[name]
    G, O = _pair(hip_api, kw, synth_cfg(**sc_kw), 40)
    G.step(3); O.step(3)
    rng = np.random.default_rng(3)
    dS, nApp = kw["dimS"], kw.get("nAppendedObs", 0)
    top = kw.get("nnBPTTseq", 4) + 1
    wins = _ragged(rng, 5, dS, [1, 2, top, top + nApp, 3])
    out = G.forward_sequences(wins)
    for i, w in enumerate(wins):
        # (the same kernels on the same rows: the looped routes are hl_forward_sequence itself, the dense rows are independent
        # workgroups of hl_forward's kernel)
        assert np.array_equal(out[i], G.forward_sequence(w)), (name, i)
        if "nn_type" in kw:
            ref = O.forward_sequence(w)
        else:     # (the oracle's ol_forward_sequence reads a dense net's last state alone: its ol_forward gets the stacked row)
            ref = O.forward(np.concatenate([w[max(len(w) - 1 - j, 0)] for j in range(nApp + 1)])[None])[0]
        assert relinf(out[i], ref) < TOL32, (name, i)


# ---- 3. training is untouched -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,hidden", [(capi.NN_LSTM, (32, 32)), (capi.NN_MGU, (24, 16, 8))], ids=["lstm-2x32", "mgu-24x16x8"])
def test_batched_acting_leaves_training_untouched(hip_api, kind, hidden):
    """After a step the next minibatch is already drawn: acting in between must neither consume nor disturb it (same sample indices
    as the oracle in the following step), eager steps and the replayed-graph form."""
    G, O = _pair(hip_api, _rec_cfg(kind, hidden), synth_cfg(seed=43, dimS=6, dimA=2, lenMin=5, lenMax=40, pTerm=0.5), 40)
    rng = np.random.default_rng(2)
    wins = _ragged(rng, 70, 6, [1, 4, 9])
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


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nApp", [0, 2])
def test_batched_acting_refusals(hip_api, nApp):
    bptt = 8
    G, O = _pair(hip_api, _rec_cfg(capi.NN_LSTM, (32, 32), nApp, bptt), synth_cfg(seed=43, dimS=6, dimA=2, lenMin=5, lenMax=40, pTerm=0.5), 40)
    G.step(2)
    rng = np.random.default_rng(4)
    wins = _ragged(rng, 6, 6, [3, bptt + 1 + nApp])
    assert G.forward_sequences([]).shape == (0, G.nOut)                       # n = 0: HL_OK
    good = G.forward_sequences(wins)
    assert np.isfinite(good).all()
    wins[4] = rng.normal(size=(bptt + 2 + nApp, 6)).astype(np.float32)        # one window too long, in the middle of the batch
    out = np.full((6, G.nOut), -7.25)
    with pytest.raises(capi.HlError) as e:
        G.forward_sequences(wins, out=out)
    assert e.value.status == 1                                                # HL_ERR_BAD_ARG
    assert (out == -7.25).all()                                               # nothing written
    n_steps = np.array([3, 0], np.int32); st = np.zeros((3, 6), np.float32)
    import ctypes as C
    rc = hip_api.fn("forward_sequences")(G.h, 2, n_steps.ctypes.data_as(C.POINTER(C.c_int32)), st.ctypes.data_as(C.POINTER(C.c_float)),
                                         out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 1 and (out == -7.25).all()                                   # a window without a state
    G.step_begin()
    with pytest.raises(capi.HlError) as e:
        G.forward_sequences(wins[:2])
    assert e.value.status == 4                                                # HL_ERR_STATE
    G.step_end()
    assert np.array_equal(G.forward_sequences(wins[:4]), G.forward_sequences(wins[:4]))


# ---- 5. one launch per chunk --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_batched_acting_is_one_launch_per_chunk(hip_api):
    G, O = _pair(hip_api, _rec_cfg(capi.NN_LSTM, (32, 32)), synth_cfg(seed=43, dimS=6, dimA=2, lenMin=5, lenMax=40, pTerm=0.5), 40)
    G.step(2); O.step(2)
    rng = np.random.default_rng(6)
    wins = _ragged(rng, 2 * capi.ACT_SEQ_CHUNK + 40, 6, [9, 1, 5])
    G.forward_sequences(wins[:3])
    G.timing_enable(True)
    n0 = G.timing_get("act_seq")[1]
    out64 = G.forward_sequences(wins[:64])
    n1 = G.timing_get("act_seq")[1]
    assert n1 - n0 == 1
    out = G.forward_sequences(wins)
    n2 = G.timing_get("act_seq")[1]
    assert n2 - n1 == -(-len(wins) // capi.ACT_SEQ_CHUNK) == 3
    G.timing_enable(False)
    assert np.array_equal(out[:64], out64)
    for i in (0, capi.ACT_SEQ_CHUNK - 1, capi.ACT_SEQ_CHUNK, 2 * capi.ACT_SEQ_CHUNK, len(wins) - 1):      # both sides of the chunk borders
        assert relinf(out[i], O.forward_sequence(wins[i])) < TOL32, i
    T = twin64(O)
    assert_columns(out, np.stack([T.forward_sequence(w) for w in wins]), TOL32, "three chunks")


# ---- 6. surface and resources (no GPU) ------------------------------------------------------------------------------------------
def _act_header():
    return open(os.path.join(ROOT, "include", "smarties_hip_act.h")).read()


def test_library_exports_the_batched_acting_surface():
    import __graft_entry__ as ge
    ge.build_hip()
    syms = sorted(set(re.findall(r"HL_API\s+[\w\s\*]+?\b(hl_\w+)\s*\(", _act_header())))
    assert "hl_forward_sequences" in syms
    api = capi.load_hip()
    for s in syms:
        assert hasattr(api.lib, s), "libsmarties_hip.so does not export %s" % s
    assert api.has("forward_sequences")
    m = re.search(r"#define\s+HL_ACT_SEQ_CHUNK\s+(\d+)", _act_header())
    assert m and int(m.group(1)) == capi.ACT_SEQ_CHUNK


def test_no_scratch_in_the_batched_acting_kernels():
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = resource_usage.kernels().get("actseq.hip")
    assert rows, "no resource remarks of actseq.hip beside the objects"
    assert any(k["name"].startswith("act_seq_kernel") for k in rows)
    for k in rows:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
