"""Acting from device memory for recurrent nets on wide inputs (hl_forward_sequences_dev, hl_select_actions_sequences_dev of
include/smarties_hip_dev.h; smarties_amd/csrc/learner_dev.h: devSeqTmForward, rectm.hip: lstm_tm_prepare_acts_dev_kernel), on the GPU:
the device call against hl_forward_sequences bit for bit and against the CPU oracle agent by agent, for ragged windows laid out packed
and as columns of a [T][nEnv] buffer written on a side stream right before the call, over several chunks of the local batch; the
truncation of long windows; calls without a full window and on rows a longer window left behind; a states tensor off a 16-byte boundary;
the heads; the training path left untouched; a closed loop act -> simulate -> append -> step on tensors against the same loop through
the host-pointer calls; the refusals of bad arguments."""
import numpy as np
import pytest

from acting import (N_AGENTS, TOL32, WIDE_IDS as _IDS, WIDE_SHAPES as SHAPES, _call_dev, _check_heads, _columns, _packed, _pair, _ragged,
                    _same_replay, _same_training_state, _side_stream, _wide_cfg as _cfg, head_np)
from oracle_api import fill_synth, synth_cfg
from parity import COL_ROWS, assert_columns, relinf, twin64
from smarties_amd import capi

pytestmark = pytest.mark.gpu

MGU = SHAPES[1]


def _synth(dS, dA=2):
    return synth_cfg(seed=21, dimS=dS, dimA=dA, lenMin=2, lenMax=30, pTerm=0.5)


def _learner(hip_api, kw, n_eps=60):
    L = capi.Learner(hip_api, capi.make_config(**kw))
    L.init_weights()
    if n_eps:
        fill_synth(L, _synth(kw["dimS"], kw["dimA"]), n_eps)
        L.initialize()
    return L


# ---- 1. bit identity with the host call, parity with the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_wide_windows_from_device_memory_equal_the_host_call_bit_for_bit(hip_api, shape):
    """(on the commit before the route: HlError, status 8, from the first device call)"""
    import torch
    kind, hidden, dS, nApp, bptt, batch = shape
    G, O = _pair(hip_api, _cfg(shape), _synth(dS), 60)
    G.step(3); O.step(3)
    rng = np.random.default_rng(11)
    nAll = 5 * batch // 2 + 1                                    # 2.5 x batch + 1 agents: three chunks, the last partial
    wins = _ragged(rng, nAll, dS, sorted({1, 2, bptt + 1, bptt + 1 + nApp}))
    ref = np.stack([O.forward_sequence(w) for w in wins])
    T = twin64(O)
    ref64 = np.stack([T.forward_sequence(w) for w in wins])
    host = G.forward_sequences(wins)
    side = _side_stream()
    perm = rng.permutation(nAll)
    for layout in (_packed(wins), _columns(wins)):
        for n in (1, 3, nAll):
            got = _call_dev(G, side, layout, np.arange(n))
            assert got.shape == (n, G.nOut)
            assert np.array_equal(got, G.forward_sequences(wins[:n])), (layout[3], n)
            for i in range(n):
                assert relinf(got[i], ref[i]) < TOL32, (layout[3], n, i, wins[i].shape[0], got[i], ref[i])
            if n >= COL_ROWS:
                assert_columns(got, ref64[:n], TOL32, (layout[3], n), ref[:n])
        # the agents in another order: an agent's result does not depend on its chunk or its row in it
        got = _call_dev(G, side, layout, perm)
        assert np.array_equal(got, host[perm]), layout[3]
        for q, i in enumerate(perm):
            assert relinf(got[q], ref[i]) < TOL32, (layout[3], q, i)
        if nAll >= COL_ROWS:
            assert_columns(got, ref64[perm], TOL32, (layout[3], "permuted"), ref[perm])
    G.close()


# ---- 2. truncation ------------------------------------------------------------------------------------------------------------------------
def test_long_wide_windows_are_truncated_to_their_newest_states(hip_api):
    kind, hidden, dS, nApp, bptt, batch = MGU
    G = _learner(hip_api, _cfg(MGU))
    G.step(2)
    top = bptt + 1 + nApp
    rng = np.random.default_rng(5)
    wins = _ragged(rng, 6, dS, [top + 7, top + 1, top, 3, top + 7, 4])
    host = G.forward_sequences([w[-top:] for w in wins])
    side = _side_stream()
    for layout in (_packed(wins), _columns(wins)):
        assert np.array_equal(_call_dev(G, side, layout, np.arange(6)), host), layout[3]
        # n_steps below 1 reads one row: the first
        states, first, n_steps, stride = layout
        for none in (0, -4):
            got = _call_dev(G, side, (states, first, np.where(np.arange(6) % 2 == 0, none, n_steps).astype(np.int32), stride), np.arange(6))
            assert np.array_equal(got, G.forward_sequences([w[:1] if i % 2 == 0 else w[-top:] for i, w in enumerate(wins)])), (layout[3], none)
    G.close()


# ---- 3. no full window, and stale rows ------------------------------------------------------------------------------------------------------
def test_short_windows_alone_and_on_rows_longer_windows_left(hip_api):
    """The chain runs nnBPTTseq + 1 steps whatever the windows are: a call whose agents all have 1 - 2 states has no agent in its later
    steps; right behind a call with full windows the chunk's rows of those steps hold that call's inputs and recurrent slots, which
    nothing of the short windows may read."""
    kind, hidden, dS, nApp, bptt, batch = MGU
    G = _learner(hip_api, _cfg(MGU))
    G.step(2)
    rng = np.random.default_rng(8)
    n = batch + 3                                                # two chunks
    short = _ragged(rng, n, dS, [1, 2])
    full = _ragged(rng, n, dS, [bptt + 1 + nApp])
    want = G.forward_sequences(short)
    side = _side_stream()
    assert np.array_equal(_call_dev(G, side, _columns(short), np.arange(n)), want)
    assert np.array_equal(_call_dev(G, side, _packed(full), np.arange(n)), G.forward_sequences(full))
    assert np.array_equal(_call_dev(G, side, _packed(short), np.arange(n)), want)
    # ... and with NaN in every state of the longer windows' call
    _call_dev(G, side, _packed([np.full_like(w, np.nan) for w in full]), np.arange(n))
    assert np.array_equal(_call_dev(G, side, _columns(short), np.arange(n)), want)
    G.close()


# ---- 4. alignment -------------------------------------------------------------------------------------------------------------------------
def test_states_off_a_16_byte_boundary_give_the_same_bits(hip_api):
    import torch
    kind, hidden, dS, nApp, bptt, batch = MGU
    G = _learner(hip_api, _cfg(MGU))
    G.step(2)
    rng = np.random.default_rng(4)
    wins = _ragged(rng, 7, dS, [1, 3, bptt + 1, bptt + 1 + nApp])
    states, first, n_steps, stride = _columns(wins)
    st = torch.from_numpy(states).cuda()
    big = torch.zeros(states.size + 4, dtype=torch.float32, device="cuda")
    assert big.data_ptr() % 16 == 0
    off = big[1:1 + states.size].view(states.shape)
    off.copy_(st)
    assert off.data_ptr() % 16 == 4 and st.data_ptr() % 16 == 0
    f, s = torch.from_numpy(first).cuda(), torch.from_numpy(n_steps).cuda()
    a = G.forward_sequences_dev(st, f, s, stride).cpu().numpy()
    b = G.forward_sequences_dev(off, f, s, stride).cpu().numpy()
    assert np.array_equal(a, b)
    assert np.array_equal(a, G.forward_sequences(wins))
    G.close()


# ---- 5. the heads -------------------------------------------------------------------------------------------------------------------------
HEADS = {
    "gaussian": _cfg(SHAPES[0]),
    "discrete": _cfg(SHAPES[0], dimA=1, bounded=[0], adv_kind=capi.ADV_DISCRETE, n_options=5),
}


@pytest.mark.parametrize("name", list(HEADS))
def test_heads_on_wide_windows_match_numpy_restatement(hip_api, name):
    import torch
    kw = HEADS[name]
    G = _learner(hip_api, kw)
    G.step(2)
    rng = np.random.default_rng(17)
    dS, dA, nOpt = kw["dimS"], kw["dimA"], kw.get("n_options", 0)
    wins = _ragged(rng, N_AGENTS, dS, [1, 2, 4])
    layout = _columns(wins)
    side = _side_stream()
    O = _call_dev(G, side, layout, np.arange(N_AGENTS))          # the head reads the device call's own outputs
    assert np.array_equal(O, G.forward_sequences(wins))
    noise = rng.uniform(size=N_AGENTS) if nOpt else np.clip(rng.normal(size=(N_AGENTS, dA)), -2, 2)
    got = _call_dev(G, side, layout, np.arange(N_AGENTS), select=torch.from_numpy(noise).cuda())
    _check_heads(kw, O, noise, [torch.from_numpy(x) for x in got])
    states, first, n_steps, stride = layout
    got = G.select_actions_sequences_dev(torch.from_numpy(states).cuda(), torch.from_numpy(first).cuda(), torch.from_numpy(n_steps).cuda(), stride, None)
    _check_heads(kw, O, None, got)                               # the evaluation action
    G.close()


# ---- 6. training is untouched -------------------------------------------------------------------------------------------------------------
def test_acting_on_wide_windows_leaves_training_untouched(hip_api):
    """One learner acts between its steps -- where the next minibatch is already drawn -- and its twin never does: weights, both moments,
    generator state, beta and the replay stay equal, eager steps and the replayed-graph form."""
    import torch
    kind, hidden, dS, nApp, bptt, batch = MGU
    A, B = [_learner(hip_api, _cfg(MGU)) for _ in range(2)]
    rng = np.random.default_rng(2)
    n = 2 * batch + 5
    wins = _ragged(rng, n, dS, [1, 4, bptt + 1, bptt + 1 + nApp])
    side = _side_stream()
    layout = _columns(wins)
    noise = torch.from_numpy(np.clip(rng.normal(size=(n, 2)), -2, 2)).cuda()

    def act():
        assert np.isfinite(_call_dev(A, side, layout, np.arange(n))).all()
        assert all(np.isfinite(x).all() for x in _call_dev(A, side, layout, np.arange(n), select=noise))

    for _ in range(2):
        A.step(1); B.step(1)
        act()
    A.step(2); B.step(2)
    _same_training_state(A, B)
    A.prepare_steps(2); B.prepare_steps(2)
    for _ in range(2):
        A.step(2); B.step(2)                                     # replayed steps: the captured graph
        act()
    A.step(2); B.step(2)
    _same_training_state(A, B)
    _same_replay(A, B)
    A.close(); B.close()


# ---- 7. the loop --------------------------------------------------------------------------------------------------------------------------
def test_wide_recurrent_loop_on_tensors_equals_loop_through_host_pointers(hip_api):
    import torch
    bptt, nEnv, L, dS, dA = 3, 4, 6, 257, 2      # episodes of 6 steps: longer than the window of bptt + 1 states
    kw = _cfg(SHAPES[0], batchSize=8, maxTotObsNum=4000, adv_kind=capi.ADV_ZERO)      # (the head of the existing closed loops)
    H, D = [_learner(hip_api, kw, n_eps=10) for _ in range(2)]
    nIt = 8                                      # 8 x 6 act calls and 8 gradient steps
    rng = np.random.default_rng(9)
    noise = np.clip(rng.normal(size=(nIt, L, nEnv, dA)), -2, 2)
    dev = "cuda"
    M = torch.from_numpy((rng.normal(size=(dS, dS)) * (0.4 / np.sqrt(dS / 6))).astype(np.float32)).to(dev)
    K = torch.from_numpy((rng.normal(size=(dA, dS)) * 0.3).astype(np.float32)).to(dev)
    s0 = torch.from_numpy(rng.normal(size=(nEnv, dS)).astype(np.float32)).to(dev)
    noise_d = torch.from_numpy(noise).to(dev)
    first = torch.arange(nEnv, dtype=torch.int64, device=dev)      # the episodes start in row 0 of the buffer: first_row = 0 * nEnv + env
    steps = [torch.full((nEnv,), t + 1, dtype=torch.int32, device=dev) for t in range(L)]

    def simulate(s, a):      # the "simulator": a linear map on the device, the same launch for both loops
        nxt = torch.tanh(s @ M + a.float() @ K)
        return nxt, -(nxt.double() ** 2).sum(dim=1)

    def buffers():
        return (torch.zeros((L + 1, nEnv, dS), dtype=torch.float32, device=dev), torch.zeros((L + 1, nEnv, dA), dtype=torch.float64, device=dev),
                torch.zeros((L + 1, nEnv, 2 * dA), dtype=torch.float64, device=dev), torch.zeros((L + 1, nEnv), dtype=torch.float64, device=dev),
                torch.zeros((L + 1, nEnv), dtype=torch.float32, device=dev), torch.zeros((L + 1, nEnv), dtype=torch.float32, device=dev))

    for it in range(nIt):
        # on tensors: the episode's start row and t + 1 -- the kernel truncates --, no state, action or value leaves the device
        S, A, MU, R, V, ADV = buffers()
        S[0] = s0
        for t in range(L):
            D.select_actions_sequences_dev(S, first, steps[t], nEnv, noise_d[it, t], out=(A[t], MU[t], V[t], ADV[t]))
            S[t + 1], R[t + 1] = simulate(S[t], A[t])
        D.append_episodes_dev([L + 1] * nEnv, [1] * nEnv, [1000 + it * nEnv + e for e in range(nEnv)], list(range(nEnv)), nEnv, S, A, MU, R, V, ADV)
        D.step(1)
        # through the host pointers: hl_forward_sequences on the truncated windows, the head on the host, hl_append_episode per episode
        Sh, Ah, MUh, Rh, Vh, ADVh = buffers()
        Sh[0] = s0
        for t in range(L):
            hist = Sh[max(0, t - bptt):t + 1].cpu().numpy()
            O = H.forward_sequences([hist[:, e] for e in range(nEnv)])
            for e in range(nEnv):
                a, mu, v, adv = head_np(O[e], noise[it, t, e], dA, kw["bounded"])
                Ah[t, e], MUh[t, e] = torch.from_numpy(a), torch.from_numpy(mu)
                Vh[t, e], ADVh[t, e] = float(v), float(adv)
            Sh[t + 1], Rh[t + 1] = simulate(Sh[t], Ah[t])
        host = [x.cpu().numpy() for x in (Sh, Ah, MUh, Rh, Vh, ADVh)]
        for e in range(nEnv):
            H.append_episode(host[0][:, e], host[1][:, e], host[2][:, e], host[3][:, e], host[4][:, e], 1, 1000 + it * nEnv + e, advantages=host[5][:, e])
        H.step(1)
        assert torch.equal(S, Sh) and torch.equal(A, Ah) and torch.equal(V, Vh), it
        s0 = S[L].clone()
    _same_training_state(H, D)
    _same_replay(H, D)
    H.close(); D.close()


# ---- 8. bad arguments and state -----------------------------------------------------------------------------------------------------------
def test_bad_arguments_and_state_are_refused_on_a_wide_net(hip_api):
    import ctypes as C
    import torch
    G = _learner(hip_api, _cfg(SHAPES[0]))
    st = torch.zeros((12, 257), dtype=torch.float32, device="cuda")
    first, steps = torch.arange(3, dtype=torch.int64, device="cuda"), torch.full((3,), 4, dtype=torch.int32, device="cuda")
    good = G.forward_sequences_dev(st, first, steps, 3)
    assert torch.isfinite(good).all()
    for call in (G.forward_sequences_dev, G.select_actions_sequences_dev):
        with pytest.raises(capi.HlError) as e:
            call(st, first, steps, 0)
        assert e.value.status == 1                            # HL_ERR_BAD_ARG: row_stride below 1
        with pytest.raises(capi.HlError) as e:
            call(st, first, steps, 3, n=-1, out=good if call == G.forward_sequences_dev else (good, good, st, st))
        assert e.value.status == 1
    ptr = lambda t: C.c_void_p(t.data_ptr())
    fwd = G.api.fn("forward_sequences_dev")
    assert fwd(G.h, 3, None, ptr(steps), 3, ptr(st), ptr(good), None) == 1      # a null array
    assert fwd(G.h, 3, ptr(first), None, 3, ptr(st), ptr(good), None) == 1
    assert fwd(G.h, 3, ptr(first), ptr(steps), 3, None, ptr(good), None) == 1
    assert fwd(G.h, 3, ptr(first), ptr(steps), 3, ptr(st), None, None) == 1
    empty = torch.empty(0, dtype=torch.int64, device="cuda"), torch.empty(0, dtype=torch.int32, device="cuda")
    assert G.forward_sequences_dev(torch.empty((0, 257), dtype=torch.float32, device="cuda"), empty[0], empty[1], 1).shape == (0, G.nOut)
    G.step_begin()
    for call in (G.forward_sequences_dev, G.select_actions_sequences_dev):
        with pytest.raises(capi.HlError) as e:
            call(st, first, steps, 3)
        assert e.value.status == 4                            # HL_ERR_STATE
    G.step_end()
    assert torch.isfinite(G.forward_sequences_dev(st, first, steps, 3)).all()      # (behind the gradient step: other weights)
    G.close()
