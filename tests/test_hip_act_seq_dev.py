"""Recurrent acting from device memory (hl_forward_sequences_dev, hl_select_actions_sequences_dev of include/smarties_hip_dev.h;
smarties_amd/csrc/learner_dev.h, actseq.hip, actdev.hip), on the GPU: the device call against hl_forward_sequences bit for bit and
against the CPU oracle agent by agent, for ragged windows laid out packed and as columns of a [T][nEnv] buffer written on a side stream
right before the call; the truncation of long windows; a dense net with appended observations; the training path left untouched; the
refusals; and a closed loop act -> simulate -> append -> step of an LSTM on tensors against the same loop through the host-pointer calls."""
import numpy as np
import pytest

from acting import (FALLBACK, TOL32, _call_dev, _columns, _packed, _pair, _ragged, _rec_cfg, _same_replay, _same_training_state, _side_stream,
                    _synth_learner as _learner, head_np)
from oracle_api import synth_cfg
from parity import COL_ROWS, assert_columns, relinf, twin64
from smarties_amd import capi

BPTT = 8
SYNTH = dict(seed=43, dimS=6, dimA=2, lenMin=5, lenMax=40, pTerm=0.5)
SHAPES = [(capi.NN_LSTM, (32, 32), 0), (capi.NN_MGU, (24, 16, 8), 0), (capi.NN_RNN, (24, 16), 0), (capi.NN_LSTM, (32, 32), 2),
          (capi.NN_LSTM, (128, 32), 0)]      # the last: the weights-through-L2 variant
IDS = ["lstm-2x32", "mgu-24x16x8", "rnn-24x16", "lstm-2x32-app2", "lstm-128x32"]


# ---- 1. bit identity with the host call, parity with the oracle -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,hidden,nApp", SHAPES, ids=IDS)
def test_windows_from_device_memory_equal_the_host_call_bit_for_bit(hip_api, kind, hidden, nApp):
    import torch
    G, O = _pair(hip_api, _rec_cfg(kind, hidden, nApp, BPTT), synth_cfg(**SYNTH), 40)
    G.step(5); O.step(5)
    rng = np.random.default_rng(11)
    wins = _ragged(rng, 300, 6, [1, 2, 5, BPTT + 1] + ([BPTT + 1 + nApp] if nApp else []))      # 300 agents: more than compute units
    ref = np.stack([O.forward_sequence(w) for w in wins])
    T = twin64(O)
    ref64 = np.stack([T.forward_sequence(w) for w in wins])
    host = G.forward_sequences(wins)
    side = _side_stream()
    perm = rng.permutation(300)
    for layout in (_packed(wins), _columns(wins)):
        for n in (1, 3, 300):
            got = _call_dev(G, side, layout, np.arange(n))
            assert got.shape == (n, G.nOut)
            assert np.array_equal(got, G.forward_sequences(wins[:n])), (layout[3], n)
            assert np.array_equal(got, host[:n]), (layout[3], n)
            for i in range(n):
                assert relinf(got[i], ref[i]) < TOL32, (layout[3], n, i, wins[i].shape[0], got[i], ref[i])
            if n >= COL_ROWS:
                assert_columns(got, ref64[:n], TOL32, (layout[3], n), ref[:n])
        # the agents in another order: an agent's result does not depend on its place in the batch
        got = _call_dev(G, side, layout, perm)
        assert np.array_equal(got, host[perm]), layout[3]
        for q, i in enumerate(perm):
            assert relinf(got[q], ref[i]) < TOL32, (layout[3], q, i)
        assert_columns(got, ref64[perm], TOL32, (layout[3], "permuted"), ref[perm])
    empty = torch.empty(0, dtype=torch.int64, device="cuda"), torch.empty(0, dtype=torch.int32, device="cuda")
    assert G.forward_sequences_dev(torch.empty((0, 6), dtype=torch.float32, device="cuda"), empty[0], empty[1], 1).shape == (0, G.nOut)


# ---- 2. truncation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nApp", [0, 2])
def test_long_windows_are_truncated_to_their_newest_states(hip_api, nApp):
    import torch
    G = _learner(hip_api, _rec_cfg(capi.NN_LSTM, (32, 32), nApp, BPTT), SYNTH)
    G.step(2)
    top = BPTT + 1 + nApp
    rng = np.random.default_rng(5)
    wins = _ragged(rng, 6, 6, [top + 7, top + 1, top, 3, top + 7, 4])
    host = G.forward_sequences([w[-top:] for w in wins])
    side = _side_stream()
    for layout in (_packed(wins), _columns(wins)):
        assert np.array_equal(_call_dev(G, side, layout, np.arange(6)), host), layout[3]
        # n_steps below 1 reads one row: the first
        states, first, n_steps, stride = layout
        for none in (0, -4):
            got = _call_dev(G, side, (states, first, np.where(np.arange(6) % 2 == 0, none, n_steps).astype(np.int32), stride), np.arange(6))
            assert np.array_equal(got, G.forward_sequences([w[:1] if i % 2 == 0 else w[-top:] for i, w in enumerate(wins)])), (layout[3], none)


# ---- 3. a dense net with appended observations --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dense_net_with_appended_observations(hip_api):
    import torch
    kw, sc_kw = FALLBACK["dense-app3"]      # hidden 24, 16, 8; dimS 9; nAppendedObs 3
    G = _learner(hip_api, kw, sc_kw)
    G.step(3)
    rng = np.random.default_rng(3)
    wins = _ragged(rng, 70, 9, [1, 2, 5, 9, 3])      # 70 agents: the row-block kernel; 5: a workgroup per row
    side = _side_stream()
    for layout in (_packed(wins), _columns(wins)):
        for n in (5, 70):
            got = _call_dev(G, side, layout, np.arange(n))
            assert np.array_equal(got, G.forward_sequences(wins[:n])), (layout[3], n)
    # the head behind it: the row calls on the stacked rows run the same kernels
    rows = np.stack([np.concatenate([w[max(len(w) - 1 - j, 0)] for j in range(4)]) for w in wins])
    noise = torch.from_numpy(np.clip(rng.normal(size=(70, 3)), -2, 2)).cuda()
    got = _call_dev(G, side, _columns(wins), np.arange(70), select=noise)
    ref = G.select_actions_dev(torch.from_numpy(rows).cuda(), noise)
    for g, r in zip(got, ref):
        assert np.array_equal(g, r.cpu().numpy())


# ---- 4. training is untouched -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,hidden", [(capi.NN_LSTM, (32, 32)), (capi.NN_MGU, (24, 16, 8))], ids=["lstm-2x32", "mgu-24x16x8"])
def test_acting_from_device_memory_leaves_training_untouched(hip_api, kind, hidden):
    """One learner acts between its steps -- where the next minibatch is already drawn -- and its twin never does: weights, both moments,
    generator state and beta stay equal, eager steps and the replayed-graph form."""
    import torch
    A, B = [_learner(hip_api, _rec_cfg(kind, hidden), SYNTH) for _ in range(2)]
    rng = np.random.default_rng(2)
    wins = _ragged(rng, 70, 6, [1, 4, 9, 14])
    side = _side_stream()
    layout = _columns(wins)
    noise = torch.from_numpy(np.clip(rng.normal(size=(70, 2)), -2, 2)).cuda()

    def act():
        assert np.isfinite(_call_dev(A, side, layout, np.arange(70))).all()
        assert all(np.isfinite(x).all() for x in _call_dev(A, side, layout, np.arange(70), select=noise))

    for _ in range(3):
        A.step(1); B.step(1)
        act()
    A.step(4); B.step(4)
    _same_training_state(A, B)
    A.prepare_steps(3); B.prepare_steps(3)
    for _ in range(2):
        A.step(3); B.step(3)
        act()
    A.step(3); B.step(3)
    _same_training_state(A, B)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lstm-512", "conv-lstm", "rnn-encoder-mgu"])
def test_nets_beyond_the_batched_kernel_are_refused(hip_api, name):
    import torch
    L = _learner(hip_api, FALLBACK[name][0], None, n_eps=0)
    st = torch.zeros((4, L.dS), dtype=torch.float32, device="cuda")
    first, steps = torch.arange(3, dtype=torch.int64, device="cuda"), torch.ones(3, dtype=torch.int32, device="cuda")
    for call in (L.forward_sequences_dev, L.select_actions_sequences_dev):
        with pytest.raises(capi.HlError) as e:
            call(st, first, steps, 1)
        assert e.value.status == 8                            # HL_ERR_UNSUPPORTED
        assert "hl_forward_sequences" in str(e.value)
    # the row calls keep refusing recurrent nets
    with pytest.raises(capi.HlError) as e:
        L.forward_dev(torch.zeros((3, L.dIn), dtype=torch.float32, device="cuda"))
    assert e.value.status == 8


@pytest.mark.gpu
def test_bad_arguments_state_and_tensors_are_refused(hip_api):
    import torch
    G = _learner(hip_api, _rec_cfg(capi.NN_LSTM, (32, 32)), SYNTH)
    st = torch.zeros((12, 6), dtype=torch.float32, device="cuda")
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
    with pytest.raises(ValueError):
        G.forward_sequences_dev(st.cpu(), first, steps, 3)                    # not on the GPU
    with pytest.raises(ValueError):
        G.forward_sequences_dev(st, first.cpu(), steps, 3)
    with pytest.raises(TypeError):
        G.forward_sequences_dev(st.double(), first, steps, 3)                 # dtype
    with pytest.raises(TypeError):
        G.forward_sequences_dev(st, first.int(), steps, 3)
    with pytest.raises(TypeError):
        G.forward_sequences_dev(st, first, steps.long(), 3)
    with pytest.raises(ValueError):
        G.forward_sequences_dev(torch.zeros((12, 12), dtype=torch.float32, device="cuda")[:, :6], first, steps, 3)      # not contiguous
    with pytest.raises(ValueError):
        G.forward_sequences_dev(st, torch.arange(6, dtype=torch.int64, device="cuda")[::2], steps, 3)
    G.step_begin()
    for call in (G.forward_sequences_dev, G.select_actions_sequences_dev):
        with pytest.raises(capi.HlError) as e:
            call(st, first, steps, 3)
        assert e.value.status == 4                            # HL_ERR_STATE
    G.step_end()
    assert torch.isfinite(G.forward_sequences_dev(st, first, steps, 3)).all()      # (behind the gradient step: other weights)


# ---- 6. the loop --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_recurrent_loop_on_tensors_equals_loop_through_host_pointers(hip_api):
    import torch
    bptt, nEnv, L, dS, dA = 3, 4, 6, 6, 2      # episodes of 6 steps: longer than the window of bptt + 1 states
    kw = dict(dimS=dS, dimA=dA, bounded=[1, 0], hidden=(16, 16), nnFunc="Tanh", batchSize=8, maxTotObsNum=4000, randSeed=5,
              nn_type=capi.NN_LSTM, nnBPTTseq=bptt)
    H, D = [_learner(hip_api, kw, dict(seed=21, dimS=dS, dimA=dA, lenMin=5, lenMax=30, pTerm=0.5), n_eps=10) for _ in range(2)]
    rng = np.random.default_rng(9)
    noise = np.clip(rng.normal(size=(20, L, nEnv, dA)), -2, 2)
    dev = "cuda"
    M = torch.from_numpy((rng.normal(size=(dS, dS)) * 0.4).astype(np.float32)).to(dev)
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

    for it in range(20):
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
