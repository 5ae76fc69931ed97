"""Acting from device memory for feed-forward nets behind convolutions (hl_forward_sequences_dev, hl_select_actions_sequences_dev of
include/smarties_hip_dev.h; smarties_amd/csrc/actconv.hip: act_conv_dev_kernel, learner_dev.h: devSeqForward), on the GPU: the device
call against the host's hl_forward_sequences bit for bit and against the CPU oracle row by row, for ragged windows laid out packed and as
columns of a [T][nEnv] buffer written on a side stream right before the call; a states array that starts at no 16-byte boundary; the
launches; the heads; the training path left untouched; weights given without a step; the refusals; and a closed loop
act -> simulate -> append -> step on tensors with stacked frames against the same loop through the host-pointer calls."""
import numpy as np
import pytest

from acting import (ILL_COLUMNS, LDS_NETS, N_AGENTS, NETS, PARITY, TOL32, _bare, _call_dev, _check_heads, _columns, _conv_pair as _pair, _count,
                    _packed, _row_bytes, _rows, _same_replay, _same_training_state, _side_stream, _stacked, _training_forwards, _window_args,
                    head_np)
from parity import COL_ROWS, assert_columns, relinf, twin64
from smarties_amd import capi


def _lengths(nApp):
    """1, 2, nAppendedObs, nAppendedObs + 1 and 9 states: windows shorter than the stack (the first state repeats), exactly it, longer"""
    return [k for k in (1, 2, nApp, nApp + 1, 9) if k >= 1]


def _wins(rng, n, kw):
    lengths = _lengths(kw.get("nAppendedObs", 0))
    return [_rows(rng, lengths[i % len(lengths)], kw["dimS"]) for i in range(n)]


# ---- 1. bit identity with the host call, parity with the oracle -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_conv_windows_from_device_memory_equal_the_host_call_and_the_oracle(hip_api, name, monkeypatch):
    kw = NETS[name]
    nApp = kw.get("nAppendedObs", 0)
    monkeypatch.delenv("SMARTIES_HIP_GENERIC", raising=False)      # the device calls need no switch, whatever the row size
    G, O = _pair(hip_api, name)
    G.step(3); O.step(3)
    host = G
    if _row_bytes(kw) > capi.ACT_CONV_MAX_ROW_BYTES:      # (app3-extra, atari) hl_forward takes the conv route only with the switch held open: a twin
        monkeypatch.setenv("SMARTIES_HIP_GENERIC", "4096")
        host = _pair(hip_api, name, oracle=False)
        monkeypatch.delenv("SMARTIES_HIP_GENERIC")
        host.step(3)
        assert np.array_equal(host.get_params()[0], G.get_params()[0])
    ns = (1, 17) if name == "atari" else (1, 17, 300) + ((capi.ACT_ROWS_CHUNK + 1,) if name == "odd" else ())
    wins = _wins(np.random.default_rng(11), max(ns), kw)
    ref = O.forward(_stacked(wins, nApp))
    ref64 = twin64(O).forward(_stacked(wins, nApp))
    want = host.forward_sequences(wins)
    side = _side_stream()
    for n in ns:
        for layout in (_packed(wins[:n]), _columns(wins[:n])):
            got = _call_dev(G, side, layout, np.arange(n))
            assert got.shape == (n, G.nOut)
            assert np.array_equal(got, want[:n]), (name, layout[3], n)
            err = [relinf(got[i], ref[i]) for i in range(n)]
            worst = int(np.argmax(err))
            print("%s n=%d stride %d: worst row %d relinf %.3g" % (name, n, layout[3], worst, err[worst]))
            assert err[worst] < TOL32, (name, layout[3], n, worst, got[worst], ref[worst])
            if n >= COL_ROWS:
                assert_columns(got, ref64[:n], TOL32, (name, layout[3], n), ref[:n], cpu_bar=name in ILL_COLUMNS)


# ---- 2. alignment -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_states_one_float_into_a_buffer_give_the_same_bits(hip_api):
    import torch
    kw = NETS["app3"]
    G = _pair(hip_api, "app3", oracle=False)
    G.step(2)
    wins = _wins(np.random.default_rng(4), 40, kw)
    states, first, n_steps, stride = _columns(wins)
    first_d, steps_d = torch.from_numpy(first).cuda(), torch.from_numpy(n_steps).cuda()
    aligned = torch.from_numpy(states).cuda()
    big = torch.zeros(states.size + 5, dtype=torch.float32, device="cuda")
    shifted = big[1:1 + states.size].view(states.shape)
    shifted.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    a = G.forward_sequences_dev(aligned, first_d, steps_d, stride).cpu().numpy()
    b = G.forward_sequences_dev(shifted, first_d, steps_d, stride).cpu().numpy()
    assert np.array_equal(a, b)
    assert np.array_equal(a, G.forward_sequences(wins))


# ---- 3. launches --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_conv_launch_for_any_n_and_no_training_forward(hip_api):
    import torch
    kw = NETS["strided"]
    G = _pair(hip_api, "strided", oracle=False)
    G.step(2)
    nMax = 2 * capi.ACT_ROWS_CHUNK + 40
    st = torch.from_numpy(_rows(np.random.default_rng(6), nMax, kw["dimS"])).cuda()
    first, steps = torch.arange(nMax, dtype=torch.int64, device="cuda"), torch.ones(nMax, dtype=torch.int32, device="cuda")
    G.forward_sequences_dev(st, first[:3], steps[:3], 1)
    G.timing_enable(True)
    G.step(1)                                                   # (the training forward launches run under these names)
    fwd = _training_forwards(G)
    assert fwd[0] > 0 and fwd[1] > 0
    others = ("act_stack_dev", "act_conv", "act_rows", "conv_fwd0")
    before = [_count(G, k) for k in others]
    for n in (1, 65, capi.ACT_ROWS_CHUNK, nMax):
        c0, r0 = _count(G, "act_conv_dev"), _count(G, "act_rows_dev")
        G.forward_sequences_dev(st, first[:n], steps[:n], 1)
        torch.cuda.synchronize()
        assert _count(G, "act_conv_dev") - c0 == 1, n
        assert _count(G, "act_rows_dev") - r0 == -(-n // capi.ACT_ROWS_CHUNK), n
    assert [_count(G, k) for k in others] == before
    assert _training_forwards(G) == fwd
    G.timing_enable(False)


# ---- 4. the heads -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["strided", "extras6"])
def test_heads_behind_conv_windows_match_numpy_restatement(hip_api, name):
    import torch
    kw = NETS[name]
    G = _pair(hip_api, name, oracle=False)
    G.step(2)
    rng = np.random.default_rng(17)
    wins = _wins(rng, N_AGENTS, kw)
    side = _side_stream()
    layout = _columns(wins)
    O = _call_dev(G, side, layout, np.arange(N_AGENTS))
    nOpt = kw.get("n_options", 0)
    if nOpt:      # u at the midpoint of option (i mod nOpt)'s interval of the CDF, from the numpy probabilities
        noise = np.zeros(N_AGENTS)
        for i in range(N_AGENTS):
            c = np.concatenate([[0.0], np.cumsum(head_np(O[i], None, 1, n_options=nOpt)[1])])
            noise[i] = (c[i % nOpt] + c[i % nOpt + 1]) / 2
    else:
        noise = np.clip(rng.normal(size=(N_AGENTS, kw["dimA"])), -2, 2)
    got = _call_dev(G, side, layout, np.arange(N_AGENTS), select=torch.from_numpy(noise).cuda())
    _check_heads(kw, O, noise, [torch.from_numpy(x) for x in got])
    states, first, n_steps, stride = layout
    got = G.select_actions_sequences_dev(torch.from_numpy(states).cuda(), torch.from_numpy(first).cuda(),
                                         torch.from_numpy(n_steps).cuda(), stride, None)      # the evaluation action
    _check_heads(kw, O, None, got)


# ---- 5. training is untouched -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_conv_acting_from_device_memory_leaves_training_untouched(hip_api):
    """One learner acts between its steps -- where the next minibatch is already drawn -- and its twin never does: weights, both moments,
    generator state and beta stay equal, eager steps and the replayed-graph form."""
    import torch
    kw = NETS["strided"]
    A, B = [_pair(hip_api, "strided", oracle=False) for _ in range(2)]
    rng = np.random.default_rng(2)
    wins = _wins(rng, 70, kw)
    side = _side_stream()
    layout = _columns(wins)
    noise = torch.from_numpy(np.clip(rng.normal(size=(70, kw["dimA"])), -2, 2)).cuda()

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


# ---- 6. weights given without a step ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_given_weights_serve_device_windows_without_a_step(hip_api):
    kw = NETS["odd"]
    G, O = _pair(hip_api, "odd", weights=lambda L: np.random.default_rng(1).uniform(-0.1, 0.1, L.get_params()[0].shape).astype(np.float32))
    wins = _wins(np.random.default_rng(9), 20, kw)
    ref = O.forward(_stacked(wins, 0))
    got = _call_dev(G, _side_stream(), _columns(wins), np.arange(20))
    for i in range(20):
        assert relinf(got[i], ref[i]) < TOL32, (i, got[i], ref[i])
    assert_columns(got, twin64(O).forward(_stacked(wins, 0)), TOL32, "given weights", ref)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
def test_row_calls_keep_refusing_conv_nets_and_name_the_window_call(hip_api):
    import torch
    L = _bare(hip_api, NETS["strided"])
    st = torch.zeros((3, L.dIn), dtype=torch.float32, device="cuda")
    for call in (L.forward_dev, L.select_actions_dev):
        with pytest.raises(capi.HlError) as e:
            call(st)
        assert e.value.status == 8                            # HL_ERR_UNSUPPORTED
        assert "hl_forward_sequences_dev" in str(e.value)


@pytest.mark.gpu
def test_conv_nets_beyond_the_plan_are_refused(hip_api, monkeypatch):
    monkeypatch.delenv("SMARTIES_HIP_GENERIC", raising=False)
    L = _bare(hip_api, LDS_NETS["map-162K"])
    for call in (L.forward_sequences_dev, L.select_actions_sequences_dev):
        with pytest.raises(capi.HlError) as e:
            call(*_window_args(L), 1)
        assert e.value.status == 8
        assert "hl_forward" in str(e.value)
    monkeypatch.setenv("SMARTIES_HIP_GENERIC", "2")      # the route over the training buffers is asked for: no device route
    L = _bare(hip_api, NETS["strided"])
    monkeypatch.delenv("SMARTIES_HIP_GENERIC")
    for call in (L.forward_sequences_dev, L.select_actions_sequences_dev):
        with pytest.raises(capi.HlError) as e:
            call(*_window_args(L), 1)
        assert e.value.status == 8


@pytest.mark.gpu
def test_conv_window_calls_bad_arguments_and_state(hip_api):
    import torch
    G = _pair(hip_api, "odd", oracle=False)
    st, first, steps = _window_args(G)
    good = G.forward_sequences_dev(st, first, steps, 1)
    assert good.shape == (3, G.nOut) and torch.isfinite(good).all()
    for call in (G.forward_sequences_dev, G.select_actions_sequences_dev):
        with pytest.raises(capi.HlError) as e:
            call(st, first, steps, 0)
        assert e.value.status == 1                            # HL_ERR_BAD_ARG: row_stride below 1
    G.step_begin()
    for call in (G.forward_sequences_dev, G.select_actions_sequences_dev):
        with pytest.raises(capi.HlError) as e:
            call(st, first, steps, 1)
        assert e.value.status == 4                            # HL_ERR_STATE
    G.step_end()
    empty = torch.empty(0, dtype=torch.int64, device="cuda"), torch.empty(0, dtype=torch.int32, device="cuda")
    assert G.forward_sequences_dev(torch.empty((0, G.dS), dtype=torch.float32, device="cuda"), empty[0], empty[1], 1).shape == (0, G.nOut)
    assert torch.isfinite(G.forward_sequences_dev(st, first, steps, 1)).all()


# ---- 8. the loop --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_stacked_frame_loop_on_tensors_equals_loop_through_host_pointers(hip_api):
    """one frame per step in a [T][nEnv][dimS] buffer, first_row = env and n_steps = t + 1: the kernel stacks the newest four frames"""
    import torch
    kw = NETS["app3"]
    nEnv, L, dS, dA = 8, 12, kw["dimS"], kw["dimA"]
    H, D = [_pair(hip_api, "app3", oracle=False) for _ in range(2)]
    rng = np.random.default_rng(9)
    rounds = 2
    noise = np.clip(rng.normal(size=(rounds, L, nEnv, dA)), -2, 2)
    dev = "cuda"
    M = torch.from_numpy((rng.normal(size=(dS, dS)) * (1.5 / np.sqrt(dS))).astype(np.float32)).to(dev)
    K = torch.from_numpy((rng.normal(size=(dA, dS)) * 0.3).astype(np.float32)).to(dev)
    s0 = torch.from_numpy(rng.normal(size=(nEnv, dS)).astype(np.float32)).to(dev)
    noise_d = torch.from_numpy(noise).to(dev)
    first = torch.arange(nEnv, dtype=torch.int64, device=dev)      # the episodes start in row 0 of the buffer: first_row = 0 * nEnv + env
    steps = [torch.full((nEnv,), t + 1, dtype=torch.int32, device=dev) for t in range(L)]

    def simulate(s, a):      # the "simulator": a linear map on the device, the same launch for both loops
        nxt = torch.tanh(s @ M + a.float() @ K)
        return nxt, -(nxt.double() ** 2).mean(dim=1)

    def buffers():
        return (torch.zeros((L + 1, nEnv, dS), dtype=torch.float32, device=dev), torch.zeros((L + 1, nEnv, dA), dtype=torch.float64, device=dev),
                torch.zeros((L + 1, nEnv, 2 * dA), dtype=torch.float64, device=dev), torch.zeros((L + 1, nEnv), dtype=torch.float64, device=dev),
                torch.zeros((L + 1, nEnv), dtype=torch.float32, device=dev), torch.zeros((L + 1, nEnv), dtype=torch.float32, device=dev))

    for it in range(rounds):
        # on tensors: the episode's start row and t + 1, no state, action or value leaves the device
        S, A, MU, R, V, ADV = buffers()
        S[0] = s0
        for t in range(L):
            D.select_actions_sequences_dev(S, first, steps[t], nEnv, noise_d[it, t], out=(A[t], MU[t], V[t], ADV[t]))
            S[t + 1], R[t + 1] = simulate(S[t], A[t])
        D.append_episodes_dev([L + 1] * nEnv, [1] * nEnv, [1000 + it * nEnv + e for e in range(nEnv)], list(range(nEnv)), nEnv, S, A, MU, R, V, ADV)
        D.step(1)
        # through the host pointers: hl_forward_sequences on the episode so far, the head on the host, hl_append_episode per episode
        Sh, Ah, MUh, Rh, Vh, ADVh = buffers()
        Sh[0] = s0
        for t in range(L):
            hist = Sh[:t + 1].cpu().numpy()
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
