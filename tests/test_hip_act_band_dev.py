"""Acting from device memory beyond the resident plans (smarties_amd/csrc/actband.hip: act_conv_band_dev_kernel, the first conv layer's
image in bands of output rows; act_rows_panel_kernel, the first dense layer's input row in panels; learner_dev.h routes the device calls
of include/smarties_hip_dev.h), on the GPU: the nets the device calls refused before -- the Nature-DQN stack, an image of 176 KB, feature
and input rows between 2049 and 8192 -- against the CPU oracle row by row and column by column, packed and as columns of a [T][nEnv]
buffer, permuted, against the host calls; the new kernels against the resident ones bit for bit on the nets both run
(SMARTIES_HIP_GENERIC=8192: three bands, panels of 64 columns); a states array at no 16-byte boundary; training left untouched; the
refusals that remain; a closed loop act -> simulate -> append -> step on tensors."""
import numpy as np
import pytest

from acting import (BAND_NETS as NEW, FALLBACK, LDS_NETS, N_EPS, NETS, PARITY, TOL32, _BASE, _bare, _call_dev, _columns, _conv_pair as _pair, _count,
                    _packed, _rows, _same_replay, _same_training_state, _side_stream, _stacked, _synth_learner as _learner, _window_args, head_np)
from parity import COL_ROWS, assert_columns, relinf, twin64
from smarties_amd import capi


def _new_pair(hip_api, name, monkeypatch, oracle=True):
    kw = NEW[name][0]
    monkeypatch.setitem(NETS, name, kw)
    if name == "nature":
        monkeypatch.setitem(N_EPS, name, 14)
    return _pair(hip_api, name, oracle=oracle)


def _wins(rng, n, kw, lengths):
    return [_rows(rng, lengths[i % len(lengths)], kw["dimS"]) for i in range(n)]


def _check(name, what, got, ref):
    err = [relinf(got[i], ref[i]) for i in range(len(got))]
    worst = int(np.argmax(err))
    print("%s %s: worst row %d relinf %.3g" % (name, what, worst, err[worst]))
    assert err[worst] < TOL32, (name, what, worst, got[worst], ref[worst])


# ---- 1. the nets served from now on, against the oracle ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NEW))
def test_newly_served_nets_match_the_oracle(hip_api, name, monkeypatch):
    """The fp32 restatement against its fp64 build on these rows after three steps (CPU): worst row / worst column 1.4e-6 / 5.5e-5
    (column 12; 7.8e-6 in column 2) for nature, 9.8e-7 / 3.9e-6 (column 0) for dense-1030x3, 2.8e-7 / 1.3e-6 image-176K, 4.8e-7 / 1.6e-6
    feat-2357, 6.4e-7 / 2.8e-6 dense-2500: the two nets with columns beyond TOL32 / 3 take assert_columns' cpu_bar."""
    import torch
    kw, ns, lengths, bands, panelled, cpu_bar = NEW[name]
    nApp = kw.get("nAppendedObs", 0)
    monkeypatch.delenv("SMARTIES_HIP_GENERIC", raising=False)
    G, O = _new_pair(hip_api, name, monkeypatch)
    G.step(3); O.step(3)
    rng = np.random.default_rng(11)
    G.timing_enable(True)
    names = ("act_conv_band_dev", "act_rows_panel_dev", "act_conv_dev", "act_rows_dev", "act_conv")

    def counted(call, n):
        c0 = [_count(G, k) for k in names]
        got = call()
        torch.cuda.synchronize()
        d = dict(zip(names, [_count(G, k) - c for k, c in zip(names, c0)]))
        chunks = -(-n // capi.ACT_ROWS_CHUNK)
        assert d["act_conv_band_dev"] == bands and d["act_conv_dev"] == (1 - bands if "conv" in kw else 0), (name, n, d)
        assert d["act_rows_panel_dev"] == (chunks if panelled else 0) and d["act_rows_dev"] == (0 if panelled else chunks), (name, n, d)
        assert d["act_conv"] == 0, (name, n, d)
        return got

    if lengths is None:      # rows through hl_forward_dev
        st = _rows(rng, max(ns), G.dIn)
        ref, ref64, host = O.forward(st), twin64(O).forward(st), G.forward(st)
        perm = rng.permutation(max(ns))
        for n in ns:
            got = counted(lambda: G.forward_dev(torch.from_numpy(st[:n]).cuda()).cpu().numpy(), n)
            assert got.shape == (n, G.nOut)
            _check(name, "n=%d" % n, got, ref)
            for i in range(n):
                assert relinf(got[i], host[i]) < 2 * TOL32, (name, n, i)      # (hl_forward runs this net over the training buffers)
            if n >= COL_ROWS:
                assert_columns(got, ref64[:n], TOL32, (name, n), ref[:n], cpu_bar=cpu_bar)
        assert np.array_equal(G.forward_dev(torch.from_numpy(st[perm]).cuda()).cpu().numpy(), got[perm])
        G.timing_enable(False)
        return
    wins = _wins(rng, max(ns), kw, lengths)
    rows = _stacked(wins, nApp)
    ref, ref64, host = O.forward(rows), twin64(O).forward(rows), G.forward_sequences(wins)
    side = _side_stream()
    for n in ns:
        both = []
        for layout in (_packed(wins[:n]), _columns(wins[:n])):
            got = counted(lambda: _call_dev(G, side, layout, np.arange(n)), n)
            assert got.shape == (n, G.nOut)
            _check(name, "n=%d stride %d" % (n, layout[3]), got, ref)
            for i in range(n):
                assert relinf(got[i], host[i]) < 2 * TOL32, (name, n, i)      # (the host call runs other kernels: the bar between routes)
            if n >= COL_ROWS:
                assert_columns(got, ref64[:n], TOL32, (name, layout[3], n), ref[:n], cpu_bar=cpu_bar)
            both.append(got)
        assert np.array_equal(both[0], both[1]), (name, n)
    n = ns[1]
    perm = rng.permutation(n)
    full = _call_dev(G, side, _columns(wins[:n]), np.arange(n))
    assert np.array_equal(_call_dev(G, side, _columns(wins[:n]), perm), full[perm]), name
    G.timing_enable(False)


# ---- 2. the resident kernels and the new ones, bit for bit ---------------------------------------------------------------------------------
def _twins(hip_api, make, monkeypatch):
    """(the learner as shipped, its twin created with bit 8192): the same weights after the same three steps"""
    monkeypatch.delenv("SMARTIES_HIP_GENERIC", raising=False)
    G = make()
    monkeypatch.setenv("SMARTIES_HIP_GENERIC", "8192")
    T = make()
    monkeypatch.delenv("SMARTIES_HIP_GENERIC")
    G.step(3); T.step(3)
    assert np.array_equal(G.get_params()[0], T.get_params()[0])
    return G, T


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY + ["dense-app3"])
def test_banded_and_panelled_kernels_equal_the_resident_ones_bit_for_bit(hip_api, name, monkeypatch):
    """bands of uneven row counts and overlapping input rows (20 -> 7, 7, 6; 10 -> 4, 4, 2; 5 -> 2, 2, 1; 3 -> 1, 1, 1 with stride 2 under a
    filter of 6), panels of 64 columns with a tail, the residual read from device memory: the sums of the resident kernels"""
    import torch
    if name == "dense-app3":
        kw, sc_kw = FALLBACK[name]
        G, T = _twins(hip_api, lambda: _learner(hip_api, kw, sc_kw), monkeypatch)
        lengths = [1, 2, 5, 9, 3]
    else:
        kw = NETS[name]
        G, T = _twins(hip_api, lambda: _pair(hip_api, name, oracle=False), monkeypatch)
        lengths = [k for k in (1, 2, kw.get("nAppendedObs", 0), kw.get("nAppendedObs", 0) + 1, 9) if k >= 1]
    rng = np.random.default_rng(11)
    ns = (1, 17) if name == "atari" else (1, 17, 300)
    wins = _wins(rng, max(ns), kw, lengths)
    side = _side_stream()
    T.timing_enable(True)
    for n in ns:
        for layout in (_packed(wins[:n]), _columns(wins[:n])):
            b0, p0 = _count(T, "act_conv_band_dev"), _count(T, "act_rows_panel_dev")
            got = _call_dev(T, side, layout, np.arange(n))
            torch.cuda.synchronize()
            if "conv" in kw:
                assert _count(T, "act_conv_band_dev") - b0 == 1, (name, n)
            if "conv" in kw or n > 64:      # (up to 64 rows of a small dense net: the one-kernel route, which the switch leaves alone)
                assert _count(T, "act_rows_panel_dev") - p0 == 1, (name, n)
            assert np.array_equal(got, _call_dev(G, side, layout, np.arange(n))), (name, layout[3], n)
    T.timing_enable(False)
    n = ns[-1]
    nOpt = kw.get("n_options", 0)
    noise = torch.from_numpy(rng.uniform(0, 1, n) if nOpt else np.clip(rng.normal(size=(n, kw["dimA"])), -2, 2)).cuda()
    layout = _columns(wins[:n])
    for g, t in zip(_call_dev(G, side, layout, np.arange(n), select=noise), _call_dev(T, side, layout, np.arange(n), select=noise)):
        assert np.array_equal(g, t), name


# ---- 3. alignment --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["image-176K", "nature"])
def test_band_loads_from_states_one_float_into_a_buffer_give_the_same_bits(hip_api, name, monkeypatch):
    import torch
    kw = NEW[name][0]
    monkeypatch.delenv("SMARTIES_HIP_GENERIC", raising=False)
    G = _new_pair(hip_api, name, monkeypatch, oracle=False)
    G.step(2)
    wins = _wins(np.random.default_rng(4), 9, kw, NEW[name][2])
    states, first, n_steps, stride = _columns(wins)
    first_d, steps_d = torch.from_numpy(first).cuda(), torch.from_numpy(n_steps).cuda()
    states = np.nan_to_num(states, nan=7.0)
    aligned = torch.from_numpy(states).cuda()
    big = torch.zeros(states.size + 5, dtype=torch.float32, device="cuda")
    shifted = big[1:1 + states.size].view(states.shape)
    shifted.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    a = G.forward_sequences_dev(aligned, first_d, steps_d, stride).cpu().numpy()
    b = G.forward_sequences_dev(shifted, first_d, steps_d, stride).cpu().numpy()
    assert np.isfinite(a).all() and np.array_equal(a, b)


# ---- 4. training is untouched --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_acting_through_the_panelled_kernel_leaves_training_untouched(hip_api, monkeypatch):
    import torch
    kw = NEW["feat-2357"][0]
    monkeypatch.delenv("SMARTIES_HIP_GENERIC", raising=False)
    A, B = [_new_pair(hip_api, "feat-2357", monkeypatch, oracle=False) for _ in range(2)]
    rng = np.random.default_rng(2)
    wins = _wins(rng, 70, kw, (1, 2, 9))
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


# ---- 5. the refusals that remain -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_nets_beyond_the_banded_and_panelled_plans_are_refused(hip_api, monkeypatch):
    import torch
    monkeypatch.delenv("SMARTIES_HIP_GENERIC", raising=False)
    wide = dict(_BASE, dimS=188, conv=[(18, 10, 1, 64, 3, 1)], hidden=(32,))      # 8 extras + 64 x 8 x 16: a feature row of 8200
    for kw, word in ((LDS_NETS["map-162K"], "any band count"), (wide, "8192")):
        L = _bare(hip_api, kw)
        for call in (L.forward_sequences_dev, L.select_actions_sequences_dev):
            with pytest.raises(capi.HlError) as e:
                call(*_window_args(L), 1)
            assert e.value.status == 8 and word in str(e.value), str(e.value)
    L = _bare(hip_api, dict(_BASE, dimS=8193, hidden=(32,)))
    with pytest.raises(capi.HlError) as e:
        L.forward_dev(torch.zeros((3, L.dIn), dtype=torch.float32, device="cuda"))
    assert e.value.status == 8 and "8192" in str(e.value), str(e.value)
    monkeypatch.setenv("SMARTIES_HIP_GENERIC", "2")
    conv, dense = _bare(hip_api, NEW["feat-2357"][0]), _bare(hip_api, NEW["dense-2500"][0])
    monkeypatch.delenv("SMARTIES_HIP_GENERIC")
    with pytest.raises(capi.HlError) as e:
        conv.forward_sequences_dev(*_window_args(conv), 1)
    assert e.value.status == 8 and "bit 2" in str(e.value), str(e.value)
    with pytest.raises(capi.HlError) as e:
        dense.forward_dev(torch.zeros((3, dense.dIn), dtype=torch.float32, device="cuda"))
    assert e.value.status == 8 and "bit 2" in str(e.value), str(e.value)


# ---- 6. the loop ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_loop_on_tensors_through_the_panelled_kernel(hip_api, monkeypatch):
    """act -> simulate -> append -> step on tensors against the same loop through the host-pointer calls.  The host call runs this net over
    the training buffers, so the two loops agree to rounding only: the first iteration is compared, both must stay finite, and the device
    loop's replay must equal one ingested from its own tensors through hl_append_episode."""
    import torch
    kw = NEW["feat-2357"][0]
    nEnv, L, dS, dA = 4, 6, kw["dimS"], kw["dimA"]
    monkeypatch.delenv("SMARTIES_HIP_GENERIC", raising=False)
    H, D, R = [_new_pair(hip_api, "feat-2357", monkeypatch, oracle=False) for _ in range(3)]
    rng = np.random.default_rng(9)
    rounds = 10
    noise = np.clip(rng.normal(size=(rounds, L, nEnv, dA)), -2, 2)
    dev = "cuda"
    M = torch.from_numpy((rng.normal(size=(dS, dS)) * (1.5 / np.sqrt(dS))).astype(np.float32)).to(dev)
    K = torch.from_numpy((rng.normal(size=(dA, dS)) * 0.3).astype(np.float32)).to(dev)
    s0 = torch.from_numpy(rng.normal(size=(nEnv, dS)).astype(np.float32)).to(dev)
    noise_d = torch.from_numpy(noise).to(dev)
    first = torch.arange(nEnv, dtype=torch.int64, device=dev)
    steps = [torch.full((nEnv,), t + 1, dtype=torch.int32, device=dev) for t in range(L)]

    def simulate(s, a):
        nxt = torch.tanh(s @ M + a.float() @ K)
        return nxt, -(nxt.double() ** 2).mean(dim=1)

    def buffers():
        return (torch.zeros((L + 1, nEnv, dS), dtype=torch.float32, device=dev), torch.zeros((L + 1, nEnv, dA), dtype=torch.float64, device=dev),
                torch.zeros((L + 1, nEnv, 2 * dA), dtype=torch.float64, device=dev), torch.zeros((L + 1, nEnv), dtype=torch.float64, device=dev),
                torch.zeros((L + 1, nEnv), dtype=torch.float32, device=dev), torch.zeros((L + 1, nEnv), dtype=torch.float32, device=dev))

    s0h = s0.clone()
    for it in range(rounds):
        tags = [1000 + it * nEnv + e for e in range(nEnv)]
        S, A, MU, R_, V, ADV = buffers()
        S[0] = s0
        for t in range(L):
            D.select_actions_sequences_dev(S, first, steps[t], nEnv, noise_d[it, t], out=(A[t], MU[t], V[t], ADV[t]))
            S[t + 1], R_[t + 1] = simulate(S[t], A[t])
        D.append_episodes_dev([L + 1] * nEnv, [1] * nEnv, tags, list(range(nEnv)), nEnv, S, A, MU, R_, V, ADV)
        D.step(1)
        own = [x.cpu().numpy() for x in (S, A, MU, R_, V, ADV)]      # the device loop's tensors through the host call
        for e in range(nEnv):
            R.append_episode(own[0][:, e], own[1][:, e], own[2][:, e], own[3][:, e], own[4][:, e], 1, tags[e], advantages=own[5][:, e])
        R.step(1)
        Sh, Ah, MUh, Rh, Vh, ADVh = buffers()
        Sh[0] = s0h
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
            H.append_episode(host[0][:, e], host[1][:, e], host[2][:, e], host[3][:, e], host[4][:, e], 1, tags[e], advantages=host[5][:, e])
        H.step(1)
        if it == 0:
            for got, want in ((own[0], host[0]), (own[1], host[1]), (own[4], host[4])):
                assert relinf(got, want) < 2 * TOL32
        s0, s0h = S[L].clone(), Sh[L].clone()
    for X in (H, D):
        assert np.isfinite(X.get_params()[0]).all()
    _same_training_state(R, D)
    _same_replay(R, D)
