"""Acting and episode ingestion from device memory (include/smarties_hip_dev.h; smarties_amd/csrc/learner_dev.h, actdev.hip), on the GPU:
hl_forward_dev against hl_forward bit for bit with the rows written on a side stream right before the call; the fp64 head kernel against
the numpy restatement of tests/acting.py; hl_append_episodes_dev against hl_append_episode for a strided rollout buffer --
fields, statistics, training after it, eviction, the episode log --; and a closed loop act -> simulate -> append -> step on tensors against
the same loop through the host-pointer calls."""
import numpy as np
import pytest

from acting import CLIP, DENSE_BASE as BASE, N_AGENTS, _check_heads, _same_replay, _same_training_state, head_np
from oracle_api import fill_synth, synth_cfg
from parity import assert_columns, twin64
from smarties_amd import capi


def _learner(hip_api, kw, n_eps=20, weights=None):
    L = capi.Learner(hip_api, capi.make_config(**kw))
    if weights is None:
        L.init_weights()
    else:
        w = np.random.default_rng(weights[0]).uniform(-weights[1], weights[1], L.nParams).astype(np.float32)
        L.set_params(w, np.zeros_like(w), np.zeros_like(w))
    if n_eps:
        fill_synth(L, synth_cfg(seed=21, dimS=kw["dimS"], dimA=kw["dimA"], lenMin=5, lenMax=30, pTerm=0.5), n_eps)
        L.initialize()
    return L


# ---- 1. forward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_forward_dev_equals_hl_forward_and_leaves_training_untouched(hip_api):
    import torch
    A, B = _learner(hip_api, BASE), _learner(hip_api, BASE)      # B never acts
    A.step(2); B.step(2)
    base = (np.random.default_rng(3).normal(size=(capi.ACT_ROWS_CHUNK + 1, A.dIn)) * 1.5 + 0.2).astype(np.float32)
    side = torch.cuda.Stream()
    for n in (1, 15, 16, 17, capi.ACT_ROWS_CHUNK + 1):      # a partial block of 16 rows, one row past a chunk
        ref = A.forward(base[:n])
        with torch.cuda.stream(side):
            half = torch.from_numpy(base[:n] * np.float32(0.5)).to("cuda", non_blocking=True)
            st = half + half                                  # the rows are written on the side stream right before the call
            out = A.forward_dev(st, stream=side)
            got = out.cpu().numpy()                           # read in that stream's order, no other synchronisation
        assert got.shape == (n, A.nOut)
        assert np.array_equal(got, ref), n
    assert_columns(got, twin64(A).forward(base), 1e-5, "forward_dev, %d rows" % len(base))      # (TOL32 of the acting tests, per output column)
    assert A.forward_dev(torch.empty((0, A.dIn), dtype=torch.float32, device="cuda")).shape == (0, A.nOut)
    A.step(3); B.step(3)
    _same_training_state(A, B)


@pytest.mark.gpu
def test_forward_dev_refusals(hip_api):
    import torch
    rec = _learner(hip_api, dict(BASE, hidden=(16, 16), nn_type=capi.NN_LSTM, nnBPTTseq=4), n_eps=0)
    conv = _learner(hip_api, dict(dimS=576, dimA=2, conv=[(12, 12, 4, 8, 3, 1), (10, 10, 8, 16, 4, 2)], hidden=(32,), nnFunc="Tanh",
                                  batchSize=12, maxTotObsNum=900, randSeed=2), n_eps=0)
    for L in (rec, conv):
        st = torch.zeros((3, L.dIn), dtype=torch.float32, device="cuda")
        with pytest.raises(capi.HlError) as e:
            L.forward_dev(st)
        assert e.value.status == 8                            # HL_ERR_UNSUPPORTED
        with pytest.raises(capi.HlError) as e:
            L.select_actions_dev(st)
        assert e.value.status == 8
    G = _learner(hip_api, BASE)
    st = torch.zeros((3, G.dIn), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        G.forward_dev(st.cpu())                               # not on the GPU
    with pytest.raises(TypeError):
        G.forward_dev(st.double())                            # dtype
    with pytest.raises(ValueError):
        G.forward_dev(torch.zeros((3, 2 * G.dIn), dtype=torch.float32, device="cuda")[:, :G.dIn])      # not contiguous
    G.step_begin()
    with pytest.raises(capi.HlError) as e:
        G.forward_dev(st)
    assert e.value.status == 4                                # HL_ERR_STATE
    G.step_end()
    assert torch.isfinite(G.forward_dev(st)).all()


# ---- 2. the heads -----------------------------------------------------------------------------------------------------------------------
HEADS = {
    "vracer": dict(BASE, dimA=3, bounded=[1, 0, 1]),
    "gaussian": dict(BASE, dimA=2, bounded=[1, 0], adv_kind=capi.ADV_GAUSSIAN),
    "discrete": dict(BASE, dimA=1, bounded=[0], adv_kind=capi.ADV_DISCRETE, n_options=5),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HEADS))
def test_head_kernel_matches_numpy_restatement(hip_api, name):
    import torch
    kw = HEADS[name]
    G = _learner(hip_api, kw, weights=(7, 1.0))              # weights of order one: means, deviations and advantages of order one to ten
    rng = np.random.default_rng(17)
    st = (rng.normal(size=(N_AGENTS, G.dIn)) * 1.5).astype(np.float32)
    O = G.forward(st)                                         # bit-identical to forward_dev's (the forward test)
    dA, nOpt = kw["dimA"], kw.get("n_options", 0)
    if nOpt:
        # u at the midpoint of option (i mod nOpt)'s interval of the CDF, from the numpy probabilities
        noise = np.zeros(N_AGENTS)
        for i in range(N_AGENTS):
            p = head_np(O[i], None, 1, n_options=nOpt)[1]
            c = np.concatenate([[0.0], np.cumsum(p)])
            noise[i] = (c[i % nOpt] + c[i % nOpt + 1]) / 2
    else:
        noise = np.clip(rng.normal(size=(N_AGENTS, dA)), -2, 2)
        nAdv = 1 + 2 * dA if kw.get("adv_kind") == capi.ADV_GAUSSIAN else 0
        # bounded component 0 of agents 0 and 1: the noise that carries mean + stdev * noise to +9 and -9, past the clip
        for i, target in ((0, 9.0), (1, -9.0)):
            mean, pre = O[i, 1 + nAdv], O[i, 1 + nAdv + dA]
            noise[i, 0] = (target - mean) / ((pre + np.sqrt(1 + pre * pre)) / 2)
        assert head_np(O[0], noise[0], dA, kw["bounded"], nAdv > 0)[0][0] == CLIP
        assert head_np(O[1], noise[1], dA, kw["bounded"], nAdv > 0)[0][0] == -CLIP
    dst = torch.from_numpy(st).cuda()
    got = G.select_actions_dev(dst, torch.from_numpy(noise).cuda())
    _check_heads(kw, O, noise, got)
    if nOpt:
        assert set(np.round(got[0].cpu().numpy()[:, 0] - 0.1).astype(int)) == set(range(nOpt))      # every option was drawn
    else:
        assert got[0][0, 0].item() == CLIP and got[0][1, 0].item() == -CLIP
    got = G.select_actions_dev(dst, None)                     # the evaluation action
    _check_heads(kw, O, None, got)


# ---- 3. ingestion -----------------------------------------------------------------------------------------------------------------------
LENGTHS = [2, 3, 17, 60, 33, 5, 41]
T_ROLL, N_ENV = 60, 7


def _rollout(rng, dS, dA, pD):
    """a [T][nEnv] rollout buffer full of numbers; episode e lives in column e from row t0[e] on"""
    buf = dict(states=rng.normal(size=(T_ROLL, N_ENV, dS)).astype(np.float32), actions=rng.normal(size=(T_ROLL, N_ENV, dA)),
               mu=np.abs(rng.normal(size=(T_ROLL, N_ENV, pD))) + 0.1, rewards=rng.normal(size=(T_ROLL, N_ENV)),
               values=rng.normal(size=(T_ROLL, N_ENV)).astype(np.float32), advantages=rng.normal(size=(T_ROLL, N_ENV)).astype(np.float32))
    t0 = [(T_ROLL - n) // 2 for n in LENGTHS]
    return buf, t0


def _append_both(H, D, rng, tag0, with_adv, no_adv_episode=None):
    """the seven episodes into H through hl_append_episode, into D through ONE hl_append_episodes_dev call on the strided buffer"""
    import torch
    buf, t0 = _rollout(rng, H.dS, H.dA, H.polDim)
    if no_adv_episode is not None:      # this episode comes without advantages on the host route: zeros in the device buffer
        e = no_adv_episode
        buf["advantages"][t0[e]:t0[e] + LENGTHS[e], e] = 0
    term = [e % 2 for e in range(N_ENV)]
    for e, n in enumerate(LENGTHS):
        sl = slice(t0[e], t0[e] + n)
        adv = buf["advantages"][sl, e] if with_adv and e != no_adv_episode else None
        H.append_episode(buf["states"][sl, e], buf["actions"][sl, e], buf["mu"][sl, e], buf["rewards"][sl, e], buf["values"][sl, e],
                         term[e], tag0 + e, advantages=adv)
    dev = {k: torch.from_numpy(v).cuda() for k, v in buf.items()}
    D.append_episodes_dev(LENGTHS, term, [tag0 + e for e in range(N_ENV)], [t0[e] * N_ENV + e for e in range(N_ENV)], N_ENV,
                          dev["states"], dev["actions"], dev["mu"], dev["rewards"], dev["values"], dev["advantages"] if with_adv else None)


@pytest.mark.gpu
def test_append_episodes_dev_equals_hl_append_episode(hip_api, tmp_path):
    H, D = _learner(hip_api, BASE, n_eps=0), _learner(hip_api, BASE, n_eps=0)
    H.set_episode_log(tmp_path / "host.dat"); D.set_episode_log(tmp_path / "dev.dat")
    _append_both(H, D, np.random.default_rng(1), 100, True, no_adv_episode=2)
    _same_replay(H, D)
    H.initialize(); D.initialize()
    H.step(3); D.step(3)
    _same_training_state(H, D)
    _append_both(H, D, np.random.default_rng(2), 200, True)      # behind gradient steps: the placeholder error comes from the statistics pass
    _same_replay(H, D)
    H.step(3); D.step(3)
    _same_training_state(H, D)
    _same_replay(H, D)
    log_h, log_d = (tmp_path / "host.dat").read_bytes(), (tmp_path / "dev.dat").read_bytes()
    assert log_h == log_d and log_h.count(b"\n") == 2 * N_ENV


@pytest.mark.gpu
def test_append_episodes_dev_with_eviction_and_without_advantages(hip_api):
    kw = dict(BASE, maxTotObsNum=200)                         # one batch holds 161 steps: the second forces episodes out
    H, D = _learner(hip_api, kw, n_eps=0), _learner(hip_api, kw, n_eps=0)
    _append_both(H, D, np.random.default_rng(3), 0, False)
    H.initialize(); D.initialize()
    H.step(3); D.step(3)
    _same_training_state(H, D)
    for r in range(2):
        _append_both(H, D, np.random.default_rng(4 + r), 100 * (r + 1), False)
        H.step(3); D.step(3)
        _same_training_state(H, D)
        _same_replay(H, D)
    assert D.counts()[1] < 3 * N_ENV                          # episodes were evicted
    with pytest.raises(capi.HlError) as e:
        D.append_episodes_dev([1], [0], [0], [0], 1, 1, 1, 1, 1, 1)      # an episode of one step: refused before anything is stored
    assert e.value.status == 1


# ---- 4. the loop ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_loop_on_tensors_equals_loop_through_host_pointers(hip_api):
    import torch
    kw = dict(BASE, dimA=2, bounded=[1, 0])
    H, D = _learner(hip_api, kw, n_eps=10), _learner(hip_api, kw, n_eps=10)
    nEnv, L, dS, dA = 4, 4, kw["dimS"], kw["dimA"]
    rng = np.random.default_rng(9)
    noise = np.clip(rng.normal(size=(20, L, nEnv, dA)), -2, 2)
    dev = "cuda"
    M = torch.from_numpy((rng.normal(size=(dS, dS)) * 0.4).astype(np.float32)).to(dev)
    K = torch.from_numpy((rng.normal(size=(dA, dS)) * 0.3).astype(np.float32)).to(dev)
    s0 = torch.from_numpy(rng.normal(size=(nEnv, dS)).astype(np.float32)).to(dev)
    noise_d = torch.from_numpy(noise).to(dev)

    def simulate(s, a):      # the "simulator": a linear map on the device, the same launch for both loops
        nxt = torch.tanh(s @ M + a.float() @ K)
        return nxt, -(nxt.double() ** 2).sum(dim=1)

    def buffers():
        return (torch.zeros((L + 1, nEnv, dS), dtype=torch.float32, device=dev), torch.zeros((L + 1, nEnv, dA), dtype=torch.float64, device=dev),
                torch.zeros((L + 1, nEnv, 2 * dA), dtype=torch.float64, device=dev), torch.zeros((L + 1, nEnv), dtype=torch.float64, device=dev),
                torch.zeros((L + 1, nEnv), dtype=torch.float32, device=dev), torch.zeros((L + 1, nEnv), dtype=torch.float32, device=dev))

    for it in range(20):
        # on tensors: no state, action or value leaves the device
        S, A, MU, R, V, ADV = buffers()
        S[0] = s0
        for t in range(L):
            D.select_actions_dev(S[t], noise_d[it, t], out=(A[t], MU[t], V[t], ADV[t]))
            S[t + 1], R[t + 1] = simulate(S[t], A[t])
        D.append_episodes_dev([L + 1] * nEnv, [1] * nEnv, [1000 + it * nEnv + e for e in range(nEnv)], list(range(nEnv)), nEnv, S, A, MU, R, V, ADV)
        D.step(1)
        # through the host pointers: hl_forward, the head on the host, hl_append_episode per episode
        Sh, Ah, MUh, Rh, Vh, ADVh = buffers()
        Sh[0] = s0
        for t in range(L):
            O = H.forward(Sh[t].cpu().numpy())
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
