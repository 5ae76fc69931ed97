"""DPG learners (hl_create_dpg) against a plain numpy fp64 restatement of one DPG step (DPG::Train), at the bound of the NAF and DQN
tests: 1e-5 relative, each column / block on its own scale.  tests/test_dpg_cpu.py holds the same restatement in fp32 to a third of it."""
import ctypes as C

import numpy as np
import pytest

from smarties_amd import capi
from blocks import TOL32
from parity import relinf

GAMMA, CLIP, NOISE, N = 0.9, 4.0, 0.4472135955, 6
# name -> dimS, dimA, hidden, batch, bounded
# (D: 272 units are a wavefront's second group of column tiles in the target launch's forward, 272 inputs its second 64-row trip backward)
SHAPES = {"A": (5, 2, (32, 32), 20, (0, 0)), "B": (17, 6, (48,), 16, (0,) * 6), "C": (9, 3, (64, 16, 80), 33, (1, 0, 1)),
          "D": (5, 2, (272, 48), 16, (0, 0))}
STEPS = (0, 1, 3, 4)      # sampled steps of an episode of N states: a pair t, t + 1; t = 4 is followed by the last state


def episodes(dS, dA, B, seed=3):
    """enough episodes of N states for B samples; every second one terminated; step 3 of the even ones far from the policy"""
    rng = np.random.RandomState(seed); eps = []
    for tag in range(-(-B // len(STEPS))):
        mu = np.concatenate([0.1 * rng.randn(N, dA), np.full((N, dA), NOISE)], 1)
        act = mu[:, :dA] + 0.3 * rng.randn(N, dA)
        if tag % 2 == 0:
            act[3] = 2.0; mu[3, :dA] = 2.0
        eps.append(dict(S=rng.randn(N, dS).astype(np.float32), A=act, MU=mu, R=1 + rng.rand(N), V=rng.randn(N).astype(np.float32), term=tag % 2, tag=tag))
    samples = [(k, t) for k in range(len(eps)) for t in STEPS][:B]
    return eps, samples


def layout(dIn, hidden, nDense, nSig):
    """offsets of the padded blob: dense 1, (dense, residual) ..., output, sigma; every block on a multiple of 8 floats"""
    up = lambda n: -(-n // 8) * 8; tot = 0; lay = []; prev = dIn
    def block(n):
        nonlocal tot
        at = tot; tot += up(n); return at
    for j, size in enumerate(hidden):
        rec = dict(nIn=prev, size=size, ld=up(size), iW=block(up(size) * prev), iB=block(size), r=0)
        if j > 0:
            rec.update(r=min(prev, size), iWr=block(size), iBr=block(size))
        lay.append(rec); prev = size
    out = dict(nIn=prev, size=nDense, ld=up(nDense), iW=block(up(nDense) * prev), iB=block(nDense))
    return dict(hid=lay, out=out, iSig=block(nSig) if nSig else None, n=tot)


def forward(W, lay, X, dt):
    """SoftSign layers with the parametric residual, Linear output -> outputs, what the backward pass needs"""
    W = W.astype(dt); inp = X.astype(dt); keep = []
    for k in lay["hid"]:
        Wj = W[k["iW"]:k["iW"] + k["nIn"] * k["ld"]].reshape(k["nIn"], k["ld"])[:, :k["size"]]
        x = inp @ Wj + W[k["iB"]:k["iB"] + k["size"]]; y = x / (1 + np.abs(x)); wr = None
        if k["r"]:
            r = k["r"]; wr = W[k["iWr"]:k["iWr"] + r]; y = y.copy(); y[:, :r] += inp[:, :r] * wr + W[k["iBr"]:k["iBr"] + r]
        keep.append(dict(inp=inp, x=x, W=Wj, wr=wr)); inp = y
    o = lay["out"]; Wo = W[o["iW"]:o["iW"] + o["nIn"] * o["ld"]].reshape(o["nIn"], o["ld"])[:, :o["size"]]
    return inp @ Wo + W[o["iB"]:o["iB"] + o["size"]], dict(y=inp, keep=keep, Wo=Wo)


def backward(lay, fw, D):
    """output deltas D -> the summed weight gradient in the blob's layout, the gradient with respect to the input rows"""
    g = np.zeros(lay["n"]); o = lay["out"]
    blk = np.zeros((o["nIn"], o["ld"])); blk[:, :o["size"]] = fw["y"].T @ D; g[o["iW"]:o["iW"] + blk.size] = blk.ravel()
    g[o["iB"]:o["iB"] + o["size"]] = D.sum(0); dres = D @ fw["Wo"].T
    for k, f in zip(lay["hid"][::-1], fw["keep"][::-1]):
        r = k["r"]
        if r:
            g[k["iWr"]:k["iWr"] + r] = (dres[:, :r] * f["inp"][:, :r]).sum(0); g[k["iBr"]:k["iBr"] + r] = dres[:, :r].sum(0)
        dl = dres / (1 + np.abs(f["x"])) ** 2
        blk = np.zeros((k["nIn"], k["ld"])); blk[:, :k["size"]] = f["inp"].T @ dl; g[k["iW"]:k["iW"] + blk.size] = blk.ravel()
        g[k["iB"]:k["iB"] + k["size"]] = dl.sum(0)
        prev = dl @ f["W"].T
        if r:
            prev[:, :r] += dres[:, :r] * f["wr"]
        dres = prev
    return g, dres


sp, spd = (lambda x: (x + np.sqrt(1 + x * x)) / 2), (lambda x: (1 + x / np.sqrt(1 + x * x)) / 2)      # SoftPlus and its derivative


def dpg_step(nets, shape, rows, beta, Cmax, Cinv, dt=np.float64):
    """one DPG step on `rows` (dicts s, s1, a, mu, r, lastTerm, nextSampled): the networks in `dt`, the head in fp64"""
    dS, dA, hidden, _, bounded = shape; Wa, Wc, Ta, Tc = nets
    la, lc = layout(dS, hidden, dA, dA), layout(dS + dA, hidden, 1, 0)
    S, S1 = np.stack([r["s"] for r in rows]), np.stack([r["s1"] for r in rows]); A = np.stack([r["a"] for r in rows])
    mean, fa = forward(Wa, la, S, dt); sig = Wa[la["iSig"]:la["iSig"] + dA].astype(np.float64)
    q, fc = forward(Wc, lc, np.concatenate([S, A], 1), dt)
    tgt = lambda X: forward(Tc, lc, np.concatenate([X, forward(Ta, la, X, dt)[0]], 1), dt)      # Q~(s, mu~(s)) through both target nets
    qT, ft = tgt(S); qN = tgt(S1)[0]
    dQda = backward(lc, ft, np.ones_like(qT))[1][:, dS:]
    out = dict(qT=qT[:, 0], qN=qN[:, 0], dQda=dQda, pvec=np.concatenate([mean.astype(np.float64), np.tile(sig, (len(rows), 1))], 1), q=q[:, 0], wb=[], nxt=[], far=[])
    Ga, Gc = np.zeros((len(rows), 2 * dA)), np.zeros((len(rows), 1)); std = sp(sig); bnd = np.asarray(bounded, bool)
    for b, r in enumerate(rows):
        m = mean[b].astype(np.float64); bm, bs = r["mu"][:dA], r["mu"][dA:]; a = r["a"]
        mc = np.where(bnd, np.clip(m, -8.31776613503286, 8.31776613503286), m)
        logw = np.sum(((a - bm) / bs) ** 2 - ((a - mc) / std) ** 2) / 2 - np.sum(np.log(std / bs))
        rho = np.exp(np.clip(logw, -7, 7)); far = bool(np.float32(rho) > np.float32(Cmax) or np.float32(rho) < np.float32(Cinv))
        dkl = np.sum((std / bs) ** 2 - 1 + ((m - bm) / bs) ** 2 - 2 * np.log(std / bs)) / 2
        target = r["r"]; useNext = not r["lastTerm"] and not far
        if useNext:
            target = target + GAMMA * float(qN[b, 0])
        pol = np.zeros(dA) if far else dQda[b].astype(np.float64)
        penM, penS = -(m - bm) / bs ** 2, -spd(sig) * (1 / bs ** 2 - 1 / std ** 2) * std
        Ga[b, :dA] = beta * pol + (1 - beta) * penM; Ga[b, dA:] = beta * spd(sig) * (NOISE - std) / 2 + (1 - beta) * penS
        e = target - float(q[b, 0]); Gc[b, 0] = 0.0 if far else e
        out["wb"].append((e, dkl, rho, float(qT[b, 0]), float(q[b, 0]) - float(qT[b, 0]))); out["far"].append(far)
        out["nxt"].append(float(qN[b, 0]) if useNext and not r["nextSampled"] else None)
    ga = backward(la, fa, Ga[:, :dA])[0]; ga[la["iSig"]:la["iSig"] + dA] = Ga[:, dA:].sum(0)
    out.update(Ga=Ga, Gc=Gc[:, 0], ga=ga, gc=backward(lc, fc, Gc)[0], la=la, lc=lc)
    return out


def blocks_of(lay):
    """(offset, length) of the output layer's and of the first layer's weights and biases"""
    o, f = lay["out"], lay["hid"][0]
    return [(o["iW"], o["nIn"] * o["ld"]), (o["iB"], o["size"]), (f["iW"], f["nIn"] * f["ld"]), (f["iB"], f["size"])]


def dev(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return 0.0 if not np.any(ref) and not np.any(a) else relinf(a, ref)


def random_nets(shape, seed=11):
    """weights of order 1 / sqrt(fan-in) for both nets and their targets (the targets differ from the live weights)"""
    dS, dA, hidden, _, _ = shape; rng = np.random.RandomState(seed); nets = []
    for lay, dIn in ((layout(dS, hidden, dA, dA), dS), (layout(dS + dA, hidden, 1, 0), dS + dA)):
        for _ in range(2):
            W = np.zeros(lay["n"], np.float32)
            for k in lay["hid"] + [lay["out"]]:
                small = 0.1 if (k is lay["out"] and lay["iSig"] is not None) else 1.0      # (means near the stored ones: most samples near-policy)
                W[k["iW"]:k["iW"] + k["nIn"] * k["ld"]] = small * rng.uniform(-1, 1, k["nIn"] * k["ld"]) * np.sqrt(3.0 / k["nIn"])
                W[k["iB"]:k["iB"] + k["size"]] = 0.1 * rng.randn(k["size"])
                if k.get("r"):
                    W[k["iWr"]:k["iWr"] + k["r"]] = 1 + 0.1 * rng.randn(k["r"]); W[k["iBr"]:k["iBr"] + k["r"]] = 0.1 * rng.randn(k["r"])
            if lay["iSig"] is not None:
                W[lay["iSig"]:lay["iSig"] + dA] = (NOISE ** 2 - 0.25) / NOISE + 0.05 * rng.randn(dA)
            nets.append(W)
    return nets[0], nets[2], nets[1], nets[3]      # Wa, Wc, Ta, Tc


def rows_of(eps, samples, mean, scale, r3):
    st = lambda e, t: (e["S"][t] - mean) * scale
    return [dict(s=st(eps[k], t), s1=st(eps[k], t + 1), a=eps[k]["A"][t], mu=eps[k]["MU"][t], lastTerm=bool(t + 2 == N and eps[k]["term"]),
                 r=float(np.float32((eps[k]["R"][t] - np.float64(r3[0])) * np.float64(r3[1]))), nextSampled=(k, t + 1) in samples) for k, t in samples]


def learner(hip_api, shape, delay=0.01, **kw):
    dS, dA, hidden, B, bounded = shape
    L = capi.create_dpg(hip_api, delay, dimS=dS, dimA=dA, bounded=bounded, hidden=hidden, batchSize=B, maxTotObsNum=4096, gamma=GAMMA,
                        clipImpWeight=CLIP, returnsEstimator="none", explNoise=NOISE, randSeed=7, **kw)
    L.init_weights(); eps, samples = episodes(dS, dA, B)
    for e in eps:
        L.append_episode(e["S"], e["A"], e["MU"], e["R"], e["V"], e["term"], e["tag"])
    L.initialize()
    order = eps[::-1]      # position 0 = newest; a flat index = transitions of the episodes in front + t
    prefix = np.concatenate([[0], np.cumsum([N - 1 for _ in order])])
    flat = np.asarray(sorted(prefix[len(eps) - 1 - k] + t for k, t in samples), np.int64)
    return L, eps, order, flat


FIELDS = dict(deltaQ=capi.EP_DELTAQ, dKL=capi.EP_DKL, impW=capi.EP_IMPW, V=capi.EP_VALUE, ADV=capi.EP_ADVANTAGE)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_step_against_the_restatement(hip_api, name):
    shape = SHAPES[name]; dS, dA, hidden, B, bounded = shape
    L, eps, order, flat = learner(hip_api, shape)
    nets = random_nets(shape); Wa, Wc, Ta, Tc = nets
    assert L.nParams == Wa.size and L.nCritic == Wc.size and L.nOut == 2 * dA
    L.set_params(Wa); L.dpg_set_critic(Wc); L.dpg_set_target(0, Ta); L.dpg_set_target(1, Tc)
    sc = L.scalars()
    want = {e["tag"]: {k: L.episode_field(p, f).astype(np.float64) for k, f in FIELDS.items()} for p, e in enumerate(order)}
    Sx = np.random.RandomState(1).randn(4, dS).astype(np.float32); mean, scale, r3 = L.get_scaling()
    O = L.forward(Sx)      # hl_forward: the actor's policy vector
    L.step(1, flat)
    samples = list(zip(L.readback(capi.TAP_TAG), L.readback(capi.TAP_TSTEP)))
    assert sorted(samples) == sorted(episodes(dS, dA, B)[1])
    ref = dpg_step(nets, shape, rows_of(eps, samples, mean, scale, r3), sc.beta, sc.CmaxRet, sc.CinvRet)
    assert any(ref["far"]) and not all(ref["far"]) and list(L.readback(capi.TAP_FAR).astype(bool)) == ref["far"]
    cols = lambda a, r: max(dev(a[:, c], r[:, c]) for c in range(r.shape[1]))
    blk = lambda a, r, lay: max(dev(a[i:i + n], r[i:i + n]) for i, n in blocks_of(lay))
    pv = forward(Wa, ref["la"], (Sx - mean) * scale, np.float64)[0]
    worst = {"forward": cols(O[:, :dA], pv), "sigma": dev(O[:, dA:], np.tile(Wa[ref["la"]["iSig"]:][:dA], (4, 1))),
             "qT": dev(L.dpg_readback(0), ref["qT"]), "qN": dev(L.dpg_readback(1), ref["qN"]), "dQda": cols(L.dpg_readback(2), ref["dQda"]),
             "pvec": cols(L.readback(capi.TAP_OUTPUT)[:B], ref["pvec"]), "q": dev(L.dpg_readback(3), ref["q"]),
             "outGradA": cols(L.readback(capi.TAP_OUTGRAD), ref["Ga"]), "outGradC": dev(L.dpg_readback(4), ref["Gc"]),
             "gradA": blk(L.readback(capi.TAP_GRADSUM), ref["ga"], ref["la"]), "gradC": blk(L.dpg_readback(5), ref["gc"], ref["lc"])}
    for (k, t), vals in zip(samples, ref["wb"]):      # setMseDklImpw, setValues(t, p, q)
        for f, v in zip(FIELDS, vals):
            want[k][f][t] = v
    for (k, t), Vn in zip(samples, ref["nxt"]):      # setValues(t + 1, Q~_next) where t + 1 is not itself sampled
        if Vn is not None:
            want[k]["V"][t + 1], want[k]["ADV"][t + 1] = Vn, 0.0
    for p, e in enumerate(order):
        for f, fid in FIELDS.items():
            worst[f] = max(worst.get(f, 0), dev(L.episode_field(p, fid), want[e["tag"]][f]))
    print(worst)
    L.close()
    assert all(v <= TOL32 for v in worst.values()), worst


@pytest.mark.gpu
@pytest.mark.parametrize("delay", [0.25, 2, 0])
def test_target_weights_follow_the_rule_and_the_checkpoint(hip_api, delay, tmp_path):
    L, eps, order, flat = learner(hip_api, SHAPES["A"], delay)
    tgt = [L.dpg_get_target(0), L.dpg_get_target(1)]
    assert np.array_equal(tgt[0], L.get_params()[0]) and np.array_equal(tgt[1], L.dpg_get_critic()[0])
    for k in range(3):
        L.step(1, flat)
        for which, w in enumerate((L.get_params()[0], L.dpg_get_critic()[0])):
            got = L.dpg_get_target(which)
            if 0 < delay < 1:
                want = (tgt[which].astype(np.float64) + delay * (w - tgt[which]).astype(np.float64)).astype(np.float32)
                assert np.all(np.abs(got - want) <= np.spacing(np.abs(want))), (k, which)
            else:
                want = w if (delay >= 1 and k % int(delay) == 0) else tgt[which]
                assert np.array_equal(got, want), (k, which)
            tgt[which] = got
    base = str(tmp_path / "agent_00_net")
    saved = [L.get_params(), L.dpg_get_critic(), tgt]
    L.save(base)
    zero = lambda n: np.zeros(n, np.float32)
    L.set_params(zero(L.nParams), zero(L.nParams), zero(L.nParams)); L.dpg_set_critic(zero(L.nCritic), zero(L.nCritic), zero(L.nCritic))
    L.dpg_set_target(0, zero(L.nParams)); L.dpg_set_target(1, zero(L.nCritic)); L.restart(base)
    for a, b in zip(saved[0] + saved[1] + tuple(saved[2]), L.get_params() + L.dpg_get_critic() + (L.dpg_get_target(0), L.dpg_get_target(1))):
        assert np.array_equal(a, b)      # the four blobs of each net, bit for bit
    (tmp_path / "agent_00_net_tgt_weights.raw").unlink(); (tmp_path / "agent_00_net_critic_tgt_weights.raw").unlink(); L.restart(base)
    assert np.array_equal(L.dpg_get_target(0), saved[0][0]) and np.array_equal(L.dpg_get_target(1), saved[1][0])      # a missing file: a copy of the weights
    L.close()


@pytest.mark.gpu
def test_statistics_of_the_1000th_step_move_with_ten_times_the_rate(hip_api):
    """The DPG constructor multiplies settings.learnrate by 10 and never resets it; the replay reads the same object, so
    MemoryProcessing::updateRewardsStats (every 1000th step, rRateFac 10) weighs the new moments with min(1, 10 x 10 x learnrate)."""
    lr, shape = 1e-4, SHAPES["A"]
    L, eps, order, flat = learner(hip_api, shape, learnrate=lr)
    mean, scale, r3 = L.get_scaling()
    L.set_scaling(mean + 0.5, scale * 0.8, [r3[0] - 0.3, r3[1] * 1.25, r3[2] / 1.25])      # (away from the sample moments hl_initialize set)
    L.step(999)
    mean, scale, r3 = [a.astype(np.float64) for a in L.get_scaling()]
    L.step(1)
    W = min(1.0, 10 * 10 * lr)
    def moved(m, sd, x):      # updateStats on E[x - m], E[(x - m)^2] over the stored transitions
        e1, e2 = (x - m).mean(0), ((x - m) ** 2).mean(0)
        return m + W * e1, sd + W * (np.sqrt(np.maximum(e2 - e1 * e1 * (2 * W - W * W), np.finfo(np.float32).eps)) - sd)
    sm, ss = moved(mean, 1 / scale, np.concatenate([e["S"][:N - 1] for e in eps]).astype(np.float64))
    rm, rs = moved(r3[0], r3[2], np.concatenate([e["R"][1:] for e in eps]))      # (EP.rewards[j + 1], j < ndata: MemoryProcessing.cpp:122)
    gm, gs, g3 = L.get_scaling()
    L.close()
    worst = {"stateMean": dev(gm, sm), "stateScale": dev(gs, 1 / ss), "rewMean": dev(g3[0], rm), "rewStd": dev(g3[2], rs), "rewScale": dev(g3[1], 1 / rs)}
    assert dev(sm, mean) > 100 * TOL32 and all(v <= TOL32 for v in worst.values()), worst      # (the statistics did move)


@pytest.mark.gpu
def test_routes_that_are_not_wired_and_foreign_handles(hip_api):
    L, eps, order, flat = learner(hip_api, SHAPES["A"])
    r = C.c_void_p()      # HL_ERR_UNSUPPORTED (8) with a message that names DPG
    calls = {"policy_snapshot": (), "act_dev_source": (1,), "rollout_create": (4, 8, 1, 0, C.byref(r)), "forward_dev": (0, None, None, None),
             "select_actions_dev": (0,) + (None,) * 7, "forward_sequences_dev": (0, None, None, 0, None, None, None),
             "select_actions_sequences_dev": (0, None, None, 0) + (None,) * 7}
    for name, args in calls.items():      # each message names its call and DPG
        assert hip_api.fn(name)(L.h, *args) == 8
        msg = hip_api.fn("last_error")(L.h)
        assert b"DPG" in msg and ("hl_" + name).encode() in msg, msg
    w = np.zeros(L.nParams, np.float32)      # HL_ERR_BAD_ARG (1): the NAF and DQN getters on a DPG handle, the DPG getters on another kind
    assert hip_api.fn("naf_get_target")(L.h, w.ctypes.data_as(C.POINTER(C.c_float))) == 1
    assert hip_api.fn("dqn_get_target")(L.h, w.ctypes.data_as(C.POINTER(C.c_float))) == 1
    L.close()
    V = capi.Learner(hip_api, capi.make_config(dimS=5, dimA=2, bounded=[0, 0], hidden=(32,), batchSize=8, maxTotObsNum=2000))
    assert hip_api.fn("dpg_get_target")(V.h, 0, np.zeros(V.nParams, np.float32).ctypes.data_as(C.POINTER(C.c_float))) == 1
    assert hip_api.fn("dpg_critic_num_params")(V.h) == -1
    V.close()


REFUSED = {"retrace": dict(returnsEstimator="retrace"), "GAE": dict(returnsEstimator="GAE"), "recurrent": dict(nn_type=1),
           "encoder_rnn": dict(encoder=(16,), encoder_rnn=1), "encoder": dict(encoder=(16,)), "ranks": dict(n_ranks=2), "dimA": dict(dimA=17, bounded=[0] * 17),
           "conv": dict(dimS=64, conv=[(8, 8, 1, 4, 3, 1)]), "appended": dict(nAppendedObs=1), "dimS": dict(dimS=513), "batch": dict(batchSize=1040),
           "width": dict(hidden=(528,)), "lds": dict(hidden=(512, 512, 512))}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals(hip_api, name):
    kw = dict(dict(dimS=6, dimA=3, hidden=(32,), batchSize=8, maxTotObsNum=4096, returnsEstimator="none"), **REFUSED[name])
    kw.setdefault("bounded", [0] * kw["dimA"])
    with pytest.raises(capi.HlError) as e:
        capi.create_dpg(hip_api, 0.01, **kw)
    assert e.value.status == 8 and "DPG" in str(e.value), e.value
