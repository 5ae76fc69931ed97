"""PPO learners (hl_create_ppo) against a plain numpy fp64 restatement of one PPO step (PPO::Train, updatePenalizationCoef), at the
bound of the NAF, DQN and DPG tests: 1e-5 relative, each column / block on its own scale.  tests/test_ppo_cpu.py holds the same
restatement in fp32 to a third of it.  The networks' restatement (layout, forward, backward) is tests/test_hip_dpg.py's."""
import ctypes as C

import numpy as np
import pytest

from smarties_amd import capi
from blocks import TOL32
from test_hip_dpg import backward, dev, forward, layout, sp, spd

GAMMA, LAMBDA, CLIP, NOISE, N, TGT, PEN0, LR = 0.5, 0.5, 0.2, 0.4472135955, 5, 0.005, 0.7, 1e-4
# name -> dimS, dimA, hidden, batch, option counts of the discrete action variables (None: continuous), bounded components
SHAPES = {"c1": (5, 1, (24,), 16, None, (0,)), "c6": (17, 6, (64, 40), 40, None, (1, 0, 1, 0, 0, 1)), "c16": (9, 16, (272, 272), 48, None, (0,) * 16),
          "d2": (5, 1, (32,), 16, (2,), (0,)), "d80": (7, 2, (64,), 32, (8, 10), (0, 0)), "d512": (6, 1, (64,), 32, (512,), (0,))}
# perturbation of the stored policy by row pattern b % 4: size d, sign of log rho -- (near, below) (near, between) (far high) (far low)
PATTERN = ((0.03, 1), (0.1, -1), (0.9, 1), (0.9, -1))


def n_out(shape):
    return (int(np.prod(shape[4])), 0) if shape[4] else (shape[1], shape[1])


def random_nets(shape, seed=11):
    """actor and critic weights of order 1 / sqrt(fan-in)"""
    dS, dA, hidden, _, values = shape[:5]; rng = np.random.RandomState(seed); nets = []; nD, nS = n_out(shape)
    for lay in (layout(dS, hidden, nD, nS), layout(dS, hidden, 1, 0)):
        W = np.zeros(lay["n"], np.float32)
        for k in lay["hid"] + [lay["out"]]:
            small = 0.1 if (k is lay["out"] and lay["iSig"] is not None) else 1.0      # (means of order 0.1: a - mean keeps its digits in fp32)
            W[k["iW"]:k["iW"] + k["nIn"] * k["ld"]] = small * rng.uniform(-1, 1, k["nIn"] * k["ld"]) * np.sqrt(3.0 / k["nIn"])
            W[k["iB"]:k["iB"] + k["size"]] = 0.1 * rng.randn(k["size"])
            if k.get("r"):
                W[k["iWr"]:k["iWr"] + k["r"]] = 1 + 0.1 * rng.randn(k["r"]); W[k["iBr"]:k["iBr"] + k["r"]] = 0.1 * rng.randn(k["r"])
        if lay["iSig"] is not None:
            W[lay["iSig"]:lay["iSig"] + dA] = (NOISE ** 2 - 0.25) / NOISE + 0.05 * rng.randn(dA)
        nets.append(W)
    return nets


def episodes(shape, Wa, seed=3):
    """B / 4 episodes of N states; the stored policy is the actor's own on the RAW states (statistics mean 0, scale 1: the tests set
    them), moved by PATTERN[b % 4]; rewards carry the sign (-1)^(b // 4), so that both clip rules meet both signs of the return"""
    dS, dA, hidden, B, values = shape[:5]; rng = np.random.RandomState(seed); eps = []; nD, nS = n_out(shape); la = layout(dS, hidden, nD, nS)
    for tag in range(B // (N - 1)):
        S = rng.randn(N, dS).astype(np.float32); out = forward(Wa, la, S, np.float64)[0]; R = np.zeros(N); mu = np.zeros((N, 2 * dA if not values else nD))
        act = np.zeros((N, dA))
        for t in range(N):
            b = tag * (N - 1) + t; d, sgn = PATTERN[b % 4]; R[t] = (1 + rng.rand()) * (-1) ** ((b - 1) // 4)      # (R[t + 1] belongs to row b = t)
            if values:
                p = sp(out[t]); p /= p.sum(); z = np.where(rng.rand(nD) < 0.5, -1.0, 1.0); label = int(rng.randint(nD)); z[label] = -sgn
                m = p * np.exp(d * z); mu[t] = m / m.sum()
                for i, v in enumerate(values):
                    act[t, i] = label % v + 0.25; label //= v
            else:
                std = sp(Wa[la["iSig"]:la["iSig"] + dA].astype(np.float64)); u = rng.randn(dA); u *= d / np.sqrt(u @ u)
                mu[t, :dA] = out[t] + u * std; mu[t, dA:] = std * 1.002
                act[t] = (out[t] if sgn > 0 else mu[t, :dA]) + 0.1 * std * rng.randn(dA)
        eps.append(dict(S=S, A=act, MU=mu, R=R, V=(0.1 * rng.randn(N)).astype(np.float32), term=tag % 2, tag=tag))
    return eps


def chain(stats, pen, tgt):
    """the serial bookkeeping of PPO::Train over (DKL, RHO, isOff) in ascending row order, then updatePenalizationCoef -> penalCoef, DKL_target"""
    cnt, delta = 0.0, 0.0
    for dkl, rho, off in stats:
        cnt += 1      # the two tests on the old DKL_target, then updateDKL_target(isOff, RHO)
        delta -= pen / 2 if dkl < tgt / 1.5 else 0
        delta += pen if dkl > 1.5 * tgt else 0
        tgt = tgt * 0.9995 if (off and tgt > rho) else (tgt * 1.0001 if (not off and tgt < rho) else tgt)
    return max(pen + 1e-4 * delta / max(1.0, cnt), float(np.finfo(np.float32).eps)), tgt


def ppo_step(nets, shape, rows, pen, tgt, lr_eff, dt=np.float64):
    """one PPO step on `rows` (dicts s, a, mu, ret, vold): the networks in `dt`, the head and the scalar chain in fp64"""
    dS, dA, hidden, B, values = shape[:5]; Wa, Wc = nets; nD, nS = n_out(shape)
    la, lc = layout(dS, hidden, nD, nS), layout(dS, hidden, 1, 0)
    S = np.stack([r["s"] for r in rows]); P, fa = forward(Wa, la, S, dt); V, fc = forward(Wc, lc, S, dt)
    P, V = P.astype(np.float64), V[:, 0].astype(np.float64); G = np.zeros((len(rows), nD + nS)); Gc = np.zeros((len(rows), 1))
    out = dict(P=P, V=V, rho=[], dkl=[], off=[], gain=[], zero=[], wb=[], la=la, lc=lc)
    if not values:
        sig = Wa[la["iSig"]:la["iSig"] + dA].astype(np.float64); std = sp(sig); out["P"] = np.concatenate([P, np.tile(sig, (len(rows), 1))], 1)
    pen0 = pen
    for b, r in enumerate(rows):
        ret, vold = float(r["ret"]), float(r["vold"])
        if values:
            label = int(sum(np.floor(a) * s for a, s in zip(r["a"], np.cumprod((1,) + values[:-1]))))
            un = sp(P[b]); Z = un.sum(); p = un / Z; rho = p[label] / r["mu"][label]; dkl = np.sum(p * np.log(p / r["mu"]))
        else:
            bm, bs = r["mu"][:dA], r["mu"][dA:]; m = P[b]; mc = np.where(np.asarray(shape[5], bool), np.clip(m, -8.31776613503286, 8.31776613503286), m)
            rho = np.exp(np.clip(np.sum(((r["a"] - bm) / bs) ** 2 - ((r["a"] - mc) / std) ** 2) / 2 - np.sum(np.log(std / bs)), -7, 7))
            dkl = np.sum((std / bs) ** 2 - 1 + ((m - bm) / bs) ** 2 - 2 * np.log(std / bs)) / 2
        off = bool(np.float32(rho) > np.float32(1) + np.float32(CLIP) or np.float32(rho) < np.float32(1) - np.float32(CLIP))
        gain = rho * (ret - vold); zero = (ret > 0 and rho > 1 + CLIP, ret < 0 and rho < 1 - CLIP)
        gain = 0.0 if any(zero) else gain
        if values:      # policyGradient(label, gain) + 0 x KLDivGradient(mu, -penalCoef)
            pol = -gain / Z * np.ones(nD); pol[label] += gain / un[label]
            tmp = -pen0 * (1 + np.log(p / r["mu"])) / Z; G[b] = (1 * pol + 0 * (tmp - np.sum(tmp * p))) * spd(P[b])
        else:
            u = (r["a"] - mc) / std; gm = gain * (r["a"] - m) / std ** 2      # (a bounded component's mean: clipped in u, and no push further into the clip)
            gm = np.where((np.abs(m) >= 8.31776613503286) & (gm * np.sign(m) > 0) & np.asarray(shape[5], bool), 0.0, gm)
            G[b, :dA] = 1 * gm + 0 * (-pen0 * (m - bm) / bs ** 2)
            G[b, dA:] = spd(sig) * (1 * gain * (u * u - 1) / std + 0 * (-pen0 * (1 / bs ** 2 - 1 / std ** 2) * std))
        Gc[b, 0] = np.float32((ret - V[b]) * (1 if off else 0))
        for k, v in zip(("rho", "dkl", "off", "gain", "zero"), (rho, dkl, off, gain, zero)):
            out[k].append(v)
        out["wb"].append((ret - V[b], dkl, rho, V[b], 0.0))
    ga = backward(la, fa, G[:, :nD])[0]
    if not values:
        ga[la["iSig"]:la["iSig"] + dA] = G[:, dA:].sum(0)
    gc = backward(lc, fc, Gc)[0]
    pen1, tgt1 = chain(zip(out["dkl"], out["rho"], out["off"]), pen0, tgt)
    out.update(G=G, Gc=Gc[:, 0], ga=ga, gc=gc, pen=pen1, tgt=tgt1)
    out["Wa"], out["Wc"] = adam(Wa, ga / len(rows), lr_eff), adam(Wc, gc / len(rows), np.float32(lr_eff) * np.float32(3))
    return out


def adam(W, g, eta, lam=0.0):
    """the first Adam step from zero moments (Optimizer.cpp:61-108: Nesterov, safe, AdamW with nnLambda 0 here)"""
    dw = g.astype(np.float64); m1 = 0.1 * dw; m2 = np.maximum(0.001 * dw * dw, m1 * m1)
    return W.astype(np.float64) + eta * ((0.9 * m1 + 0.1 * dw) / (np.finfo(np.float32).eps + np.sqrt(m2)) - lam * W)


def all_blocks(lay):
    """(offset, length) of every block of a blob: each layer's weights and biases, the residuals', the ParamLayer"""
    out = []
    for k in lay["hid"] + [lay["out"]]:
        out += [(k["iW"], k["nIn"] * k["ld"]), (k["iB"], k["size"])] + ([(k["iWr"], k["r"]), (k["iBr"], k["r"])] if k.get("r") else [])
    return out + ([(lay["iSig"], lay["out"]["size"])] if lay["iSig"] is not None else [])


def conditions(ref, tgt=TGT):
    """every branch of the head and of the chain is taken and not taken, and no row sits where fp32 outputs could flip one"""
    rho, dkl, off, zero = np.asarray(ref["rho"]), np.asarray(ref["dkl"]), np.asarray(ref["off"]), np.asarray(ref["zero"])
    assert off.any() and not off.all() and zero[:, 0].any() and zero[:, 1].any() and not zero.any(1).all()
    assert (dkl < tgt / 1.5).any() and (dkl > 1.5 * tgt).any() and ((dkl > tgt / 1.5) & (dkl < 1.5 * tgt)).any()
    assert min(np.abs(rho - x).min() for x in (1 + CLIP, 1 - CLIP, tgt)) > 1e-3
    assert min(np.abs(dkl / x - 1).min() for x in (tgt / 1.5, 1.5 * tgt)) > 1e-3


def learner(hip_api, shape, eps=None, nEpochs=2, horizon=None, **kw):
    dS, dA, hidden, B, values = shape[:5]
    L = capi.create_ppo(hip_api, TGT, nEpochs, values, dimS=dS, hidden=hidden, batchSize=B, maxTotObsNum=horizon or B, gamma=GAMMA, lambda_=LAMBDA,
                        clipImpWeight=CLIP, returnsEstimator="GAE", explNoise=NOISE, learnrate=LR, randSeed=7, **(dict(kw) if values else dict(kw, dimA=dA, bounded=list(shape[5]))))
    L.init_weights()
    for e in eps or []:
        L.append_episode(e["S"], e["A"], e["MU"], e["R"], e["V"], e["term"], e["tag"])
    return L


def rows_of(L, eps, samples):
    """the rows of a step: raw states (statistics 0 / 1), stored action and policy, the STORED return estimate and state value"""
    pos = {e["tag"]: len(eps) - 1 - k for k, e in enumerate(eps)}      # position 0 = newest
    ret = {k: L.episode_field(p, capi.EP_RETURN).astype(np.float64) for k, p in pos.items()}
    val = {k: L.episode_field(p, capi.EP_VALUE).astype(np.float64) for k, p in pos.items()}
    by = {e["tag"]: e for e in eps}
    return [dict(s=by[k]["S"][t], a=by[k]["A"][t], mu=by[k]["MU"][t], ret=ret[k][t], vold=val[k][t]) for k, t in samples]


FIELDS = dict(deltaQ=capi.EP_DELTAQ, dKL=capi.EP_DKL, impW=capi.EP_IMPW, V=capi.EP_VALUE, ADV=capi.EP_ADVANTAGE)


def check_step(L, shape, nets, eps, worst, nstep=1):
    """Adam step `nstep` of the device on every stored transition, from zero moments, against the restatement"""
    dS, dA, hidden, B, values = shape[:5]; nD, nS = n_out(shape)
    L.set_params(nets[0], np.zeros_like(nets[0]), np.zeros_like(nets[0])); L.ppo_set_critic(nets[1], np.zeros_like(nets[1]), np.zeros_like(nets[1]))
    st = L.ppo_state(); samples = [(e["tag"], t) for e in eps for t in range(N - 1)]
    order = eps[::-1]; rows = rows_of(L, eps, samples)
    want = {e["tag"]: {k: L.episode_field(p, f).astype(np.float64) for k, f in FIELDS.items()} for p, e in enumerate(order)}
    L.step(1, np.arange(B, dtype=np.int64))
    got = list(zip(L.readback(capi.TAP_TAG), L.readback(capi.TAP_TSTEP)))
    rows = [rows[samples.index(g)] for g in got]
    eta = np.float32(LR) * np.float32(np.sqrt(np.float32(1 - 0.999 ** nstep)) / np.float32(1 - 0.9 ** nstep))      # the bias-corrected rate (Optimizer.cpp:66)
    ref = ppo_step(nets, shape, rows, st.penalCoef, st.DKL_target, float(eta))
    conditions(ref, st.DKL_target)
    cols = lambda a, r: max(dev(a[:, c], r[:, c]) for c in range(r.shape[1]))
    blk = lambda a, r, lay: max(dev(a[i:i + n], r[i:i + n]) for i, n in all_blocks(lay))      # every block on its own scale
    assert list(L.ppo_readback(2).astype(bool)) == ref["off"]
    new = L.ppo_state()
    worst.update({"pvec": cols(L.readback(capi.TAP_OUTPUT)[:B], ref["P"]), "V": dev(L.ppo_readback(4), ref["V"]), "rho": dev(L.ppo_readback(0), ref["rho"]),
                  "dkl": dev(L.ppo_readback(1), ref["dkl"]), "gain": dev(L.ppo_readback(3), ref["gain"]), "outGradA": cols(L.readback(capi.TAP_OUTGRAD), ref["G"]),
                  "outGradC": dev(L.ppo_readback(5), ref["Gc"]), "gradA": blk(L.readback(capi.TAP_GRADSUM), ref["ga"], ref["la"]),
                  "gradC": blk(L.ppo_readback(6), ref["gc"], ref["lc"]),
                  "adamA": dev(L.get_params()[0], ref["Wa"]), "adamC": dev(L.ppo_get_critic()[0], ref["Wc"]),
                  "penalCoef": dev([new.penalCoef - st.penalCoef], [ref["pen"] - st.penalCoef]), "DKL_target": dev([new.DKL_target], [ref["tgt"]])})
    for (k, t), vals in zip(got, ref["wb"]):      # setMseDklImpw, setValues(t, V, V)
        for f, v in zip(FIELDS, vals):
            want[k][f][t] = v
    for p, e in enumerate(order):
        for f, fid in FIELDS.items():
            worst[f] = max(worst.get(f, 0), dev(L.episode_field(p, fid), want[e["tag"]][f]))


def prepared(hip_api, shape, **kw):
    nets = random_nets(shape); eps = episodes(shape, nets[0])
    L = learner(hip_api, shape, eps, **kw); L.initialize()
    dS = shape[0]; r3 = L.get_scaling()[2]
    L.set_scaling(np.zeros(dS, np.float32), np.ones(dS, np.float32), r3)      # (the stored policies were formed on the raw states)
    return L, nets, eps


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_step_against_the_restatement(hip_api, name):
    shape = SHAPES[name]
    L, nets, eps = prepared(hip_api, shape)
    assert L.nParams == nets[0].size and L.nCritic == nets[1].size and L.nOut == sum(n_out(shape))
    L.ppo_set_state(PEN0, TGT)
    worst = {}
    check_step(L, shape, nets, eps, worst)
    print(name, worst)
    L.close()
    assert all(v <= TOL32 for v in worst.values()), worst


@pytest.mark.gpu
def test_epochs_and_clear(hip_api):
    """nHorizon 64, batch 16, nEpochs 2: eight steps, the reward statistics move at steps 4 and 8 -- with 3 x learnrate, the constructor's
    factor that stays in the settings the replay reads (PPO_common.cpp:71, MemoryProcessing.cpp:102) --, then the replay is empty"""
    shape = (5, 1, (24,), 16, None, (0,)); big = shape[:3] + (64,) + shape[4:]
    nets = random_nets(shape); eps = episodes(big, nets[0])
    L = learner(hip_api, shape, eps[:-1], nEpochs=2, horizon=64); L.initialize()
    step = hip_api.fn("step")
    assert step(L.h, 1, None) == 4 and b"PPO" in hip_api.fn("last_error")(L.h)      # HL_ERR_STATE below nHorizon
    e = eps[-1]; L.append_episode(e["S"], e["A"], e["MU"], e["R"], e["V"], e["term"], e["tag"])
    assert step(L.h, 9, None) == 4 and L.counts()[2] == 0      # more than the steps left: none runs
    m, sc, r3 = L.get_scaling(); L.set_scaling(m, sc, [r3[0] - 0.3, r3[1], r3[2]])      # (away from the sample mean hl_initialize set)
    Rmean = np.mean(np.concatenate([e["R"][1:] for e in eps]))
    for k in range(1, 9):
        before = L.get_scaling()[2].copy(); L.step(1); st = L.ppo_state(); moved = not np.array_equal(before, L.get_scaling()[2])
        assert (st.cntBatch, st.cntEpoch, st.stepsLeft) == ((16 * k) % 64, (k // 4) % 2, 8 - k if k < 8 else 8) and moved == (k % 4 == 0), (k, moved)
        if moved:      # updateStats: mean += W (E[r] - mean), W = min(1, 1 x 3 learnrate)
            assert dev([L.get_scaling()[2][0]], [before[0] + 3 * LR * (Rmean - np.float64(before[0]))]) <= TOL32
    assert L.counts()[:3] == (0, 0, 8)
    assert step(L.h, 1, None) == 4      # empty: refused
    L.close()
    L, nets, eps = prepared(hip_api, shape)      # a fresh horizon after a clear: the step matches the restatement
    L.ppo_set_state(PEN0, TGT, 0, 1); L.step(1)      # (the last epoch's one step: cleared behind it)
    assert L.counts()[0] == 0
    L.set_scaling(np.zeros(shape[0], np.float32), np.ones(shape[0], np.float32), L.get_scaling()[2])      # (the first step's statistics moved them)
    eps = [dict(e, tag=e["tag"] + 100) for e in eps]
    for e in eps:
        L.append_episode(e["S"], e["A"], e["MU"], e["R"], e["V"], e["term"], e["tag"])
    L.ppo_set_state(PEN0, TGT); worst = {}
    check_step(L, shape, nets, eps, worst, nstep=2)
    L.close()
    assert all(v <= TOL32 for v in worst.values()), worst


REFUSED = {"recurrent": dict(nn_type=1), "encoder_rnn": dict(encoder=(16,), encoder_rnn=1), "encoder": dict(encoder=(16,)), "ranks": dict(n_ranks=2),
           "dimA": dict(dimA=17, bounded=[0] * 17), "conv": dict(dimS=64, conv=[(8, 8, 1, 4, 3, 1)]), "appended": dict(nAppendedObs=1), "dimS": dict(dimS=513),
           "batch": dict(batchSize=1040), "clip": dict(clipImpWeight=1.0), "epochs": dict(nEpochs=0), "options": dict(values=(23, 23))}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_values_forward_checkpoint_and_refusals(hip_api, name, tmp_path):
    kw = dict(dict(dimS=6, dimA=3, hidden=(32,), batchSize=8, maxTotObsNum=64, clipImpWeight=CLIP, returnsEstimator="GAE", nEpochs=1, values=None), **REFUSED[name])
    nE, values = kw.pop("nEpochs"), kw.pop("values")
    if not values:
        kw.setdefault("bounded", [0] * kw["dimA"])
    with pytest.raises(capi.HlError) as e:
        capi.create_ppo(hip_api, TGT, nE, values, **kw)
    assert e.value.status == 8 and "PPO" in str(e.value), e.value
    if name != "recurrent":      # the rest once
        return
    shape = SHAPES["c6"]; L, nets, eps = prepared(hip_api, shape); dS, dA = shape[:2]
    L.step(1)      # (moments that are not zero; the blobs' padding stays zero, as the checkpoint's format leaves it)
    base = str(tmp_path / "agent_00_net"); saved = L.get_params() + L.ppo_get_critic(); L.save(base)
    zero = lambda n: np.zeros(n, np.float32)
    L.set_params(zero(L.nParams), zero(L.nParams), zero(L.nParams)); L.ppo_set_critic(zero(L.nCritic), zero(L.nCritic), zero(L.nCritic)); L.restart(base)
    assert np.any(saved[1]) and np.any(saved[4]) and all(np.array_equal(a, b) for a, b in zip(saved, L.get_params() + L.ppo_get_critic()))
    L.set_params(nets[0]); L.ppo_set_critic(nets[1]); L.set_scaling(np.zeros(dS, np.float32), np.ones(dS, np.float32), L.get_scaling()[2])      # (the step's statistics moved them)
    Sx = np.random.RandomState(1).randn(37, dS).astype(np.float32)
    la, lc = layout(dS, shape[2], dA, dA), layout(dS, shape[2], 1, 0)
    worst = {"values": dev(L.ppo_values(Sx), forward(nets[1], lc, Sx, np.float64)[0][:, 0]),
             "forward": max(dev(L.forward(Sx)[:, c], forward(nets[0], la, Sx, np.float64)[0][:, c]) for c in range(dA))}
    assert all(v <= TOL32 for v in worst.values()), worst
    r = C.c_void_p()      # HL_ERR_UNSUPPORTED (8) with a message that names PPO
    calls = {"step_begin": (None,), "policy_snapshot": (), "act_dev_source": (1,), "rollout_create": (4, 8, 1, 0, C.byref(r)), "forward_dev": (0, None, None, None),
             "select_actions_dev": (0,) + (None,) * 7, "forward_sequences_dev": (0, None, None, 0, None, None, None),
             "select_actions_sequences_dev": (0, None, None, 0) + (None,) * 7}
    for call, args in calls.items():
        assert hip_api.fn(call)(L.h, *args) == 8 and b"PPO" in hip_api.fn("last_error")(L.h), call
    pf = C.POINTER(C.c_float); w = np.zeros(max(L.nParams, L.nCritic), np.float32).ctypes.data_as(pf)
    assert hip_api.fn("dpg_get_critic")(L.h, w, None, None) == 1 and hip_api.fn("naf_get_target")(L.h, w) == 1      # HL_ERR_BAD_ARG both ways
    L.close()
    V = capi.Learner(hip_api, capi.make_config(dimS=5, dimA=2, bounded=[0, 0], hidden=(32,), batchSize=8, maxTotObsNum=2000))
    assert hip_api.fn("ppo_get_critic")(V.h, w, None, None) == 1 and hip_api.fn("ppo_critic_num_params")(V.h) == -1
    assert hip_api.fn("ppo_get_state")(V.h, C.byref(capi.PpoState())) == 1
    V.close()
