"""DQN learners (hl_create_dqn) against a plain numpy fp64 restatement of one DQN step -- the dense net and the formulas of the head
(headdq.hip) -- at the per-block parity tests' bound (tests/blocks.py: TOL32, each output column / parameter block on its own scale).
The restatement takes plain arrays: tests/test_dqn_cpu.py holds its fp32 network to a third of the bound on a machine without a GPU.
A first step moves beta off 1 (one sample of eight is far-policy), so the compared step carries the penalty term; rewards of order one
keep |e| away from zero."""
import ctypes as C

import numpy as np
import pytest

from smarties_amd import capi
from blocks import TOL32
from parity import relinf

DS, GAMMA, CLIP, LR = 5, 0.9, 4.0, 1e-3
VALUES = [(2,), (3, 6), (64,), (65,), (200,), (512,)]      # minimum; several variables, partial column tile; tile edge; one past; odd; cap
HIDDEN = [(24, 24), (40, 264)]                             # the second: no multiple of a K chunk, beyond 256
MODES = [("none", 0.01), ("none", 0), ("retrace", 0.01)]   # (estimator, targetDelay)
CASES = [(v, h, e, d, 8) for v in VALUES for h in HIDDEN for e, d in MODES] + [((65,), (24, 24), e, d, 40) for e, d in MODES]
FIELDS = dict(deltaQ=capi.EP_DELTAQ, dKL=capi.EP_DKL, impW=capi.EP_IMPW, V=capi.EP_VALUE, ADV=capi.EP_ADVANTAGE)


def episodes(B):
    """-> (steps per episode, sampled (episode, t)): three episodes -- terminated, truncated, terminated --, every other step sampled, so
    a terminal and a truncated next state are sampled and no two sampled steps are adjacent (B = 8: the NAF test's layout)"""
    N = 6 if B == 8 else 28
    return N, [(e, t) for e in (0, 1) for t in range(0, N - 1, 2)] + [(2, t) for t in range(1, 2 * (B - N) + 1, 2)]


def replay(values, B, seed=3):
    rng = np.random.RandomState(seed); N, _ = episodes(B); nOpt = int(np.prod(values)); eps = []
    for tag in range(3):
        mu = np.exp(0.3 * rng.randn(N, nOpt)); mu /= mu.sum(1, keepdims=True)      # rho stays inside [1 / C, C]
        act = np.stack([rng.randint(0, v, N) for v in values], 1).astype(np.float64)
        if tag == 0:      # step (0, 2) is far-policy: the behaviour policy found its action unlikely, the net's policy does not
            a = label(act[2], values); mu[2, a] *= 0.02; mu[2] /= mu[2].sum()
        eps.append(dict(S=rng.randn(N, DS).astype(np.float32), A=act, MU=mu, R=1 + rng.rand(N), V=rng.randn(N).astype(np.float32), term=int(tag != 1), tag=tag))
    return eps


def label(a, values):
    return int(np.dot(np.floor(a), np.concatenate([[1], np.cumprod(values)[:-1]])))


def layout(dS, hidden, nOpt):
    """the blob's layers: input, dense 1, (dense, residual) ..., output; every block on a multiple of 8 floats -> indW, indB, nParams"""
    up = lambda n: -(-n // 8) * 8
    sizes, prev = [(0, 0)], dS
    for j, h in enumerate(hidden):
        sizes += [(up(h) * prev, h)] + ([(h, h)] if j else []); prev = h
    sizes.append((up(nOpt) * prev, nOpt))
    indW, indB, tot = [], [], 0
    for w, b in sizes:
        indW.append(tot); tot += up(w); indB.append(tot); tot += up(b)
    return dict(indW=indW, indB=indB), tot


def outputs(W, lay, hidden, X, nOpt, dt=np.float64):
    """-> Q [n][nOpt] in fp64 from a network in `dt`, and what the backward pass needs"""
    W = W.astype(dt); inp = X.astype(dt); keep = []; l = 1
    for j, size in enumerate(hidden):
        ld = -(-size // 8) * 8; nIn = inp.shape[1]
        Wj = W[lay["indW"][l]:lay["indW"][l] + nIn * ld].reshape(nIn, ld)[:, :size]
        x = inp @ Wj + W[lay["indB"][l]:lay["indB"][l] + size]; y = x / (1 + np.abs(x)); l += 1      # SoftSign
        rec = dict(inp=inp, x=x, iW=lay["indW"][l - 1], iB=lay["indB"][l - 1], ld=ld, r=0)
        if j > 0:
            r = min(nIn, size); wr = W[lay["indW"][l]:lay["indW"][l] + r]; br = W[lay["indB"][l]:lay["indB"][l] + r]
            y = y.copy(); y[:, :r] += inp[:, :r] * wr + br
            rec.update(r=r, iWr=lay["indW"][l], iBr=lay["indB"][l]); l += 1
        keep.append(rec); inp = y
    ld = -(-nOpt // 8) * 8; H = inp.shape[1]
    Wo = W[lay["indW"][l]:lay["indW"][l] + H * ld].reshape(H, ld)[:, :nOpt]
    Q = inp @ Wo + W[lay["indB"][l]:lay["indB"][l] + nOpt]
    return Q.astype(np.float64), dict(y=inp, keep=keep, Wo=Wo, l=l, ld=ld)


def policy(Q):
    u = np.exp(np.clip(Q, -8, 8)); Z = max(u.sum(), np.finfo(np.float64).eps)
    return u, Z, u / Z


def head(Q, a, mu, target, beta, Cmax, Cinv):
    """one sample: section 2 of the issue -> gradient [nOpt], e, D_KL, rho, V, Q_a, far"""
    u, Z, p = policy(Q); rho = p[a] / mu[a]; lr = np.log(p / mu); dkl = np.sum(p * lr)
    far = bool(np.float32(Cmax) > 1 and (np.float32(rho) > np.float32(Cmax) or np.float32(rho) < np.float32(Cinv)))
    e = target - Q[a]; g = np.zeros_like(Q); g[a] = e
    if Cmax > 1:
        tau = -(1 + lr) / Z
        g = beta * (0 * g if far else g) + (1 - beta) * u * (tau - tau @ p)
    return g, e, dkl, rho, p @ Q, Q[a], far


def restate(W, Wt, lay, nParams, hidden, nOpt, X, X1, lab, MU, tgt, beta, Cmax, Cinv, dt=np.float64):
    """one step from plain arrays.  tgt: dict(r=[B] scaled rewards, term=[B] t+1 terminal) for "none" or dict(ret=[B]); Wt: the target
    blob or None (no target net) -> outputs, output gradients, write-backs, sum_i p^_i Q^_i of the live net on s_{t+1}, weight gradient"""
    Q, fw = outputs(W, lay, hidden, X, nOpt, dt); Qh = outputs(W, lay, hidden, X1, nOpt, dt)[0]
    Qt = Qh if Wt is None else outputs(Wt, lay, hidden, X1, nOpt, dt)[0]
    G = np.zeros_like(Q); wb = []; nfar = 0
    for b in range(len(X)):
        target = tgt["ret"][b] if "ret" in tgt else tgt["r"][b] + (0 if tgt["term"][b] else GAMMA * (policy(Qh[b])[2] @ Qt[b]))
        G[b], e, dkl, rho, V, Qa, far = head(Q[b], lab[b], MU[b], target, beta, Cmax, Cinv); nfar += far
        wb.append((e, dkl, rho, V, Qa - V))
    g = np.zeros(nParams); l = fw["l"]; H = fw["y"].shape[1]      # back-propagation: the summed weight gradient in the blob's layout
    blk = np.zeros((H, fw["ld"])); blk[:, :nOpt] = fw["y"].T @ G; g[lay["indW"][l]:lay["indW"][l] + blk.size] = blk.ravel()
    g[lay["indB"][l]:lay["indB"][l] + nOpt] = G.sum(0)
    k = fw["keep"][-1]; r = k["r"]; dres = G @ fw["Wo"].T      # ... and of the last hidden block; the blocks in front are left at zero
    if r:
        g[k["iWr"]:k["iWr"] + r] = (dres[:, :r] * k["inp"][:, :r]).sum(0); g[k["iBr"]:k["iBr"] + r] = dres[:, :r].sum(0)
    dl = dres / (1 + np.abs(k["x"])) ** 2; size = dl.shape[1]
    blk = np.zeros((k["inp"].shape[1], k["ld"])); blk[:, :size] = k["inp"].T @ dl; g[k["iW"]:k["iW"] + blk.size] = blk.ravel()
    g[k["iB"]:k["iB"] + size] = dl.sum(0)
    return dict(O=Q, G=G, wb=wb, vnext=np.array([policy(q)[2] @ q for q in Qh]), gradsum=g, nfar=nfar)


def dev(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return 0.0 if not np.any(ref) and not np.any(a) else relinf(a, ref)


def worst(got, ref, lay, hidden, nOpt):
    """largest deviation of the output gradients per column and of the weight gradient per block: the last hidden block (+ its
    residual) and the output layer"""
    nl = len(lay["indW"]); first = nl - (3 if len(hidden) > 1 else 2); up = lambda n: -(-n // 8) * 8
    ends = sorted(lay["indW"] + lay["indB"] + [len(ref["gradsum"])])
    blocks = [(i, ends[ends.index(i) + 1]) for l in range(first, nl) for i in (lay["indW"][l], lay["indB"][l])]
    return max([dev(got["G"][:, c], ref["G"][:, c]) for c in range(nOpt)] + [dev(got["gradsum"][i:j], ref["gradsum"][i:j]) for i, j in blocks if j > i])


def learner(hip_api, values, hidden, est, delay, B=8):
    L = capi.create_dqn(hip_api, delay, values, dimS=DS, hidden=hidden, batchSize=B, maxTotObsNum=4096, gamma=GAMMA, clipImpWeight=CLIP,
                        returnsEstimator=est, learnrate=LR, penalTol=0.01, randSeed=7)      # (one far-policy step of the stored 15 / 81 is beyond penalTol)
    L.init_weights(); eps = replay(values, B)
    for e in eps:
        L.append_episode(e["S"], e["A"], e["MU"], e["R"], e["V"], e["term"], e["tag"])
    L.initialize()
    order = eps[::-1]      # position 0 = newest; a flat index = transitions of the episodes in front + t
    prefix = np.concatenate([[0], np.cumsum([len(e["R"]) - 1 for e in order])])
    flat = np.asarray(sorted(prefix[len(eps) - 1 - k] + t for k, t in episodes(B)[1]), np.int64)
    return L, eps, order, flat


@pytest.mark.gpu
@pytest.mark.parametrize("values,hidden,est,delay,B", CASES)
def test_head_and_step_against_the_restatement(hip_api, values, hidden, est, delay, B):
    nOpt = int(np.prod(values)); none = est == "none"
    L, eps, order, flat = learner(hip_api, values, hidden, est, delay, B)
    L.step(1, flat)      # (beta leaves 1: the compared step mixes the penalty in)
    W0, Wt0, sc = L.get_params()[0], L.dqn_get_target(), L.scalars()
    assert sc.beta < 1 and L.nOut == nOpt
    want = {e["tag"]: {k: L.episode_field(p, f).astype(np.float64) for k, f in FIELDS.items()} for p, e in enumerate(order)}
    ret = {e["tag"]: L.episode_field(p, capi.EP_RETURN) for p, e in enumerate(order)}      # the return estimates the step reads
    L.step(1, flat)
    tags, ts = L.readback(capi.TAP_TAG), L.readback(capi.TAP_TSTEP)
    assert sorted(zip(tags, ts)) == sorted(episodes(B)[1])
    assert L.readback(capi.TAP_FAR).sum() == 1      # exactly the step built to be far-policy
    mean, scale, r3 = L.get_scaling(); N = episodes(B)[0]
    X, X1 = [np.stack([(eps[e]["S"][t + d] - mean) * scale for e, t in zip(tags, ts)]) for d in (0, 1)]
    lab = [label(eps[e]["A"][t], values) for e, t in zip(tags, ts)]; MU = np.stack([eps[e]["MU"][t] for e, t in zip(tags, ts)])
    tgt = dict(ret=np.array([ret[e][t] for e, t in zip(tags, ts)], np.float64)) if not none else dict(
        r=np.array([np.float32((eps[e]["R"][t] - np.float64(r3[0])) * np.float64(r3[1])) for e, t in zip(tags, ts)], np.float64),
        term=[t + 2 == N and eps[e]["term"] for e, t in zip(tags, ts)])
    lay, nP = layout(DS, hidden, nOpt); ll = L.layout()
    assert nP == L.nParams and lay["indW"] == list(ll["indW"]) and lay["indB"] == list(ll["indB"])
    args = (lay, nP, hidden, nOpt, X, X1, lab, MU, tgt, sc.beta, sc.CmaxRet, sc.CinvRet)
    ref = restate(W0, Wt0 if delay > 0 else None, *args)
    ref32 = restate(W0, Wt0 if delay > 0 else None, *args, dt=np.float32)      # the fp32 network alone: a third of the bound
    assert ref["nfar"] == 1 and worst(ref32, ref, lay, hidden, nOpt) <= TOL32 / 3
    got = dict(G=L.readback(capi.TAP_OUTGRAD), gradsum=L.readback(capi.TAP_GRADSUM))
    w = {"O": max(dev(L.readback(capi.TAP_OUTPUT)[:, c], ref["O"][:, c]) for c in range(nOpt)), "grad": worst(got, ref, lay, hidden, nOpt)}
    for (e, t), vals, vn in zip(zip(tags, ts), ref["wb"], ref["vnext"]):      # setMseDklImpw, setValues(t, V, Q); then setValues(t + 1, V_next)
        for k, v in zip(FIELDS, vals):
            want[e][k][t] = v
        if not none and t + 2 == N and not eps[e]["term"]:
            want[e]["V"][t + 1], want[e]["ADV"][t + 1] = vn, 0.0
    for p, e in enumerate(order):
        for k, f in FIELDS.items():
            w[k] = max(w.get(k, 0), dev(L.episode_field(p, f), want[e["tag"]][k]))
    print(w)
    L.close()
    assert all(v <= TOL32 for v in w.values()), w


@pytest.mark.gpu
@pytest.mark.parametrize("delay", [0.25, 3, 0])
def test_target_weights_follow_the_rule_and_the_checkpoint(hip_api, delay, tmp_path):
    L, eps, order, flat = learner(hip_api, (3, 6), (24, 24), "none", delay)
    tgt = L.dqn_get_target()
    assert np.array_equal(tgt, L.get_params()[0])
    for k in range(4):
        L.step(1, flat)
        w = L.get_params()[0]
        if 0 < delay < 1:
            want = (tgt.astype(np.float64) + delay * (w - tgt).astype(np.float64)).astype(np.float32)
            got = L.dqn_get_target()
            assert np.all(np.abs(got - want) <= np.spacing(np.abs(want))), k
            tgt = got
        else:
            tgt = w if (delay >= 1 and k % int(delay) == 0) else tgt
            assert np.array_equal(L.dqn_get_target(), tgt), k
    base = str(tmp_path / "agent_00_net")
    L.save(base)
    L.dqn_set_target(np.zeros_like(tgt)); L.restart(base)
    assert np.array_equal(L.dqn_get_target(), tgt)
    (tmp_path / "agent_00_net_tgt_weights.raw").unlink(); L.restart(base)
    assert np.array_equal(L.dqn_get_target(), w)
    L.close()


@pytest.mark.gpu
def test_acting_outputs_and_the_routes_that_are_not_wired(hip_api):
    values, hidden = (3, 6), (24, 24)
    L, eps, order, flat = learner(hip_api, values, hidden, "retrace", 0.01)
    S = np.random.RandomState(1).randn(4, DS).astype(np.float32)
    mean, scale, _ = L.get_scaling()
    ref = outputs(L.get_params()[0], layout(DS, hidden, 18)[0], hidden, (S - mean) * scale, 18)[0]
    O = L.forward(S)
    assert O.shape == (4, 18) and max(dev(O[:, c], ref[:, c]) for c in range(18)) <= TOL32
    r = C.c_void_p()      # HL_ERR_UNSUPPORTED (8) with a message that names DQN
    for rc in (hip_api.fn("policy_snapshot")(L.h), hip_api.fn("act_dev_source")(L.h, 1), hip_api.fn("rollout_create")(L.h, 4, 8, 1, 0, C.byref(r)),
               hip_api.fn("forward_dev")(L.h, 0, None, None, None)):
        assert rc == 8 and b"DQN" in hip_api.fn("last_error")(L.h)
    w = np.zeros(L.nParams, np.float32)
    assert hip_api.fn("naf_get_target")(L.h, w.ctypes.data_as(C.POINTER(C.c_float))) == 1      # HL_ERR_BAD_ARG: no NAF learner
    L.close()
    with pytest.raises(capi.HlError) as e:
        capi.create_dqn(hip_api, 0.01, (513,), dimS=DS, hidden=hidden, batchSize=8, maxTotObsNum=4096)
    assert e.value.status == 8 and "DQN" in str(e.value)
