"""Discrete actions of several variables and of up to 512 options (include/smarties_hip_discrete.h) on the GPU: several variables within
64 options against the CPU oracle on the flattened labels, the head launch beyond 64 options (headw.hip) against plain fp64 numpy, acting."""
import numpy as np
import pytest

from acting import TOL32, _net2v, head_np
from oracle_api import oracle_learner, synth_cfg, synth_episode
from parity import relinf
from smarties_amd import capi

U = 2.0 ** -53


def _message(labels, values):
    """ActionInfo::label2actionMessage (Core/StateAction.h:327-341) for an array of labels: [n][len(values)] entries index_i + 0.1"""
    shifts = np.concatenate([[1], np.cumprod(values)[:-1]])
    return (np.asarray(labels)[:, None] // shifts[None, :]) % np.asarray(values)[None, :] + 0.1


# ---- 2. several variables within 64 options: the oracle runs with one variable on the same labels.  (32, 32): the step chain's head
# (head_body.h); (64, 64): the wide fused kernel's (head_rows.h) ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("values,hidden", [((3, 4), (32, 32)), ((2, 2, 2, 2, 4), (32, 32)), ((3, 4), (64, 64))])
def test_several_variables_match_the_oracle_on_the_flattened_labels(hip_api, values, hidden):
    nopt = int(np.prod(values))
    kw = dict(dimS=6, bounded=[0], hidden=hidden, nnFunc="Tanh", batchSize=16, maxTotObsNum=4000, randSeed=5)
    G = capi.create_discrete(hip_api, values, **dict(kw, bounded=[0] * len(values)))
    O = oracle_learner(capi.make_config(dimA=1, adv_kind=capi.ADV_DISCRETE, n_options=nopt, **kw))
    sc = synth_cfg(seed=21, dimS=6, dimA=1, lenMin=5, lenMax=30, pTerm=0.5)
    G.init_weights(); O.init_weights()
    for e in range(24):
        ep = synth_episode(sc, e, nopt)
        O.append_episode(**ep)
        msg = _message(np.floor(ep["actions"][:, 0]).astype(np.int64), values)
        msg[-1] = 0.0      # (the last step carries no action: zeros, as the flattened episode)
        G.append_episode(**dict(ep, actions=msg))
    for L in (G, O):
        L.initialize(); L.set_tap(True)
    for _ in range(3):
        G.step(1); O.step(1)
        assert np.array_equal(G.readback(capi.TAP_FLAT), O.readback(capi.TAP_FLAT))
        assert np.array_equal(G.readback(capi.TAP_FAR), O.readback(capi.TAP_FAR))
        for tap in (capi.TAP_RHO, capi.TAP_DKL, capi.TAP_OUTGRAD, capi.TAP_GRADSUM):
            assert relinf(G.readback(tap), O.readback(tap)) < TOL32, tap
        assert G.scalars().nFarPolicySteps == O.scalars().nFarPolicySteps
    assert relinf(G.get_params()[0], O.get_params()[0]) < TOL32
    with pytest.raises(capi.HlError):      # an entry beyond its variable's count
        G.append_episode(**dict(ep, actions=np.full_like(msg, values[0] + 0.1)))


# ---- 3. the tiled head against plain fp64 numpy ----------------------------------------------------------------------------------------
def _head_reference(O, label, mu, Qret, beta, Cmax, Cinv):
    """head_body.h:181-219 for one sample in numpy float64: (rho, dkl, far, gradient row [g0 | gA | gP], fp64 margin per entry, DKL's scale).
    The margin: every sum of the head is formed in another order than here -- at most 8 terms per lane, six butterfly levels, numpy's
    pairwise tree, a log of 1-2 ulp on either side: fewer than 64 roundings of 2^-53, times the magnitudes that enter each entry"""
    n = mu.size
    adv, x = O[1:1 + n], O[1 + n:]
    un = (x + np.sqrt(1 + x * x)) / 2
    norm = max(un.sum(), np.finfo(np.float64).eps)
    p = un / norm
    assert np.abs(p - head_np(O, None, 1, n_options=n)[1]).max() <= 8 * U      # the probabilities, as the acting tests form them
    lr = np.log(p / mu)
    rho, dkl = p[label] / mu[label], float((p * lr).sum())
    far = bool(np.float32(Cmax) > 1 and (np.float32(rho) > np.float32(Cmax) or np.float32(rho) < np.float32(Cinv)))
    V, vdiff = _net2v(O[0]), 100 - 5000 / np.sqrt(2601 + 100 * abs(O[0]))
    A_RET = Qret - V
    dQ = A_RET - (adv[label] - (p * adv).sum())
    g0 = 0.0 if far else min(1.0, rho) * dQ * beta * vdiff
    Qer = 0.0 if far else beta * (min(Cmax, rho) * dQ)
    tmp, dpos, hot = -(1 + lr) / norm, (1 + x / np.sqrt(1 + x * x)) / 2, (np.arange(n) == label).astype(np.float64)
    tp = (tmp * p).sum()
    factor = 0.0 if far else A_RET * min(Cmax, rho)
    gP = beta * ((hot * factor / un - factor / norm) * dpos) + (1 - beta) * ((tmp - tp) * dpos)
    mag = abs(Qret) + abs(V) + np.abs(adv).max()                   # what enters dQ
    mP = 64 * U * ((1 - beta) * (np.abs(tmp).max() + abs(tp)) + beta * (abs(Qret) + abs(V)) * Cmax * (1 / un.min() + 1 / norm))
    margin = np.concatenate([[64 * U * mag * beta * abs(vdiff)], np.full(n, 64 * U * mag * beta * Cmax), np.full(n, mP)])
    return rho, dkl, far, np.concatenate([[g0], Qer * (hot - p), gP]), margin, np.abs(p * lr).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("values,H,out", [((65,), 32, "Linear"), ((128,), 32, "Linear"), ((10, 13), 32, "Linear"), ((8, 8, 8), 32, "Linear"),
                                          ((10, 13), 160, "Tanh")], ids=["65", "128", "10x13", "8x8x8", "10x13-h160-tanh"])
def test_wide_head_matches_fp64_numpy(hip_api, values, H, out):
    """65 / 128 / 130 / 512 options: one option in the second tile, a full second tile, a ragged tile behind a full one, the upper bound;
    160 hidden units under a Tanh output layer: three rounds of the backward's 64-unit loop, the last one ragged, and f'(x) on the deltas.
    Given transitions: t = 7 is a truncated episode's last one (a next-state row), odd t are far-policy (the label's behaviour probability
    a twentieth of uniform, rho ~ 20 > Cmax = 5), even t near (its double).  The net itself in numpy from the parameters: HL_TAP_OUTPUT,
    V(s') of the next rows and the hidden layer's bias gradient (Wo d f'(y): Dres / D) within the fp32 bound of the parity tests.
    RHO and DKL (fp64) within 64 x 2^-53 relative (DKL: of sum |p log(p / mu)|); every entry of the HL_TAP_OUTGRAD row -- (double)(float)g --
    within half a float ulp of the fp64 reference plus its fp64 margin (_head_reference).  Measured on an MI355X: RHO / DKL off by at most
    1.04e-15 (130 options; 8.0e-16 at 65, 4.9e-16 at 128, 9.1e-16 at 512) against that bound of 7.1e-15; no OUTGRAD entry beyond half a float ulp."""
    nopt, rng = int(np.prod(values)), np.random.default_rng(int(np.prod(values)))
    L = capi.create_discrete(hip_api, values, dimS=6, bounded=[0] * len(values), hidden=(H,), nnFunc="Tanh", nnOutputFunc=out, batchSize=8,
                             maxTotObsNum=4000, randSeed=7)
    L.init_weights()
    eps = []
    for e in range(12):      # episodes of 9 states: 8 transitions each
        w, lab = rng.uniform(0.5, 1.5, size=(9, nopt)), rng.integers(0, nopt, size=9)
        w[np.arange(9), lab] = np.where(np.arange(9) % 2 == 1, 0.05, 2.0)
        mu, R = w / w.sum(1, keepdims=True), rng.normal(size=9)
        mu[-1], lab[-1], R[0] = 0.0, 0, 0.0
        eps.append(dict(states=rng.normal(size=(9, 6)).astype(np.float32), labels=lab, mu=mu))
        msg = _message(lab, values); msg[-1] = 0.0
        L.append_episode(eps[e]["states"], msg, mu, R, (0.5 * rng.normal(size=9)).astype(np.float32), 0, e)
    L.initialize(); L.set_tap(True)
    pos = {L.episode_info(k)[0]: k for k in range(12)}
    ret = {g: L.episode_field(k, capi.EP_RETURN) for g, k in pos.items()}
    s, w, lay, (mean, scale, _) = L.scalars(), L.get_params()[0].astype(np.float64), L.layout(), L.get_scaling()
    iW, iB, nD, ld0, ldo = lay["indW"], lay["indB"], 1 + 2 * nopt, (H + 7) // 8 * 8, (2 * nopt + 8) // 8 * 8
    W0, b0 = w[iW[1]:iW[1] + 6 * ld0].reshape(6, ld0)[:, :H], w[iB[1]:iB[1] + H]
    Wo, bo = w[iW[-1]:iW[-1] + H * ldo].reshape(H, ldo)[:, :nD], w[iB[-1]:iB[-1] + nD]

    def net(S):      # (hidden outputs, network outputs) of raw states
        y = np.tanh(((S.astype(np.float64) - mean) * scale) @ W0 + b0)
        return y, (np.tanh(y @ Wo + bo) if out == "Tanh" else y @ Wo + bo)
    L.step(1, flat=np.array([7, 15, 16, 25, 34, 43, 52, 61]))
    O, Gd = L.readback(capi.TAP_OUTPUT), L.readback(capi.TAP_OUTGRAD)
    rho, dkl, far, tags, ts = [L.readback(t) for t in (capi.TAP_RHO, capi.TAP_DKL, capi.TAP_FAR, capi.TAP_TAG, capi.TAP_TSTEP)]
    y, Oref = net(np.stack([eps[int(g)]["states"][int(t)] for g, t in zip(tags, ts)]))
    assert relinf(O, Oref) < TOL32      # every column tile of the output layer
    fars, worst64, nNext = set(), 0.0, 0
    for b in range(8):
        ep, t = eps[int(tags[b])], int(ts[b])
        r, d, f, g, margin, klmag = _head_reference(O[b], int(ep["labels"][t]), ep["mu"][t], float(ret[int(tags[b])][t]), s.beta, s.CmaxRet, s.CinvRet)
        fars.add(f)
        worst64 = max(worst64, abs(rho[b] - r) / abs(r), abs(dkl[b] - d) / klmag)
        assert abs(rho[b] - r) <= 64 * U * abs(r) and abs(dkl[b] - d) <= 64 * U * klmag, (b, rho[b], r, dkl[b], d)
        assert bool(far[b]) == f, (b, rho[b], r)
        half = 0.5 * np.spacing(np.abs(g).astype(np.float32)).astype(np.float64)      # of the reference rounded to float
        assert np.all(np.abs(Gd[b] - g) - half <= margin), (b, float((np.abs(Gd[b] - g) - half - margin).max()))
        if t == 7:      # the truncated end's V(s_{t+1}), written into the replay by the next-state row
            Vn, nNext = _net2v(net(ep["states"][8:9])[1][0, 0]), nNext + 1
            assert abs(L.episode_field(pos[int(tags[b])], capi.EP_VALUE)[8] - Vn) <= TOL32 * max(abs(Vn), 1.0)
    print("options %d: RHO / DKL worst fp64 deviation %.3g (bound %.3g)" % (nopt, worst64, 64 * U))
    assert fars == {True, False} and nNext == 2      # both branches and the next-state rows ran
    # the deltas of every column reach the backward launches (the output layer's bias gradient: their column sums) and, through Wo and
    # f'(y), the last hidden block (its bias gradient)
    dl, gs = (Gd * (1 - O * O) if out == "Tanh" else Gd), L.readback(capi.TAP_GRADSUM).astype(np.float64)
    assert np.all(np.abs(gs[iB[-1]:iB[-1] + nD] - dl.sum(0)) <= 8 * 2.0 ** -24 * np.abs(dl).sum(0) + 1e-30)      # eight fp32 additions per column
    assert relinf(gs[iB[1]:iB[1] + H], ((dl @ Wo.T) * (1 - y * y)).sum(0)) < TOL32


# ---- 4. acting -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_acting_writes_one_entry_per_variable(hip_api):
    import torch
    values, nopt, n = (10, 13), 130, 37
    L = capi.create_discrete(hip_api, values, dimS=6, bounded=[0, 0], hidden=(32,), nnFunc="Tanh", batchSize=8, maxTotObsNum=4000, randSeed=7)
    L.init_weights()
    rng = np.random.default_rng(3)
    S = torch.from_numpy(rng.normal(size=(n, 6)).astype(np.float32)).cuda()
    u = rng.uniform(size=n)
    O = L.forward_dev(S).cpu().numpy()
    act, mu, _, _ = [t.cpu().numpy() for t in L.select_actions_dev(S, torch.from_numpy(u).cuda())]
    refs = [head_np(O[i], u[i], 1, n_options=nopt) for i in range(n)]
    labels = [int(np.floor(r[0][0])) for r in refs]
    assert np.array_equal(act, _message(labels, values)) and max(labels) >= 64      # (options of the second tile were drawn)
    assert all(np.all(np.abs(mu[i] - refs[i][1]) <= 1e-12 * refs[i][1]) for i in range(n))
    # a rollout of a few calls: the stored actions decode to the labels their uniforms imply on the stored probabilities
    roll = L.rollout(4, 8, seed=1)
    for call in range(3):
        s = torch.from_numpy(rng.normal(size=(4, 6)).astype(np.float32)).cuda()
        uu = rng.uniform(size=4)
        roll.step(s, torch.zeros(4, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"),
                  noise=torch.from_numpy(uu).cuda(), store=False)
        for e in range(4):
            k, _, A, MU, _, _, _ = roll.read(e)
            assert k == call + 1
            label = min(int(np.searchsorted(np.cumsum(MU[call]), uu[e], side="right")), nopt - 1)
            assert np.array_equal(A[call], _message([label], values)[0]), (call, e, A[call], label)
