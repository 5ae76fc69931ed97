"""What the GPU acting tests (tests/test_hip_act_*.py) share: the net tables, learner and pair builders, row and window generators, the
layouts of windows in device memory, the numpy restatement of RACER::selectAction's heads, the comparisons of training state and replay.
A plain module beside parity.py and blocks.py: no fixtures."""
import numpy as np

from oracle_api import oracle_learner, fill_synth, synth_cfg
from parity import relinf
from smarties_amd import capi

TOL32 = 1e-5     # the bound the acting tests hold hl_forward, hl_forward_sequence and the training outputs to against the oracle
N_AGENTS = 37
CLIP = 8.31776613503286      # SquashedNormalPolicy::sample (Continuous_policy.h:356-360)


# ---- the checker of the heads: smarties_amd/host/vracer_hip.h:209-258 in numpy fp64, one agent per call (pinned against values worked
# out by hand in tests/test_act_dev_cpu.py) ----------------------------------------------------------------------------------------------
def _softplus(x):
    return (x + np.sqrt(1 + x * x)) / 2


def _net2v(x):      # Learners/RACER_common.cpp:23-27
    return 100 * (x + 51) - 100 * np.sqrt(2601 + 100 * x) if x > 0 else 100 * (x - 51) + 100 * np.sqrt(2601 - 100 * x)


def _clip(v):
    return CLIP if v > CLIP else (-CLIP if v < -CLIP else v)


def _store(V, A):
    """(values, advantages) as MB.appendValues keeps them: (Fval)V, (Fval)((Fval)(V + A) - (Fval)V)"""
    return np.float32(V), np.float32(np.float32(V + A) - np.float32(V))


def head_np(out, noise, dA, bounded=(), gaussian=False, n_options=0):
    """One agent: network outputs (float64) -> (action [dA], mu [polDim], value f32, advantage f32).  noise None: the evaluation action."""
    out = np.asarray(out, np.float64)
    V = _net2v(out[0])
    if n_options:
        probs = np.array([_softplus(out[1 + n_options + j]) for j in range(n_options)])
        norm = 0.0
        for p in probs:
            norm += p
        probs = probs / max(norm, np.finfo(np.float64).eps)
        if noise is None:
            label = int(np.argmax(probs))
        else:
            cdf, label = 0.0, n_options - 1
            for j in range(n_options):
                cdf += probs[j]
                if cdf > float(noise):
                    label = j
                    break
        expA = 0.0
        for j in range(n_options):
            expA += probs[j] * out[1 + j]
        v, a = _store(V, out[1 + label] - expA)
        return np.array([label + 0.1]), probs, v, a
    nAdv = 1 + 2 * dA if gaussian else 0
    nDense = 1 + nAdv + dA
    mean = out[1 + nAdv:1 + nAdv + dA].copy()
    stdev = np.array([_softplus(out[nDense + i]) for i in range(dA)])
    act = mean.copy()
    if noise is not None:
        for i in range(dA):
            a = mean[i] + stdev[i] * noise[i]
            act[i] = _clip(a) if (i < len(bounded) and bounded[i]) else a
    A = 0.0
    if gaussian:
        quad, ratio = 0.0, 1.0
        for i in range(dA):
            m = _clip(mean[i]) if (i < len(bounded) and bounded[i]) else mean[i]
            p1, p2, Sv = _softplus(out[2 + i]), _softplus(out[2 + dA + i]), stdev[i] * stdev[i]
            quad += (act[i] - m) * (act[i] - m) / (p1 if act[i] > m else p2)
            ratio *= np.sqrt(p1 / (p1 + Sv)) / 2 + np.sqrt(p2 / (p2 + Sv)) / 2
        A = _softplus(out[1]) * (np.exp(-quad / 2) - ratio)
    v, a = _store(V, A)
    return act, np.concatenate([mean, stdev]), v, a


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _check_heads(kw, O, noise, got):
    """device results against head_np, agent by agent: f64 outputs within 1e-12 relative, f32 within one float ulp of the larger operand"""
    act, mu, val, adv = [t.cpu().numpy() for t in got]
    gauss, nOpt = kw.get("adv_kind") == capi.ADV_GAUSSIAN, kw.get("n_options", 0)
    for i in range(N_AGENTS):
        ra, rm, rv, radv = head_np(O[i], None if noise is None else noise[i], kw["dimA"], kw["bounded"], gauss, nOpt)
        if nOpt:
            assert act[i, 0] == ra[0], (i, act[i], ra)       # the label is exact by construction
        assert np.all(np.abs(act[i] - ra) <= 1e-12 * np.abs(ra)), (i, act[i], ra)
        assert np.all(np.abs(mu[i] - rm) <= 1e-12 * np.abs(rm)), (i, mu[i], rm)
        V = float(rv)
        assert abs(float(val[i]) - V) <= _ulp32(V), (i, val[i], rv)
        # advantage = (Fval)((Fval)(V + A) - (Fval)V): the larger operand is V + A or V
        big = max(abs(V), abs(V + float(radv)))
        assert abs(float(adv[i]) - float(radv)) <= _ulp32(big), (i, adv[i], radv, V)


# ---- the nets -------------------------------------------------------------------------------------------------------------------------
DENSE_BASE = dict(dimS=6, dimA=2, bounded=[1, 0], hidden=(32, 32), nnFunc="Tanh", batchSize=8, maxTotObsNum=4000, randSeed=5)
# dense nets beyond the one-kernel route's 1024 columns (tests/test_hip_act_rows.py)
ROWS_WIDE = {
    "h1040": dict(dimS=9, dimA=3, bounded=[1, 0, 0], hidden=(1040,), nnFunc="Tanh", batchSize=8, maxTotObsNum=2000, randSeed=17),
    "in1030": dict(dimS=1030, dimA=2, bounded=[1, 0], hidden=(32,), nnFunc="Tanh", batchSize=8, maxTotObsNum=2000, randSeed=17),
}

CONV_ATARI = [(84, 84, 4, 8, 8, 4), (20, 20, 8, 16, 6, 2), (8, 8, 16, 32, 4, 1), (5, 5, 32, 64, 3, 1)]      # RACER_atari.json
_BASE = dict(dimA=2, bounded=[1, 0], batchSize=8, maxTotObsNum=1500, randSeed=5)
NETS = {
    # 8 channels (half a channel tile), stride 2
    "strided": dict(_BASE, dimS=576, conv=[(12, 12, 4, 8, 3, 1), (10, 10, 8, 16, 4, 2)], hidden=(32,), nnFunc="Tanh"),
    # non-square image, 5 channels, K = 27 (no multiple of 4), 35 positions
    "odd": dict(_BASE, dimS=189, conv=[(9, 7, 3, 5, 3, 1)], hidden=(32, 24), nnFunc="SoftSign"),
    # stMean[c % dS] over stacked frames
    "app3": dict(_BASE, dimS=200, nAppendedObs=3, conv=[(10, 10, 8, 16, 6, 2)], hidden=(40,)),
    # 6 extras, a row that is no multiple of 4 floats
    "extras6": dict(_BASE, dimS=1030, dimA=1, bounded=[0], adv_kind=capi.ADV_DISCRETE, n_options=5,
                    conv=[(8, 8, 16, 32, 4, 1), (5, 5, 32, 64, 3, 1)], hidden=(48,)),
    # one extra per frame, feature rows 1028 wide
    "app3-extra": dict(_BASE, dimS=801, nAppendedObs=3, conv=[(20, 20, 8, 16, 6, 2)], hidden=(40, 24)),
    # more extras (40) than the first dense layer is wide: its residual reads extras only
    "extras40": dict(_BASE, dimS=229, conv=[(9, 7, 3, 5, 3, 1)], hidden=(32, 32), nnFunc="SoftSign"),
    "atari": dict(dimS=7056, dimA=1, bounded=[0], adv_kind=capi.ADV_DISCRETE, n_options=6, nAppendedObs=3, conv=CONV_ATARI, hidden=(64,),
                  nnFunc="SoftSign", batchSize=8, maxTotObsNum=400, randSeed=11),
}
N_EPS = {"atari": 14}
# nets whose output columns the fp32 restatement itself does not resolve to TOL32 / 3 against its build in double (measured on the CPU after
# the three steps of the row-by-row test, 17 rows: 6 of the 13 columns of "atari" between 3.5e-6 and 3.6e-5 -- outputs of 7e-4 .. 5e-2 behind
# the 3136-term sums of its dense layer): parity.assert_columns holds those columns to 4 x the restatement's own loss
ILL_COLUMNS = ("atari",)
LDS_NETS = {
    # 176 KB of image (rows beyond HL_ACT_CONV_MAX_ROW_BYTES as well: the switch is held open, so the plan is what refuses)
    "image-176K": dict(_BASE, dimS=44100, conv=[(210, 210, 1, 2, 10, 8)], hidden=(32,), maxTotObsNum=300),
    # rows of 5.6 KB, within the switch as shipped: the first map, 32 x 36 x 36 floats = 162 KB, is what exceeds the LDS
    "map-162K": dict(_BASE, dimS=1444, conv=[(38, 38, 1, 32, 3, 1), (36, 36, 32, 2, 4, 4)], hidden=(32,), maxTotObsNum=300),
}
PARITY = ["strided", "odd", "app3", "app3-extra", "extras6", "atari"]      # the conv nets the device window calls are held to the host call on

NATURE = [(84, 84, 4, 32, 8, 4), (20, 20, 32, 64, 4, 2), (9, 9, 64, 64, 3, 1)]      # Network/Builder.cpp:189-194
# the nets beyond the resident plans (tests/test_hip_act_band_dev.py):
# name -> (configuration, row counts, window lengths, band launches per call, the dense layers run panelled, cpu_bar of assert_columns)
BAND_NETS = {
    # two bands of 10 output rows (44 input rows x 84 x 4 channels), a feature row of 3136 in panels of 1024 and one of 64
    "nature": (dict(dimS=7056, dimA=1, bounded=[0], adv_kind=capi.ADV_DISCRETE, n_options=6, nAppendedObs=3, conv=NATURE, hidden=(512,),
                    nnFunc="Tanh", batchSize=8, maxTotObsNum=400, randSeed=11), (1, 17), (1, 2, 3, 4, 9), 1, True, True),
    # ONE conv layer: every band's part of the map goes straight behind the (zero) extras of the feature vector
    "image-176K": (LDS_NETS["image-176K"], (1, 17, 300), (1, 2), 1, False, False),
    # 5 extras, a row that is no multiple of 4 floats, a feature row of 2357, the residual of 48 columns over a panelled input
    "feat-2357": (dict(_BASE, dimS=517, conv=[(16, 16, 2, 12, 3, 1)], hidden=(48, 24), nnFunc="SoftSign"), (1, 17, 300), (1, 2, 9), 0, True, False),
    "dense-2500": (dict(_BASE, dimS=2500, hidden=(48, 24)), (1, 17, 300), None, 0, True, False),
    # a stacked row of 3090 through act_stack_dev_kernel
    "dense-1030x3": (dict(_BASE, dimS=1030, nAppendedObs=2, hidden=(64,)), (1, 17, 300), (1, 2, 3, 9), 0, True, True),
}

CONV = [(8, 8, 16, 32, 4, 1), (5, 5, 32, 64, 3, 1)]
# shapes hl_forward_sequences serves beside the batched window kernel: name -> (configuration, synthetic episodes)
FALLBACK = {
    "conv-lstm": (dict(dimS=256, dimA=1, adv_kind=capi.ADV_DISCRETE, n_options=4, nAppendedObs=3, conv=CONV, hidden=(32,), nnFunc="Tanh",
                       batchSize=16, maxTotObsNum=2000, randSeed=3, nn_type=capi.NN_LSTM, nnBPTTseq=4),
                  dict(seed=5, dimS=256, dimA=1, lenMin=10, lenMax=40, pTerm=0.5)),
    "rnn-encoder-mgu": (dict(dimS=5, dimA=2, bounded=[1, 0], hidden=(16, 16), encoder=[24], encoder_rnn=1, nn_type=capi.NN_MGU, nnFunc="Tanh",
                             batchSize=16, maxTotObsNum=2000, randSeed=5, adv_kind=capi.ADV_GAUSSIAN, nnBPTTseq=5),
                        dict(seed=21, dimS=5, dimA=2, lenMin=5, lenMax=40, pTerm=0.5)),
    "lstm-512": (dict(dimS=7, dimA=2, bounded=[1, 0], hidden=(512,), nnFunc="Tanh", batchSize=6, maxTotObsNum=8000, randSeed=5,
                      nn_type=capi.NN_LSTM, adv_kind=capi.ADV_GAUSSIAN, nnBPTTseq=3),
                 dict(seed=21, dimS=7, dimA=2, lenMin=2, lenMax=30, pTerm=0.5)),
    "dense-app3": (dict(dimS=9, dimA=3, bounded=[0, 0, 0], hidden=(24, 16, 8), nnFunc="Tanh", batchSize=8, maxTotObsNum=1000, randSeed=5,
                        nAppendedObs=3),
                   dict(seed=3, dimS=9, dimA=3, lenMin=5, lenMax=30, pTerm=0.3)),
}

KINDS = {"lstm": capi.NN_LSTM, "mgu": capi.NN_MGU, "rnn": capi.NN_RNN}
WIDE_SHAPES = [  # recurrent nets on wide inputs: (layer type, hidden, dimS, nAppendedObs, bptt, batch)
    ("lstm", (32, 16), 257, 0, 3, 6),       # one component above the old bound; dimS % 4 != 0: scalar loads; a chunk below a 16-row tile
    ("mgu", (64, 32), 300, 4, 4, 20),       # context states, windows that begin before the episode's start, both MGU phases, a partial second row block, 16-byte loads
    ("rnn", (272,), 1027, 0, 3, 6),         # an odd reduction length, 17 cell tiles
    ("lstm", (512,), 260, 0, 2, 8),         # wide inputs and a layer beyond 256 cells together
    ("lstm", (16,), 8192, 0, 2, 4),         # the upper bound
]
WIDE_IDS = ["%s-%s-dS%d-app%d" % (sh[0], "x".join(map(str, sh[1])), sh[2], sh[3]) for sh in WIDE_SHAPES]


def _wide_cfg(shape, **over):
    kind, hidden, dS, nApp, bptt, batch = shape
    kw = dict(dimS=dS, dimA=2, bounded=[1, 0], hidden=hidden, nnFunc="Tanh", batchSize=batch, maxTotObsNum=8000, randSeed=5,
              nn_type=KINDS[kind], adv_kind=capi.ADV_GAUSSIAN, nnBPTTseq=bptt, nAppendedObs=nApp)
    kw.update(over)
    return kw


def _rec_cfg(kind, hidden, nApp=0, bptt=8):
    return dict(dimS=6, dimA=2, bounded=[1, 0], hidden=hidden, nnFunc="Tanh", batchSize=16, maxTotObsNum=5000, randSeed=51,
                adv_kind=capi.ADV_GAUSSIAN, nn_type=kind, nnBPTTseq=bptt, nAppendedObs=nApp)


# ---- learners and pairs ---------------------------------------------------------------------------------------------------------------
def _pair(hip_api, cfg_kw, sc, n_eps, given=False):
    """(library learner, CPU oracle) on the same synthetic episodes.  given: both start from the same given weights instead of
    hl_init_weights -- which refuses a Tanh output layer under the Gaussian advantage, whose initial outputs of -1 / +1 have no finite
    pre-image (test_output_functions_without_a_finite_start_are_refused)"""
    G = capi.Learner(hip_api, capi.make_config(**cfg_kw))
    O = oracle_learner(capi.make_config(**cfg_kw))
    w = None
    for L in (G, O):
        if given:
            if w is None:
                w = np.random.default_rng(1).uniform(-0.1, 0.1, L.get_params()[0].shape).astype(np.float32)
            L.set_params(w, np.zeros_like(w), np.zeros_like(w))
        else:
            L.init_weights()
        fill_synth(L, sc, n_eps)
        L.initialize()
        L.set_tap(True)
    return G, O


def _conv_sc(kw, **over):
    d = dict(seed=21, dimS=kw["dimS"], dimA=kw["dimA"], lenMin=4, lenMax=12, pTerm=0.5)
    d.update(over)
    return synth_cfg(**d)


def _conv_pair(hip_api, name, oracle=True, weights=None):
    """the pair of a net of NETS by name (or of a configuration given as it is); oracle=False: the library learner alone"""
    kw = NETS[name] if isinstance(name, str) else name
    Ls = [capi.Learner(hip_api, capi.make_config(**kw))] + ([oracle_learner(capi.make_config(**kw))] if oracle else [])
    for L in Ls:
        if weights is None:
            L.init_weights()
        else:
            w = weights(L)
            L.set_params(w, np.zeros_like(w), np.zeros_like(w))
        fill_synth(L, _conv_sc(kw), N_EPS.get(name, 30) if isinstance(name, str) else 30)
        L.initialize()
        L.set_tap(True)
    return Ls if oracle else Ls[0]


def _synth_learner(hip_api, kw, sc_kw, n_eps=40):
    L = capi.Learner(hip_api, capi.make_config(**kw))
    L.init_weights()
    if n_eps:
        fill_synth(L, synth_cfg(**sc_kw), n_eps)
        L.initialize()
    return L


def _bare(hip_api, kw):
    L = capi.Learner(hip_api, capi.make_config(**kw))
    L.init_weights()
    return L


def _compare_step(G, O):
    assert np.array_equal(G.readback(capi.TAP_FLAT), O.readback(capi.TAP_FLAT))
    assert np.array_equal(G.readback(capi.TAP_TAG), O.readback(capi.TAP_TAG))
    assert np.array_equal(G.readback(capi.TAP_TSTEP), O.readback(capi.TAP_TSTEP))
    assert np.array_equal(G.readback(capi.TAP_STATE), O.readback(capi.TAP_STATE))
    assert relinf(G.readback(capi.TAP_OUTPUT), O.readback(capi.TAP_OUTPUT)) < TOL32
    assert relinf(G.readback(capi.TAP_RHO), O.readback(capi.TAP_RHO)) < TOL32
    assert relinf(G.readback(capi.TAP_DKL), O.readback(capi.TAP_DKL)) < TOL32
    assert relinf(G.readback(capi.TAP_OUTGRAD), O.readback(capi.TAP_OUTGRAD)) < TOL32
    assert np.array_equal(G.readback(capi.TAP_FAR), O.readback(capi.TAP_FAR))
    assert relinf(G.readback(capi.TAP_GRADSUM), O.readback(capi.TAP_GRADSUM)) < TOL32


def _same_training_state(A, B):
    for a, b in zip(A.get_params(), B.get_params()):      # weights and both moments
        assert np.array_equal(a, b)
    assert np.array_equal(A.get_rng_state(), B.get_rng_state())
    assert A.scalars().beta == B.scalars().beta


def _same_replay(A, B):
    assert A.counts() == B.counts()
    for pos in range(A.counts()[1]):
        assert A.episode_info(pos) == B.episode_info(pos), pos
        assert np.array_equal(A.episode_stats(pos), B.episode_stats(pos)), pos
        for field in range(6):
            assert np.array_equal(A.episode_field(pos, field), B.episode_field(pos, field)), (pos, field)
        # states, actions, policies and rewards as stored (bytes: the wire format's trailer holds integers that read as NaN)
        assert A.pack_episode(pos).tobytes() == B.pack_episode(pos).tobytes(), pos


# ---- rows, windows and their layouts in device memory -----------------------------------------------------------------------------------
def _rows(rng, n, dIn):
    return (rng.normal(size=(n, dIn)) * 1.5 + 0.2).astype(np.float32)


def _ragged(rng, n, dS, lengths):
    """n windows whose lengths go round `lengths` (so that the first few cover all of them)"""
    return [(rng.normal(size=(lengths[i % len(lengths)], dS)) * 1.5 + 0.2).astype(np.float32) for i in range(n)]


def _stacked(wins, nApp):
    """the rows hl_forward reads: the last state, then the ones before it, steps before the first given state repeating it"""
    return np.stack([np.concatenate([w[max(len(w) - 1 - j, 0)] for j in range(1 + nApp)]) for w in wins])


def _row_bytes(kw):
    return 4 * kw["dimS"] * (1 + kw.get("nAppendedObs", 0))


def _count(G, name):
    return G.timing_get(name)[1]


def _training_forwards(G):
    """launches of the training forward path: the first conv layer and whichever name the dense layers behind run under"""
    return _count(G, "conv_fwd0"), _count(G, "fwd_chain") + sum(_count(G, "gemm16_fwd%d" % j) for j in range(8))


_SIDE = []


def _side_stream():
    """ONE side stream for the whole process: every stream torch hands out and that is used keeps a hardware queue of the process for
    good, and the tests of several replicas in one process (test_hip_parity.py, test_hip_r6.py) need a queue per replica"""
    import torch
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream())
    return _SIDE[0]


def _packed(wins):
    """the windows back to back: (states [rows][dS], first_row, n_steps, row_stride 1)"""
    n_steps = np.array([w.shape[0] for w in wins], np.int32)
    first = np.concatenate([[0], np.cumsum(n_steps[:-1])]).astype(np.int64)
    return np.concatenate(wins, axis=0), first, n_steps, 1


def _columns(wins):
    """the windows as columns of a [T][nEnv] rollout buffer, agent e in column e from row e % 3 on; cells no window owns hold NaN, so a
    row read from the wrong place shows in the outputs: (states [T nEnv][dS], first_row, n_steps, row_stride nEnv)"""
    n_env, dS = len(wins), wins[0].shape[1]
    T = max(w.shape[0] for w in wins) + 2
    buf = np.full((T, n_env, dS), np.nan, np.float32)
    for e, w in enumerate(wins):
        buf[e % 3:e % 3 + w.shape[0], e] = w
    first = np.array([(e % 3) * n_env + e for e in range(n_env)], np.int64)
    return buf.reshape(T * n_env, dS), first, np.array([w.shape[0] for w in wins], np.int32), n_env


def _call_dev(G, side, layout, order, select=None):
    """the device call on agents `order` of a layout, the buffer written on the side stream right before it and the outputs read in that
    stream's order, no other synchronisation"""
    import torch
    states, first, n_steps, stride = layout
    with torch.cuda.stream(side):
        tables = (torch.from_numpy(first[order]).to("cuda", non_blocking=True), torch.from_numpy(n_steps[order]).to("cuda", non_blocking=True))
        half = torch.from_numpy(states * np.float32(0.5)).to("cuda", non_blocking=True)
        st = half + half
        if select is None:
            return G.forward_sequences_dev(st, tables[0], tables[1], stride, stream=side).cpu().numpy()
        return [t.cpu().numpy() for t in G.select_actions_sequences_dev(st, tables[0], tables[1], stride, select, stream=side)]


def _window_args(L, n=3):
    import torch
    return (torch.zeros((n + 1, L.dS), dtype=torch.float32, device="cuda"), torch.arange(n, dtype=torch.int64, device="cuda"),
            torch.ones(n, dtype=torch.int32, device="cuda"))
