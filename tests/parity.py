"""Shared parity machinery: drive a learner (HIP library or CPU oracle -- same C-ABI) through a
golden fixture recorded from the compiled reference and report the deviations."""
import os

import numpy as np

from golden_io import load_blob
from oracle_api import fill_synth, synth_cfg
from smarties_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture(name):
    return load_blob(os.path.join(GOLDEN, name))


def fixture_config(fx, **over):
    dS, dA, B = [int(x) for x in fx["cfg"][:3]]
    hp = fx["hp"]
    func = over.pop("nnFunc", None)
    adv = int(fx["cfg"][11]) if len(fx["cfg"]) > 11 else 0     # 0 = VRACER, 1 = RACER with the Gaussian advantage
    nopt = int(fx["cfg"][12]) if len(fx["cfg"]) > 12 else 0    # discrete head: options of the action variable
    nnt = int(fx["cfg"][13]) if len(fx["cfg"]) > 13 else 0     # hidden layer type: 0 dense, 1 LSTM
    bptt = int(fx["cfg"][14]) if len(fx["cfg"]) > 14 else 0
    kw = dict(adv_kind=adv, n_options=nopt, nn_type=nnt, nnBPTTseq=bptt, dimS=dS, dimA=dA, bounded=fx["bounded"], hidden=[int(x) for x in fx["layers"]], batchSize=B,
              maxTotObsNum=int(hp[12]), clipImpWeight=hp[0], penalTol=hp[1], epsAnneal=hp[2], gamma=hp[3],
              lambda_=hp[4], learnrate=hp[5], explNoise=hp[6], outWeightsPrefac=hp[7], nnLambda=hp[8],
              randSeed=42, nnFunc=func or "SoftSign")
    if "preproc" in fx:      # appended observations and convolutional layers (W, H, C, K, F, S per layer) of the MDP
        pre = [int(x) for x in fx["preproc"]]
        kw["nAppendedObs"] = pre[0]
        kw["conv"] = [tuple(pre[1 + 6 * i:7 + 6 * i]) for i in range((len(pre) - 1) // 6)]
    if "sampling" in fx:
        kw["dataSamplingAlgo"] = int(fx["sampling"][0])
    if "erFilter" in fx:
        kw["ERoldSeqFilter"] = int(fx["erFilter"][0])
    if "minObs" in fx:           # (matters once episodes arrive during training: time stamps count from this many observations)
        kw["minTotObsNum"] = int(fx["minObs"][0])
    if "threads" in fx:          # OpenMP threads of the reference run that recorded the fixture
        kw["ref_threads"] = int(fx["threads"][0])
    if "retEst" in fx:           # settings keys returnsEstimator, nnOutputFunc, encoderLayerSizes of the recording run
        kw["returnsEstimator"] = int(fx["retEst"][0])
        kw["nnOutputFunc"] = int(fx["outFunc"][0])
        kw["encoder"] = [int(x) for x in fx["encoder"]]
    if "pomdp" in fx and nnt == 0:   # a partially observable MDP with nnType left non-recurrent: RNN encoder layers under MGU layers (Approximator.cpp:221-223, 264-270)
        kw["nn_type"] = capi.NN_MGU
        kw["encoder_rnn"] = 1
    kw.update(over)
    return capi.make_config(**kw)


def fixture_arrival(fx, k):
    """Tag of the synthetic episode the recording run appended behind gradient step k (ref_driver addEvery=n), or None."""
    n = int(fx["addEvery"][0]) if "addEvery" in fx else 0
    return int(fx["cfg"][3]) + k // n - 1 if n > 0 and k % n == 0 else None


def fixture_synth(fx):
    dS, dA = int(fx["cfg"][0]), int(fx["cfg"][1])
    hp = fx["hp"]
    return synth_cfg(seed=int(fx["cfg"][8]), dimS=dS, dimA=dA, lenMin=int(fx["cfg"][9]), lenMax=int(fx["cfg"][10]),
                     pTerm=hp[9], muSpread=hp[10], actNoise=hp[11])


def relinf(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def fx_vec_dev(fx, key, mine):
    """Deviation of a parameter-sized vector from the fixture's: the whole vector, or -- "lean" fixtures of large
    networks (oracle/ref_driver.cpp: writeParams) -- every 53rd element plus the sum and the sum of squares."""
    m = np.asarray(mine, np.float64)
    if key in fx:
        return relinf(m, fx[key])
    sub, (s1, s2, n) = np.asarray(fx[key + "_sub"], np.float64), fx[key + "_sums"]
    assert int(n) == m.size, (key, n, m.size)
    scale = max(np.abs(m).max(), 1e-300)
    d = np.abs(m[::53] - sub).max() / scale
    d = max(d, abs(m.sum() - s1) / max(np.abs(m).sum(), 1e-300), abs((m * m).sum() - s2) / max(2 * s2, 1e-300))
    return float(d)


def _f32_to_u64_x86(x):
    """float -> unsigned long as gcc compiles it for x86-64 (cvttss2si; out of range: the 'integer indefinite' value)"""
    cvtt = lambda v: int(v) if -2.0 ** 63 <= v < 2.0 ** 63 else -2 ** 63
    if x < 2.0 ** 63:
        return cvtt(x) % 2 ** 64
    return (cvtt(np.float32(x - np.float32(2.0 ** 63))) % 2 ** 64) ^ 2 ** 63


def _fma_f32(a, b, c):
    """a * b + c rounded once to float32 (the reference's statement compiles to vfmadd in the build the fixtures come from)"""
    from fractions import Fraction
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    f = np.float32(float(x))
    best = f
    for g in (np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))):
        if not np.isfinite(g):
            continue
        dg, db = abs(Fraction(float(g)) - x), abs(Fraction(float(best)) - x)
        if dg < db or (dg == db and (int(np.float32(g).view(np.uint32)) & 1) == 0):
            best = g
    return np.float32(best)


def far_count_loop(L, tags_in_order):
    """ReplayStats::nFarPolicySteps as MemoryProcessing.cpp:202-238 accumulates it -- `Uint += float * float` per episode, in the
    given storage order -- over the fractions learner L holds."""
    rec = {}
    for p in range(L.scalars().nStoredEps):
        tag, N, _ = L.episode_info(p)
        rec[tag] = (np.float32(N), np.float32(L.episode_stats(p)[2]))
    n = 0
    for tag in tags_in_order:
        N, f = rec[int(tag)]
        n = _f32_to_u64_x86(_fma_f32(N, f, np.float32(n)))
    if L.scalars().CmaxRet <= 1:
        n = 0
    return n - 2 ** 64 if n >= 2 ** 63 else n


def storage_order(L):
    return [L.episode_info(p)[0] for p in range(L.scalars().nStoredEps)]


def flat_for(L, tags, ts):
    """flat indices (in the learner's own episode order) selecting the given (tag, t) pairs"""
    n = L.scalars().nStoredEps
    prefix, acc = {}, 0
    for k in range(n):
        tag, N, _ = L.episode_info(k)
        prefix[tag] = acc
        acc += N - 1
    return np.array([prefix[int(g)] + int(t) for g, t in zip(tags, ts)], np.int64)


def setup_from_fixture(L, fx, use_fixture_weights=False):
    """create -> init weights -> fill synthetic replay -> initializeLearner."""
    nEps = int(fx["cfg"][3])
    if use_fixture_weights:
        L.set_params(w=fx["W0"])
        L.set_rng_state(fx["rng_before_init"])
    else:
        L.init_weights()
    fill_synth(L, fixture_synth(fx), nEps)
    L.initialize()


def tags_of(L):
    n = L.scalars().nStoredEps
    return np.array([L.episode_info(k)[0] for k in range(n)], np.int64)


def episode_arrays_by_tag(L, field):
    out = {}
    for k in range(L.scalars().nStoredEps):
        out[L.episode_info(k)[0]] = L.episode_field(k, field)
    return out


def fixture_arrays_by_tag(fx, tags_key, arr_key, lens):
    out, o = {}, 0
    for tag in fx[tags_key]:
        n = lens[int(tag)]
        out[int(tag)] = fx[arr_key][o:o + n]
        o += n
    return out

import pytest  # noqa: E402

def check_packed_roundtrip(make_learner, fx):
    """Episodes in the reference's wire format (Episode::packEpisode, Episode.cpp:24-86), as packed by the
    compiled reference right after Learner::initializeLearner."""
    from oracle_api import synth_episode
    cfg = fixture_config(fx)
    sc = fixture_synth(fx)
    nopt = int(fx["cfg"][12]) if len(fx["cfg"]) > 12 else 0     # discrete head: policies are n_options probabilities
    tags = [int(t) for t in fx["pack_tags"]]
    packs = [np.asarray(fx["pack_%d" % k], np.float32) for k in range(len(tags))]
    # (1) same learner state as the reference had: the library's own pack == the reference's pack
    L = make_learner(cfg)
    setup_from_fixture(L, fx)                      # pushes the synthetic episodes, initialize
    pos_of = {L.episode_info(p)[0]: p for p in range(int(fx["cfg"][3]))}
    for tag, ref in zip(tags, packs):
        mine = L.pack_episode(pos_of[tag])
        assert mine.size == ref.size
        nfl = ref.size - 10
        assert np.array_equal(mine[:nfl], ref[:nfl]), tag     # states, rewards, actions, policies, RET, ADV, V, dQ, impW, KL
        assert mine[nfl:].view(np.uint8)[0] == ref[nfl:].view(np.uint8)[0]   # bReachedTermState
    # (2) unpack: appending the packed record == appending the original arrays rounded through fp32
    A = make_learner(cfg); A.init_weights()
    Bq = make_learner(cfg); Bq.init_weights()
    for tag, ref in zip(tags, packs):
        A.append_packed_episode(ref)
        ep = synth_episode(sc, tag, nopt)
        ep["actions"] = ep["actions"].astype(np.float32).astype(np.float64)
        ep["mu"] = ep["mu"].astype(np.float32).astype(np.float64)
        ep["rewards"] = ep["rewards"].astype(np.float32).astype(np.float64)
        ep["tag"] = int(np.frombuffer(ref[ref.size - 10:].tobytes()[1:9], np.int64)[0])   # the reference's episode ID
        Bq.append_episode(**ep)
    A.initialize(); Bq.initialize()
    for p in range(len(tags)):
        assert A.episode_info(p) == Bq.episode_info(p)
        assert A.pack_episode(p).tobytes() == Bq.pack_episode(p).tobytes()      # (the trailer bytes read as NaN floats)
    with pytest.raises(Exception):
        A.append_packed_episode(packs[0][:-3])         # wrong size


def real2ss(v, w, bpos):
    """Utilities::real2SS (Utils/SstreamUtilities.h:51-63): ' ' + fixed, width w, precision by magnitude."""
    a = abs(v)
    drop = 7 if a >= 1e4 else 6 if a >= 1e3 else 5 if a >= 1e2 else 4 if a >= 10 else 3
    return " %*.*f" % (w, max(w - drop + bpos, 0), v)


def stats_file_lines(fx):
    """(header, [lines]) of the <learner>_stats.txt the recording run wrote (Learner::processStats, Learner.cpp:158-196):
    "ID #/T   <header>" once, then "<learnID> <step / 1000><columns>" per statistics line."""
    txt = bytes(bytearray(fx["stats_file"])).decode().splitlines()
    head = txt[0][len("ID #/T   "):]
    return head, [l[len("00 00001"):] for l in txt[1:]]


def stats_line(L):
    """The line Learner::logStats writes (MemoryBuffer::getMetrics, MemoryBuffer.cpp:522-548, then
    AdamOptimizer::getMetrics, Optimizer.cpp:216-220), rebuilt from a learner's read-back state (without the dRet column
    of the lines that follow a 1000-step sweep: metrics() of the library and of the oracle print -- and consume -- that)."""
    st, sc = L.stats(), L.scalars()
    rew = L.get_scaling()[2]
    out = real2ss(st.avgReturn, 9, 0) + real2ss(float(rew[0]), 6, 0) + real2ss(float(rew[2]), 6, 1)
    out += real2ss(st.avgKLdivergence, 5, 1)
    if st.minQ < st.maxQ:
        eps = float(np.finfo(np.float32).eps)
        out += real2ss(np.sqrt(max(eps, st.avgSquaredErr)), 6, 1) + real2ss(st.maxAbsError, 6, 1)
        out += real2ss(st.stdevQ, 6, 1) + real2ss(st.avgQ, 6, 0) + real2ss(st.minQ, 6, 0) + real2ss(st.maxQ, 6, 0)
    out += " %5d %7d %7d %8d %7d" % (sc.nStoredEps, sc.nStoredSteps, sc.nSeenEps, sc.nSeenSteps, st.nFarPolicySteps)
    if sc.CmaxRet > 1:
        out += real2ss(sc.beta, 6, 1)
    w = L.get_params()[0].astype(np.longdouble)
    return out + real2ss(float(np.sqrt((w * w).sum())), 7, 1)


def lines_agree(mine, ref, head, rel=0.0):
    """Same layout; each number equal at the printed precision (2 units of the last digit, or rel)."""
    if len(mine) != len(ref):
        return False
    names = head.replace("|", " ").split()
    for name, a, b in zip(names, mine.split(), ref.split()):
        ulp = 10.0 ** -len(b.split(".")[1]) if "." in b else 1.0
        if abs(float(a) - float(b)) > max(2 * ulp, rel * abs(float(b))):
            return False
    return True


# ---- per-block deviations -----------------------------------------------------------------------------------------------
# relinf() takes its scale from the largest element of the whole array: one large block (the first layer's weights, the policy
# columns of a tap) sets the bar for all the others.  The helpers below take the scale per parameter block and per output column.

def _layer_kinds(cfg):
    """(kind, units) per layer in build order, as the port's buildNet lays them out (oracle/port/vracer_port.cpp); kind is one of
    in, conv, join, dense, rnn, lstm, mgu, res, out, sigma"""
    hidden = [int(cfg.encoder[j]) for j in range(cfg.n_encoder) if cfg.encoder[j] > 0]
    nEnc = len(hidden)
    hidden += [int(cfg.hidden[j]) for j in range(cfg.n_hidden)]
    kinds = [("in", 0)] + [("conv", 0)] * cfg.n_conv
    inAll = cfg.dimS * (1 + cfg.nAppendedObs)
    inImg = cfg.conv[0].inpFeatures * cfg.conv[0].inpY * cfg.conv[0].inpX if cfg.n_conv else inAll
    if inAll > inImg:
        kinds += [("in", 0), ("join", 0)]
    nHid = 0
    for hsz in hidden:
        if hsz <= 0:
            continue
        ID = len(kinds)
        kind = {capi.NN_FFNN: "dense", capi.NN_LSTM: "lstm", capi.NN_MGU: "mgu", capi.NN_RNN: "rnn"}[cfg.nn_type]
        if cfg.encoder_rnn and nHid < nEnc:
            kind = "rnn"
        nHid += 1
        kinds.append((kind, hsz))
        if ID != 1:
            kinds.append(("res", hsz))
    kinds.append(("out", 0))
    if cfg.adv_kind != capi.ADV_DISCRETE:
        kinds.append(("sigma", 0))
    return kinds


_GATES = {"lstm": ("cell", "in", "forget", "out"), "mgu": ("forget", "state")}


def param_blocks(L):
    """[(name, start, n)] over the parameter vector of learner L: one entry per non-empty weight block and per non-empty bias block
    of L.layout().  The weights of a recurrent layer are split into input and recurrent weights (rows [0, nIn) and [nIn, nIn + cells)
    of its matrix: forwardNet, packBlob of the port), those of LSTM / MGU layers per gate as well; a gate's weights are a column
    range of every row, so for these entries `start` is the array of their n indices."""
    lay, kinds = L.layout(), _layer_kinds(L.cfg)
    assert len(kinds) == len(lay["nW"]), (kinds, lay)
    out = []
    for i, (kind, units) in enumerate(kinds):
        iW, nW, iB, nB = [int(lay[k][i]) for k in ("indW", "nW", "indB", "nB")]
        name = "L%d.%s" % (i, kind)
        if nW > 0 and kind == "rnn":
            ld = (units + 7) // 8 * 8                      # nOutSimd
            assert nB == units and nW % ld == 0
            nIn = nW // ld - units
            out += [(name + ".Wx", iW, ld * nIn), (name + ".Wr", iW + ld * nIn, ld * units)]
        elif nW > 0 and kind in _GATES:
            g = len(_GATES[kind])
            assert nB == g * units and nW % (g * units) == 0
            nIn = nW // (g * units) - units
            for part, rows in (("Wx", np.arange(nIn)), ("Wr", nIn + np.arange(units))):
                for k, gate in enumerate(_GATES[kind]):
                    idx = (iW + rows[:, None] * (g * units) + k * units + np.arange(units)[None, :]).ravel()
                    if idx.size:
                        out.append(("%s.%s.%s" % (name, part, gate), idx, idx.size))
        elif nW > 0:
            out.append((name + ".W", iW, nW))
        if nB > 0:
            out.append((name + ".B", iB, nB))
    return out


def _dev(a, ref, what):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max() if ref.size else 0.0
    if scale == 0.0:
        assert not np.any(a), "%s: the reference is identically zero, the array is not (max %g)" % (what, np.abs(a).max())
        return "zero"
    return float(np.abs(a - ref).max() / scale)


def blockdev(blocks, a, ref):
    """{name: max|a - ref| / max|ref|} over each block of param_blocks(); "zero" where the reference block is identically zero
    (a must then be identically zero too)"""
    a, ref = np.asarray(a), np.asarray(ref)
    out = {}
    for name, start, n in blocks:
        sl = slice(start, start + n) if np.ndim(start) == 0 else start
        out[name] = _dev(a[sl], ref[sl], name)
    return out


def coldev(a, ref):
    """{"c<j>": max|a - ref| / max|ref|} per column j of a [B, nOut] array (a [B] vector is one column); "zero" as in blockdev"""
    a, ref = np.asarray(a), np.asarray(ref)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    a, ref = a.reshape(a.shape[0], -1), ref.reshape(ref.shape[0], -1)
    return {"c%d" % j: _dev(a[:, j], ref[:, j], "column %d" % j) for j in range(a.shape[1])}


def worst_dev(devs):
    """(deviation, name) of the largest numeric entry of a {name: deviation} dict"""
    num = [(v, k) for k, v in devs.items() if v != "zero"]
    return max(num) if num else (0.0, "-")


def twin64(L):
    """The restatement with its arrays in double (oracle/liboracle_port64.so) holding learner L's weights and state scaling: the
    reference of the acting calls (forward, forward_sequence), which read nothing else."""
    from oracle_api import oracle64_learner
    T = oracle64_learner(L.cfg)
    T.set_params(*L.get_params())
    T.set_scaling(*L.get_scaling())
    return T


def assert_columns(got, ref, tol, what=None, ref32=None, cpu_bar=False):
    """Every output column of a batch on its own scale: max|got - ref| / max|ref| over the rows below tol.  The row-wise checks of
    the acting tests take the scale from a row's largest output, which hides its value and advantage columns.  ref32 (the fp32
    restatement's rows), where given, is printed beside the worst column.
    cpu_bar: for a net whose columns are ill-conditioned -- outputs of 1e-3 behind sums of thousands of terms, where the fp32
    restatement itself loses more than tol / 3 against ref -- the bar of such a column is 4 x what the fp32 restatement loses
    in it, taken here from ref32 (the rule of tests/blocks.py for ill-conditioned blocks); every other column keeps tol."""
    d = coldev(got, ref)
    w, c = worst_dev(d)
    e_cpu = None if ref32 is None else coldev(ref32, ref)
    cpu = "" if e_cpu is None else ", fp32 restatement there %s" % (e_cpu[c],)
    print("%s: worst column %s dev %.3g over %d rows%s" % (what, c, w, np.asarray(ref).shape[0], cpu))
    if not cpu_bar:
        assert w < tol, (what, c, w)
        return
    for c, v in d.items():
        bar = tol if e_cpu[c] == "zero" or e_cpu[c] <= tol / 3 else 4 * e_cpu[c]
        assert v == "zero" or v < bar, (what, c, v, bar, e_cpu[c])


def conv_rec_dx_call(L):
    """the development entry hl_debug_conv_rec_dx of learner L's library, with its argument types"""
    import ctypes as C
    f = L.api.lib.hl_debug_conv_rec_dx
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
    return f


def conv_rec_dx_form(L):
    """(1 where tm_conv_dx_kernel forms the gradient into the feature rows, 0 where the GEMM_X problem does; 1 where the net runs time-step-major)"""
    import ctypes as C
    dims = (C.c_int32 * 2)()
    L._ck(conv_rec_dx_call(L)(L.h, 4, None, 0, dims))
    return dims[0], dims[1]


COL_ROWS = 16      # a column's scale is taken over a batch: calls of fewer rows are left to the row-wise checks
