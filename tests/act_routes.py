"""The route table of the acting calls: which launches every acting call makes, per net, SMARTIES_HIP_GENERIC, call, row or agent count
and source.  Recorded once from the library (tools/act_route_table.py -> tests/act_routes_parent.json) and held to entry by entry
(tests/test_hip_act_routes.py): the tool and the test build the table with the one function below, on the nets of tests/acting.py."""
import hashlib
import os

import numpy as np

from acting import (BAND_NETS, DENSE_BASE, FALLBACK, KINDS, LDS_NETS, N_EPS, NETS, ROWS_WIDE, WIDE_IDS, WIDE_SHAPES, _BASE, _count, _packed,
                    _rec_cfg, _synth_learner, _training_forwards, _wide_cfg)
from smarties_amd import capi

ACT_LABELS = ("act_rows", "act_conv", "act_seq", "act_tm_chain", "act_win_chain", "act_forward_dev", "act_rows_dev", "act_rows_panel_dev",
              "act_stack_dev", "act_seq_dev", "act_tm_dev", "act_conv_dev", "act_conv_band_dev", "act_head_kernel")
ROUTES_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "act_routes_parent.json")
_REC_SYNTH = dict(seed=43, dimS=6, dimA=2, lenMin=5, lenMax=40, pTerm=0.5)


def _route_nets():
    """name -> (configuration, synthetic episodes, their number)"""
    def sc(kw, lo=4, hi=12):
        return dict(seed=21, dimS=kw["dimS"], dimA=kw["dimA"], lenMin=lo, lenMax=hi, pTerm=0.5)
    nets = {"dense-base": (DENSE_BASE, sc(DENSE_BASE, 5, 30), 20)}
    for name, kw in ROWS_WIDE.items():      # a layer / an input row beyond ACT_MAXW
        nets["dense-" + name] = (kw, sc(kw, 5, 40), 20)
    big = dict(dimS=9, dimA=3, bounded=[1, 0, 0], hidden=(1024, 768), nnFunc="Tanh", batchSize=600, maxTotObsNum=4000, randSeed=19)
    nets["dense-large-b600"] = (big, sc(big, 20, 40), 40)      # beyond ACT_ROWS_SMALL_NET weights, 2 x Mmax = 2400 rows
    wide = dict(_BASE, dimS=8193, hidden=(32,))
    nets["dense-8193"] = (wide, sc(wide), 10)
    for name, kw in list(NETS.items()) + list(LDS_NETS.items()):
        nets["conv-" + name] = (kw, sc(kw), N_EPS.get(name, 30))
    for name, entry in BAND_NETS.items():
        if name not in LDS_NETS:
            nets["band-" + name] = (entry[0], sc(entry[0]), 14 if name == "nature" else 30)
    for kind in KINDS:
        for hidden in ((32, 32), (272,)):
            nets["rec-%s-%s" % (kind, "x".join(map(str, hidden)))] = (_rec_cfg(KINDS[kind], hidden), _REC_SYNTH, 40)
    for name in ("rnn-encoder-mgu", "conv-lstm"):
        nets["rec-" + name] = FALLBACK[name] + (40,)
    for shape, name in zip(WIDE_SHAPES, WIDE_IDS):
        kw = _wide_cfg(shape)
        nets["wide-" + name] = (kw, sc(kw, 2, 30), 60)
    return nets


ROUTE_NETS = _route_nets()


def _route_counters(L):
    return [_count(L, k) for k in ACT_LABELS] + list(_training_forwards(L))


def _route_entry(L, call):
    """one call: [status, error text, {acting label: launches}, [training forwards: first conv layer, dense layers], SHA-256 of the outputs]"""
    import torch
    c0 = _route_counters(L)
    status, err, digest = 0, "", ""
    try:
        got = call()
        torch.cuda.synchronize()
        arrs = [x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in ([] if got is None else got if isinstance(got, (tuple, list)) else [got])]
        digest = hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrs)).hexdigest()
    except capi.HlError as e:
        status, err = e.status, str(e)
    d = [b - a for a, b in zip(c0, _route_counters(L))]
    return [status, err, {k: v for k, v in zip(ACT_LABELS, d) if v}, d[len(ACT_LABELS):], digest]


def route_table(hip_api, name):
    """{"bits|call|n|source": entry} of one net of ROUTE_NETS: per SMARTIES_HIP_GENERIC in (0, 2, 8192; conv nets 4096 too) a learner with
    initial weights and a filled replay, no gradient step; the host and the device calls on rows at n = 1, 64, 65, 1025 (and around two
    rounds of the training rows where that is more) and on windows at n = 3, 65 agents with ragged lengths from 1 to the longest window,
    the device calls under both sources (the two with the head behind them at n = 1, 65 rows and 3, 65 agents) -- and under the snapshot
    source once before any snapshot was taken"""
    import torch
    kw, sc_kw, n_eps = ROUTE_NETS[name]
    rec, nApp = "nn_type" in kw, kw.get("nAppendedObs", 0)
    dS, dIn = kw["dimS"], kw["dimS"] * (1 + nApp)
    mmax = -(-2 * kw["batchSize"] // 16) * 16
    ns_rows = [1, 64, 65, 1025] + ([2 * mmax - 1, 2 * mmax] if 2 * mmax > 1025 else [])
    top = kw["nnBPTTseq"] + 1 + nApp if rec else nApp + 2
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((max(ns_rows), dIn), dtype=np.float32) * np.float32(1.5) + np.float32(0.2)
    wins = [rng.standard_normal(([1, top, 2, max(top - nApp, 1), 3][i % 5], dS), dtype=np.float32) * np.float32(1.5) + np.float32(0.2) for i in range(65)]
    rows_d = torch.from_numpy(rows).cuda()
    packed = {n: _packed(wins[:n]) for n in (3, 65)}
    packed_d = {n: [torch.from_numpy(a).cuda() for a in p[:3]] for n, p in packed.items()}
    table = {}
    saved = os.environ.get("SMARTIES_HIP_GENERIC")
    try:
        for bits in (0, 2, 8192) + ((4096,) if "conv" in kw else ()):
            os.environ["SMARTIES_HIP_GENERIC"] = str(bits)      # read when the learner is created
            L = _synth_learner(hip_api, kw, sc_kw, n_eps)
            L.timing_enable(True)

            def put(call, n, source, fn):
                table["%d|%s|%d|%s" % (bits, call, n, source)] = _route_entry(L, fn)

            def device(source):
                for n in ns_rows:
                    put("forward_dev", n, source, lambda: L.forward_dev(rows_d[:n]))
                for n, (st, first, steps) in packed_d.items():
                    put("forward_sequences_dev", n, source, lambda: L.forward_sequences_dev(st, first, steps, 1))
                # (the head behind the forward pass: the same launches and one more; below and above ACT_MAXROWS, where the forward pass is chunked)
                for n in (1, 65):
                    put("select_actions_dev", n, source, lambda: L.select_actions_dev(rows_d[:n]))
                for n, (st, first, steps) in packed_d.items():
                    put("select_actions_sequences_dev", n, source, lambda: L.select_actions_sequences_dev(st, first, steps, 1))

            for n in ns_rows:
                put("forward", n, "host", lambda: L.forward(rows[:n]))
            for n in (3, 65):
                put("forward_sequences", n, "host", lambda: L.forward_sequences(wins[:n]))
            device("live")
            L.act_source("snapshot")
            put("forward_dev", 1, "snapshot-none", lambda: L.forward_dev(rows_d[:1]))
            put("forward_sequences_dev", 3, "snapshot-none", lambda: L.forward_sequences_dev(*packed_d[3], 1))
            put("policy_snapshot", 0, "snapshot", L.policy_snapshot)
            device("snapshot")
            L.timing_enable(False)
            L.close()
    finally:
        if saved is None:
            os.environ.pop("SMARTIES_HIP_GENERIC", None)
        else:
            os.environ["SMARTIES_HIP_GENERIC"] = saved
    return table


def route_pack(tables):
    """{net: table} as the file holds it: every error text and every hash once ("errors", "hashes": the refusals repeat, and so do the
    outputs of routes that give the same bits), the entries of a net grouped by "bits|call|source" as {n: entry} with indices in place of
    the texts (-1: none; a hash of null: dropped, the outputs differed between two recordings) and trailing defaults left out, and groups
    with the same entries -- live and snapshot source, bits that do not move the route -- written once under all their names"""
    texts = sorted({e[1] for t in tables.values() for e in t.values() if e[1]})
    hashes = sorted({e[4] for t in tables.values() for e in t.values() if e[4]})
    nets = {}
    for name, table in tables.items():
        groups = {}
        for key, (status, err, labels, forwards, digest) in table.items():
            bits, call, n, source = key.split("|")
            e = [status, texts.index(err) if err else -1, labels, forwards, digest if digest is None else hashes.index(digest) if digest else -1]
            for default in (-1, [0, 0], {}, -1):
                if e[-1] is None or e[-1] != default:
                    break
                e.pop()
            groups.setdefault("%s|%s|%s" % (bits, call, source), {})[n] = e
        nets[name] = []
        for group, by_n in groups.items():
            same = [g for g in nets[name] if g[1] == by_n]
            if same:
                same[0][0].append(group)
            else:
                nets[name].append([[group], by_n])
    return {"errors": texts, "hashes": hashes, "nets": nets}


def route_unpack(packed):
    tables = {}
    for name, groups in packed["nets"].items():
        table = tables[name] = {}
        for names, by_n in groups:
            for group in names:
                bits, call, source = group.split("|")
                for n, e in by_n.items():
                    status, err, labels, forwards, digest = list(e) + [-1, {}, [0, 0], -1][len(e) - 1:]
                    table["%s|%s|%s|%s" % (bits, call, n, source)] = [status, packed["errors"][err] if err >= 0 else "", labels, forwards,
                                                                      digest if digest is None else packed["hashes"][digest] if digest >= 0 else ""]
    return tables


def route_table_diff(got, want):
    """the first entry at which two tables of a net differ (None: none); an entry recorded without a hash is held to its counters alone"""
    if sorted(got) != sorted(want):
        return "entries", sorted(set(got) ^ set(want))[:5]
    for key in want:
        g, w = list(got[key]), list(want[key])
        if w[4] is None:
            g[4] = None
        if g != w:
            return key, g, w
    return None
