#!/usr/bin/env python3
"""Bits of the workgroup-per-sample recurrent kernels (smarties_amd/csrc/rec.hip: rec_*, lstm_*_lds, mgu_*, rnn_*), for comparing two
builds of the library: the fifteen nets of tests/test_hip_rec_sample_kernels.py (one per instantiation) plus the convolutional front and
the two-type stack of tests/test_hip_act_win.py.  Per net: three training steps (TAP_FLAT of each), then the generator state, the
parameters and both Adam moments, hl_forward_sequence on windows of 1, 2 and nnBPTTseq + 1 states and, for the last two nets,
hl_forward_sequences of ragged windows.  One process per library:

  python tools/rec_sample_dump.py OUT.npz [--lib libsmarties_hip.so]       dump
  python tools/rec_sample_dump.py --compare A.npz B.npz [--json OUT.json]  every array np.array_equal, or exit 1
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def dump(out, lib):
    import torch  # noqa: F401  (first, so that a single HIP runtime is resident in the process)
    from smarties_amd import capi
    from oracle_api import fill_synth
    import test_hip_rec_sample_kernels as rs
    import test_hip_act_win as aw
    api = capi.CApi(lib) if lib else capi.load_hip()
    nets = [(n,) + rs.shape_cfg(n) + (None,) for n in rs.SHAPES]
    nets += [(n, aw._cfg(n), aw._synth(n), aw._ragged_lengths(n)) for n in ("conv-lstm", "rnn-enc-mgu")]
    arrays = {}
    for name, kw, sc, ragged in nets:
        G = capi.Learner(api, capi.make_config(**kw))
        G.init_weights(); fill_synth(G, sc, 30); G.initialize(); G.set_tap(True)
        for i in range(3):
            G.step(1)
            arrays["%s/flat%d" % (name, i)] = G.readback(capi.TAP_FLAT)
        arrays[name + "/rng"] = G.get_rng_state()
        for what, a in zip(("params", "moment1", "moment2"), G.get_params()):
            arrays["%s/%s" % (name, what)] = a
        for w in rs.act_windows(kw):
            arrays["%s/forward_sequence%d" % (name, w.shape[0])] = G.forward_sequence(w)
        if ragged:
            arrays[name + "/forward_sequences"] = G.forward_sequences(aw._windows(np.random.default_rng(11), 20, kw["dimS"], ragged))
        G.close()
        print(name, "done", flush=True)
    np.savez(out, **arrays)


def compare(a, b, out_json):
    A, B = np.load(a), np.load(b)
    rows = [dict(array=k, shape=list(A[k].shape), dtype=str(A[k].dtype), equal=bool(k in B.files and np.array_equal(A[k], B[k]))) for k in A.files]
    missing = [k for k in B.files if k not in A.files]
    ok = all(r["equal"] for r in rows) and not missing
    res = dict(what="tools/rec_sample_dump.py: parent build against this one, np.array_equal per array", arrays=len(rows), all_equal=ok,
               only_in_second=missing, rows=rows)
    if out_json:
        with open(out_json, "w") as f:
            json.dump(res, f, indent=1)
    print("%d arrays, all equal: %s" % (len(rows), ok))
    for r in rows:
        if not r["equal"]:
            print("DIFFERS", r["array"], r["shape"])
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--lib")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.json))
    if not args.out:
        ap.error("OUT.npz")
    dump(args.out, args.lib)
