"""Wall-clock cost of hl_forward on dense nets, this build against a build of the parent commit (the many-row route of
smarties_amd/csrc/actrows.hip against the route over the training buffers it replaces), on three shapes --

  2x256    the headline net: dimS 17, dimA 6, two SoftSign layers of 256, batchSize 256
  2x512    two SoftSign layers of 512, same otherwise: the shape that placed HL_ACT_ROWS_SMALL_NET (just above it)
  3x1024   three Tanh layers of 1024, dimS 17, dimA 6, batchSize 256

-- at n = 1, 64 (the one-kernel route, unchanged: the control), 65, 256, 1024 and 4096 rows, and an interleaved loop -- hl_step(1), then
hl_forward(n) -- whose time per iteration shows what keeping the minibatch drawn ahead is worth.

Method: every measurement is a child process of its own (a fresh HIP context, one library mapped), the two libraries ALTERNATING for
--rounds rounds (default 5); inside a child what is timed is the C call alone, per n the median of --calls calls after --warmup calls.
Reported per n and library: the median over the rounds' medians and their spread (min, max).  A route "loses" only where its median is
above the other's by more than the two spreads.

    python tools/act_rows_timing.py --parent-lib PATH/libsmarties_hip.so [--rounds 5] [--calls 100] [--out profiles/act_rows_timing.json]

--parent-lib: libsmarties_hip.so of the parent commit, built from a checkout of it (`git worktree add DIR HEAD~1`, then
`python -c "import __graft_entry__ as g; g.build_hip()"` in DIR).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NS = (1, 64, 65, 256, 1024, 4096)
LOOP_NS = (65, 256, 1024)
SHAPES = {
    "2x256": ("dimS 17, dimA 6, SoftSign 2x256, batchSize 256", dict(dimS=17, dimA=6, hidden=(256, 256), nnFunc="SoftSign", batchSize=256,
                                                                    maxTotObsNum=65536, randSeed=1)),
    "2x512": ("dimS 17, dimA 6, SoftSign 2x512, batchSize 256", dict(dimS=17, dimA=6, hidden=(512, 512), nnFunc="SoftSign", batchSize=256,
                                                                    maxTotObsNum=65536, randSeed=1)),
    "3x1024": ("dimS 17, dimA 6, Tanh 3x1024, batchSize 256", dict(dimS=17, dimA=6, hidden=(1024, 1024, 1024), nnFunc="Tanh", batchSize=256,
                                                                  maxTotObsNum=65536, randSeed=1)),
}


def child(lib, calls, warmup, loop_iters):
    import numpy as np
    import torch  # noqa: F401  (first, so that a single HIP runtime is resident in the process)
    from smarties_amd import capi
    from oracle_api import fill_synth, synth_cfg
    api = capi.CApi(lib, "hl_")
    res = {}
    for name, (_, cfg) in SHAPES.items():
        L = capi.Learner(api, capi.make_config(**cfg)); L.init_weights()
        fill_synth(L, synth_cfg(seed=3, dimS=cfg["dimS"], dimA=cfg["dimA"], lenMin=100, lenMax=300, pTerm=0.7), 50); L.initialize()
        L.step(10); L.sync()
        st = np.random.default_rng(0).standard_normal((max(NS), L.dIn)).astype(np.float32)
        out = np.zeros((max(NS), L.nOut), np.float64)
        st_p, out_p = st.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_double))
        fwd = api.fn("forward")

        def call(n):
            rc = fwd(L.h, n, st_p, out_p)
            assert rc == 0, rc

        us = {}
        for n in NS:
            for _ in range(warmup):
                call(n)
            t = []
            for _ in range(calls):
                t0 = time.perf_counter(); call(n); t.append(time.perf_counter() - t0)
            us[n] = float(np.median(t) * 1e6)
        loop = {}
        for n in LOOP_NS:
            for _ in range(5):
                L.step(1); call(n)
            L.sync()
            t0 = time.perf_counter()
            for _ in range(loop_iters):
                L.step(1)
                call(n)
            L.sync()
            loop[n] = (time.perf_counter() - t0) / loop_iters * 1e6
        t0 = time.perf_counter()
        for _ in range(loop_iters):
            L.step(1)
        L.sync()
        step_only = (time.perf_counter() - t0) / loop_iters * 1e6
        L.close()
        res[name] = dict(forward_us={str(n): us[n] for n in NS}, loop_us={str(n): loop[n] for n in LOOP_NS}, step_only_us=step_only)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loop-iters", type=int, default=100)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.calls, a.warmup, a.loop_iters)
    assert a.rounds >= 5, "medians of at least five alternating runs"
    libs = {"branch": os.path.join(ROOT, "smarties_amd", "libsmarties_hip.so")}
    if a.parent_lib:
        libs["parent"] = os.path.abspath(a.parent_lib)
    runs = {k: [] for k in libs}
    for r in range(a.rounds):
        for k, lib in libs.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, "--calls", str(a.calls), "--warmup", str(a.warmup),
                                "--loop-iters", str(a.loop_iters)], stdout=subprocess.PIPE, text=True, timeout=300)
            if p.returncode != 0:      # (nothing more is started on the device after a child that failed)
                sys.exit("round %d, %s: the child ended with status %d" % (r, k, p.returncode))
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1]
            runs[k].append(json.loads(line[7:]))
            print("round %d %s done" % (r, k), flush=True)

    def stat(vals):
        v = sorted(vals)
        return dict(median=v[len(v) // 2], min=v[0], max=v[-1])

    res = dict(rounds=a.rounds, calls=a.calls, warmup=a.warmup, loop_iters=a.loop_iters, shapes={})
    for name, (what, _) in SHAPES.items():
        s = dict(shape=what, forward_us={}, loop_us={}, step_only_us={k: stat([x[name]["step_only_us"] for x in runs[k]]) for k in libs})
        for n in NS:
            s["forward_us"][str(n)] = {k: stat([x[name]["forward_us"][str(n)] for x in runs[k]]) for k in libs}
        for n in LOOP_NS:
            s["loop_us"][str(n)] = {k: stat([x[name]["loop_us"][str(n)] for x in runs[k]]) for k in libs}
        res["shapes"][name] = s
        print("%s: %s" % (name, what))
        for sect in ("forward_us", "loop_us"):
            for n, d in s[sect].items():
                print("  %-10s n=%5s  " % (sect, n) + "   ".join("%s %8.1f us (%.1f .. %.1f)" % (k, d[k]["median"], d[k]["min"], d[k]["max"]) for k in d))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
