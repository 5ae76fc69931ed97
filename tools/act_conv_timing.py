"""Wall-clock cost of hl_forward on feed-forward nets behind convolutions, this build against a build of the parent commit (the route of
smarties_amd/csrc/actconv.hip -- the conv stack of a row per workgroup, then act_rows_kernel on the feature rows -- against the training
forward launches over minibatch buffer 0 it replaces), on four shapes --

  atari     the RACER_atari.json net: 84 x 84 frames x (1 + 3 appended), four SoftSign convolutions, dense 64, 6 options, batchSize 128
  strided   dimS 576: a 12 x 12 x 4 image, 8 channels 3 x 3, then 16 channels 4 x 4 stride 2, dense 32 (Tanh), batchSize 128
  frame20   dimS 800 x (1 + 3 appended): 20 x 20 x 8, 16 channels 6 x 6 stride 2, dense 40; rows of 12.5 KB
  frame42   dimS 7056: 42 x 42 x 4, 8 channels 8 x 8 stride 2, 16 channels 6 x 6 stride 2, dense 64; rows of 27.6 KB
(the last two place HL_ACT_CONV_MAX_ROW_BYTES between the 2.3 KB rows of `strided` and the 110 KB rows of `atari`)

-- at n = 1, 16, 64, 256 and 1024 rows, and an interleaved loop -- hl_step(1), then hl_forward(n) -- as an embedding runs it: its time per
iteration shows what keeping the minibatch drawn ahead (and not synchronising the stream) is worth.  The route is judged by the loop.

Method: every measurement is a child process of its own (a fresh HIP context, one library mapped), the two libraries ALTERNATING for
--rounds rounds (default 5); inside a child what is timed is the C call alone, per n the median of --calls calls after --warmup calls.
Reported per n and library: the median over the rounds' medians and their spread (min, max).  A route "loses" only where its median is
above the other's by more than the two spreads.  --open: this build runs with SMARTIES_HIP_GENERIC=4096, which holds the switch
HL_ACT_CONV_MAX_ROW_BYTES open -- every shape then takes the new route, also those the library keeps on the training launches.

    python tools/act_conv_timing.py --parent-lib PATH/libsmarties_hip.so [--rounds 5] [--calls 30] [--open] [--out profiles/act_conv_timing.json]

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

NS = (1, 16, 64, 256, 1024)
SHAPES = {
    "atari": ("RACER_atari.json: 84x84x(1+3), conv 8/16/32/64, dense 64, 6 options, batchSize 128",
              dict(dimS=7056, dimA=1, bounded=[0], discrete=True, n_options=6, nAppendedObs=3, hidden=(64,), nnFunc="SoftSign", batchSize=128,
                   conv=[(84, 84, 4, 8, 8, 4), (20, 20, 8, 16, 6, 2), (8, 8, 16, 32, 4, 1), (5, 5, 32, 64, 3, 1)], maxTotObsNum=2048, randSeed=1),
              dict(lenMin=20, lenMax=40, pTerm=0.5), 40),
    "frame42": ("dimS 7056: 42x42x4, conv 8 (8x8, stride 2) / 16 (6x6, stride 2), dense 64 SoftSign, batchSize 128",
                dict(dimS=7056, dimA=2, bounded=[1, 0], hidden=(64,), nnFunc="SoftSign", batchSize=128, conv=[(42, 42, 4, 8, 8, 2), (18, 18, 8, 16, 6, 2)],
                     maxTotObsNum=4096, randSeed=1),
                dict(lenMin=20, lenMax=40, pTerm=0.5), 60),
    "frame20": ("dimS 800 x (1 + 3): 20x20x8, conv 16 (6x6, stride 2), dense 40 SoftSign, batchSize 128",
                dict(dimS=800, dimA=2, bounded=[1, 0], nAppendedObs=3, hidden=(40,), nnFunc="SoftSign", batchSize=128, conv=[(20, 20, 8, 16, 6, 2)],
                     maxTotObsNum=8192, randSeed=1),
                dict(lenMin=30, lenMax=80, pTerm=0.5), 50),
    "strided": ("dimS 576: 12x12x4, conv 8 (3x3) / 16 (4x4, stride 2), dense 32 Tanh, batchSize 128",
                dict(dimS=576, dimA=2, bounded=[1, 0], hidden=(32,), nnFunc="Tanh", batchSize=128, conv=[(12, 12, 4, 8, 3, 1), (10, 10, 8, 16, 4, 2)],
                     maxTotObsNum=16384, randSeed=1),
                dict(lenMin=50, lenMax=150, pTerm=0.7), 50),
}


def child(lib, calls, warmup, loop_iters):
    import numpy as np
    import torch  # noqa: F401  (first, so that a single HIP runtime is resident in the process)
    from smarties_amd import capi
    from oracle_api import fill_synth, synth_cfg
    api = capi.CApi(lib, "hl_")
    res = {}
    for name, (_, cfg, sc, n_eps) in SHAPES.items():
        cfg = dict(cfg)
        if cfg.pop("discrete", False):
            cfg["adv_kind"] = capi.ADV_DISCRETE
        L = capi.Learner(api, capi.make_config(**cfg)); L.init_weights()
        fill_synth(L, synth_cfg(seed=3, dimS=cfg["dimS"], dimA=cfg["dimA"], **sc), n_eps); L.initialize()
        L.step(5); L.sync()
        st = np.random.default_rng(0).standard_normal((max(NS), L.dIn)).astype(np.float32)
        out = np.zeros((max(NS), L.nOut), np.float64)
        st_p, out_p = st.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_double))
        fwd = api.fn("forward")

        def call(n):
            rc = fwd(L.h, n, st_p, out_p)
            assert rc == 0, rc

        us, loop = {}, {}
        for n in NS:
            for _ in range(warmup):
                call(n)
            t = []
            for _ in range(calls):
                t0 = time.perf_counter(); call(n); t.append(time.perf_counter() - t0)
            us[n] = float(np.median(t) * 1e6)
        for n in NS:
            for _ in range(3):
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
        res[name] = dict(forward_us={str(n): us[n] for n in NS}, loop_us={str(n): loop[n] for n in NS}, step_only_us=step_only)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--loop-iters", type=int, default=30)
    ap.add_argument("--open", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.calls, a.warmup, a.loop_iters)
    assert a.rounds >= 5, "medians of at least five alternating runs"
    branch = os.path.join(ROOT, "smarties_amd", "libsmarties_hip.so")
    libs = {"branch": (branch, "4096" if a.open else None)}
    if a.parent_lib:
        libs["parent"] = (os.path.abspath(a.parent_lib), None)
    runs = {k: [] for k in libs}
    for r in range(a.rounds):
        for k, (lib, generic) in libs.items():
            env = dict(os.environ)
            env.pop("SMARTIES_HIP_GENERIC", None)
            if generic:
                env["SMARTIES_HIP_GENERIC"] = generic
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, "--calls", str(a.calls), "--warmup", str(a.warmup),
                                "--loop-iters", str(a.loop_iters)], stdout=subprocess.PIPE, text=True, timeout=300, env=env)
            if p.returncode != 0:      # (nothing more is started on the device after a child that failed)
                sys.exit("round %d, %s: the child ended with status %d" % (r, k, p.returncode))
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1]
            runs[k].append(json.loads(line[7:]))
            print("round %d %s done" % (r, k), flush=True)

    def stat(vals):
        v = sorted(vals)
        return dict(median=v[len(v) // 2], min=v[0], max=v[-1])

    res = dict(gate_open=bool(a.open), rounds=a.rounds, calls=a.calls, warmup=a.warmup, loop_iters=a.loop_iters, shapes={})
    for name, (what, _, _, _) in SHAPES.items():
        s = dict(shape=what, forward_us={}, loop_us={}, step_only_us={k: stat([x[name]["step_only_us"] for x in runs[k]]) for k in libs})
        for n in NS:
            s["forward_us"][str(n)] = {k: stat([x[name]["forward_us"][str(n)] for x in runs[k]]) for k in libs}
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
