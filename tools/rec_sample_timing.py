#!/usr/bin/env python3
"""us per replayed training step of four nets whose recurrent layers run in the workgroup-per-sample kernels (smarties_amd/csrc/rec.hip),
for comparing two builds of the library in alternating runs, one fresh process per run:

  conv2_lstm32_b64_bptt4, pomdp_rnn24_mgu2x16_b128_bptt5    bench.py's own configurations (bench.other_configs)
  lstm_2x16_b128_bptt16, mgu_2x16_b128_bptt16               two layers of 16 cells (lstm_*_lds_kernel<2>, mgu_*_kernel<true, 2>)

  python tools/rec_sample_timing.py [--lib libsmarties_hip.so]                      one run, one JSON line
  python tools/rec_sample_timing.py --against PARENT.so [--runs 5] [--json OUT]     PARENT, this, PARENT, ...: medians and the parent's spread
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def one_run(lib, steps):
    import numpy as np
    import torch  # noqa: F401  (first, so that a single HIP runtime is resident in the process)
    import bench
    from smarties_amd import capi
    api = capi.CApi(lib) if lib else capi.load_hip()
    res = {k: v["us_per_step"] for k, v in bench.other_configs(api, steps=4 * steps, only=["conv2_lstm32_b64_bptt4", "pomdp_rnn24_mgu2x16_b128_bptt5"]).items()}
    for name, kind in (("lstm_2x16_b128_bptt16", capi.NN_LSTM), ("mgu_2x16_b128_bptt16", capi.NN_MGU)):
        L = capi.Learner(api, capi.make_config(randSeed=7, dimS=4, dimA=1, bounded=[1], hidden=(16, 16), nnFunc="Tanh", batchSize=128, maxTotObsNum=262144,
                                               gamma=0.99, adv_kind=capi.ADV_GAUSSIAN, nn_type=kind, nnBPTTseq=16, nnLambda=1e-6, explNoise=0.1))
        L.init_weights()
        for e in range(300):
            L.append_episode(**bench.synthetic_episode(np, e, dS=4, dA=1, N=200))
        L.initialize()
        L.step(64); L.sync()      # (replayed graphs from here on)
        t0 = time.perf_counter(); L.step(steps); L.sync()
        res[name] = round((time.perf_counter() - t0) / steps * 1e6, 2)
        L.close()
    return res


def against(parent, runs, steps, out_json):
    series = {"parent": [], "new": []}
    for i in range(2 * runs):
        who = "parent" if i % 2 == 0 else "new"
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(steps)] + (["--lib", parent] if who == "parent" else [])
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            return out.returncode
        series[who].append(json.loads(out.stdout.strip().splitlines()[-1]))
        print(who, series[who][-1], flush=True)
    res = {"what": "us per replayed step, alternating fresh processes (parent, new, parent, ...)", "steps": steps, "runs": series, "summary": {}}
    ok = True
    for k in series["parent"][0]:
        p, n = [r[k] for r in series["parent"]], [r[k] for r in series["new"]]
        s = dict(parent_median=statistics.median(p), new_median=statistics.median(n), parent_spread=round(max(p) - min(p), 2))
        s["within_parent_spread"] = s["new_median"] <= s["parent_median"] + s["parent_spread"]
        ok = ok and s["within_parent_spread"]
        res["summary"][k] = s
    print(json.dumps(res["summary"], indent=1))
    if out_json:
        with open(out_json, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if ok else 2


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--against", metavar="PARENT.so")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.against:
        sys.exit(against(args.against, args.runs, args.steps, args.json))
    print(json.dumps(one_run(args.lib, args.steps)))
