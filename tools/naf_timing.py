#!/usr/bin/env python3
"""Device time of the NAF head launch and of the eager NAF step: cfg-NS's net (dimS 17, dense 256 x 256), dimA 6, batch 256, both estimators
that change the launch list ("none": the target path in front of the head; "retrace": the head alone).

  launches_us  hl_timing_get: events around the launches of eager steps, --per steps per round, median over --rounds (least, largest)
  step_us      host clock around hl_step(--per) + hl_sync, per step, median over --rounds (least, largest)
--bench-parent <tree>: also runs bench.py of this tree and of <tree> (a checkout of the parent commit with its library built) in turn,
--bench-rounds times each, and records every value: the run-to-run spread of the headline figure on the same machine, and the two medians.

  python tools/naf_timing.py --out profiles/naf_timing.json [--bench-parent <tree>]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("step_tail_kernel", "fwd_chain", "gemm16_fwd0", "gemm16_fwd1", "naf_next_gather", "naf_tgt_fwd", "naf_vtgt", "head_naf", "gemm16_dx1",
         "dw_table_kernel", "gemm16_dw", "naf_adam_target", "post_kernel")


def bench(tree, steps, warmup):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                         capture_output=True, text=True, check=True).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["ms_per_step"] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--per", type=int, default=200)
    ap.add_argument("--bench-parent", default="")
    ap.add_argument("--bench-rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch  # (first, so that a single HIP runtime is resident in the process)
    torch.cuda.set_device(0)
    from smarties_amd import capi, load_hip
    api = load_hip()
    res = dict(command=" ".join(["python"] + sys.argv), batch=256, hidden=[256, 256], dimS=17, dimA=6, rounds=a.rounds, per=a.per, cases={})
    mm = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    for est in ("none", "retrace"):
        L = capi.create_naf(api, 0.01, dimS=17, dimA=6, hidden=(256, 256), batchSize=256, maxTotObsNum=100000, returnsEstimator=est, randSeed=43, device_id=0)
        L.init_weights()
        rng = np.random.default_rng(5)
        for e in range(200):
            n = 100
            mu = np.concatenate([0.1 * rng.normal(size=(n, 6)), np.full((n, 6), 0.45)], 1)
            L.append_episode(rng.normal(size=(n, 17)).astype(np.float32), mu[:, :6] + 0.3 * rng.normal(size=(n, 6)), mu, rng.normal(size=n),
                             (0.5 * rng.normal(size=n)).astype(np.float32), e % 2, e)
        L.initialize()
        L.step(50); L.sync()      # warm-up: every launch of the step has run
        wall, timed = [], {k: [] for k in NAMES}
        for r in range(a.rounds):
            t0 = time.perf_counter(); L.step(a.per); L.sync(); wall.append((time.perf_counter() - t0) * 1e6 / a.per)
        for r in range(a.rounds):      # (the timers synchronise around every launch: a run of their own)
            L.timing_enable(True); L.step(a.per); L.sync()
            for k in NAMES:
                ms, cnt = L.timing_get(k)
                timed[k].append(ms * 1e3 * cnt / a.per)
            L.timing_enable(False)
        res["cases"][est] = dict(step_us=mm(wall), launches_us={k: mm(v) for k, v in timed.items() if max(v) > 0})
        print("NAF %-8s eager step %.1f us (%.1f .. %.1f); head_naf %.1f us" % (est, np.median(wall), min(wall), max(wall), np.median(timed["head_naf"])), flush=True)
        L.close()
    if a.bench_parent:
        runs = {"this": [], "parent": []}
        for r in range(a.bench_rounds):      # alternating, in one call
            runs["this"].append(bench(ROOT, 2000, 200)); runs["parent"].append(bench(os.path.abspath(a.bench_parent), 2000, 200))
        res["bench_us_per_step"] = dict(runs, this_median=float(np.median(runs["this"])), parent_median=float(np.median(runs["parent"])),
                                        spread_this=float(max(runs["this"]) - min(runs["this"])), spread_parent=float(max(runs["parent"]) - min(runs["parent"])))
        print("bench.py us per step: this %r, parent %r" % (runs["this"], runs["parent"]), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
