#!/usr/bin/env python3
"""Device time of the DPG target launch (dpgt.hip: dpg_target_kernel), of the DPG head launch and of the eager DPG step, with cfg-NS's
net: dense (256, 256), dimS 17, dimA 6, batch 256.

  launches_us  hl_timing_get: events around the launches of eager steps, --per steps per round, median over --rounds (least, largest)
  step_us      host clock around hl_step(--per) + hl_sync, per step, median over --rounds (least, largest)
Beside them, from the same call: a NAF learner of the same shape (returnsEstimator "none"), whose naf_tgt_fwd counter holds the
per-layer launches of ONE target forward through the generic launches (two launches per step here) -- the yardstick for what a target
forward costs there; the DPG target launch runs four such chains (two nets on two row sets) and the critic's backward to the action.
--bench-parent <tree>: also runs bench.py of this tree and of <tree> (a checkout of the parent commit with its library built) in turn,
--bench-rounds times each, and records every value: the run-to-run spread of the headline figure on the same machine, and the two medians.

  python tools/dpg_timing.py --out profiles/dpg_timing.json [--bench-parent <tree>]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("step_tail_kernel", "fwd_chain", "gemm16_fwd0", "gemm16_fwd1", "dpg_critic_gather", "dpg_critic_fwd", "dpg_target", "head_dpg", "dpg_critic_dx",
         "dpg_critic_dw", "naf_next_gather", "naf_tgt_fwd", "naf_vtgt", "head_naf", "gemm16_dx1", "dw_table_kernel", "gemm16_dw", "dpg_adam_target",
         "naf_adam_target", "post_kernel")
DS, DA, HIDDEN, B = 17, 6, (256, 256), 256


def bench(tree, steps, warmup):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                         capture_output=True, text=True, check=True).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["ms_per_step"] * 1e3


def measure(L, a):
    """fill the replay, warm up, then --rounds rounds by the host clock and --rounds under the launch timers"""
    rng = np.random.default_rng(5)
    L.init_weights()
    for e in range(100):
        n = 60
        mu = np.concatenate([0.1 * rng.normal(size=(n, DA)), np.full((n, DA), 0.4472135955)], 1)
        L.append_episode(rng.normal(size=(n, DS)).astype(np.float32), mu[:, :DA] + 0.3 * rng.normal(size=(n, DA)), mu, rng.normal(size=n),
                         (0.5 * rng.normal(size=n)).astype(np.float32), e % 2, e)
    L.initialize()
    L.step(50); L.sync()      # warm-up: every launch of the step has run
    mm = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    wall, timed = [], {k: [] for k in NAMES}
    for r in range(a.rounds):
        t0 = time.perf_counter(); L.step(a.per); L.sync(); wall.append((time.perf_counter() - t0) * 1e6 / a.per)
    for r in range(a.rounds):      # (the timers synchronise around every launch: a run of their own)
        L.timing_enable(True); L.step(a.per); L.sync()
        for k in NAMES:
            ms, cnt = L.timing_get(k)
            timed[k].append(ms * 1e3 * cnt / a.per)
        L.timing_enable(False)
    return dict(step_us=mm(wall), launches_us={k: mm(v) for k, v in timed.items() if max(v) > 0})


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
    kw = dict(dimS=DS, dimA=DA, bounded=[0] * DA, hidden=HIDDEN, batchSize=B, maxTotObsNum=100000, randSeed=43, device_id=0, returnsEstimator="none")
    res = dict(command=" ".join(["python"] + sys.argv), rounds=a.rounds, per=a.per, targetDelay=0.01, dimS=DS, dimA=DA, hidden=list(HIDDEN), batch=B)
    L = capi.create_dpg(api, 0.01, **kw); res["dpg"] = measure(L, a); L.close()
    L = capi.create_naf(api, 0.01, **kw); res["naf"] = measure(L, a); L.close()
    d, n = res["dpg"]["launches_us"], res["naf"]["launches_us"]
    print("DPG eager step %.1f us; dpg_target %.1f us, head_dpg %.1f us; NAF eager step %.1f us, naf_tgt_fwd (one target forward, per-layer launches) %.1f us"
          % (res["dpg"]["step_us"]["median"], d["dpg_target"]["median"], d["head_dpg"]["median"], res["naf"]["step_us"]["median"], n["naf_tgt_fwd"]["median"]), flush=True)
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
