#!/usr/bin/env python3
"""Device time of the DQN head launch (headdq.hip) and of the eager DQN step: dense (128, 128) at batch 128, dimS 24, with 18, 64, 128 and
512 options -- the shape of profiles/discrete_wide_timing.json --, and cfg-NS's (256, 256) at batch 256, dimS 17, with 18 options; both
estimators that change the launch list ("none": the next-state chains in front of the head, three products in it; "retrace": one product).

  launches_us  hl_timing_get: events around the launches of eager steps, --per steps per round, median over --rounds (least, largest)
  step_us      host clock around hl_step(--per) + hl_sync, per step, median over --rounds (least, largest)
Beside them, from the same call: head_kernel (headw.hip's head_wide_kernel, a wavefront per sample) of a discrete RACER learner of the
first shape at 128 and 512 options, timed the same way, and the ratio head_dqn ("none") / head_kernel.  That head does one product over
1 + 2 nOpt columns where the DQN head does three over nOpt each.
--bench-parent <tree>: also runs bench.py of this tree and of <tree> (a checkout of the parent commit with its library built) in turn,
--bench-rounds times each, and records every value: the run-to-run spread of the headline figure on the same machine, and the two medians.

  python tools/dqn_timing.py --out profiles/dqn_timing.json [--bench-parent <tree>]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("step_tail_kernel", "fwd_chain", "gemm16_fwd0", "gemm16_fwd1", "dqn_next_gather", "dqn_nxt_fwd", "dqn_tgt_fwd", "head_dqn", "head_kernel",
         "gemm16_dx1", "dw_table_kernel", "gemm16_dw", "dqn_adam_target", "post_kernel")
VALUES = {18: (18,), 64: (64,), 128: (128,), 512: (8, 8, 8)}
SHAPES = [(24, (128, 128), 128, n) for n in (18, 64, 128, 512)] + [(17, (256, 256), 256, 18)]      # (dimS, hidden, batch, options)


def bench(tree, steps, warmup):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                         capture_output=True, text=True, check=True).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["ms_per_step"] * 1e3


def measure(L, dS, nopt, a):
    """fill the replay, warm up, then --rounds rounds by the host clock and --rounds under the launch timers"""
    values = VALUES[nopt]; rng = np.random.default_rng(nopt); shifts = np.concatenate([[1], np.cumprod(values)[:-1]])
    L.init_weights()
    for e in range(100):
        n = 60
        mu = rng.uniform(0.5, 1.5, size=(n, nopt)); mu /= mu.sum(1, keepdims=True)
        act = (rng.integers(0, nopt, size=n)[:, None] // shifts[None, :]) % np.asarray(values)[None, :] + 0.1
        L.append_episode(rng.normal(size=(n, dS)).astype(np.float32), act, mu, rng.normal(size=n), (0.5 * rng.normal(size=n)).astype(np.float32), e % 2, e)
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
    res = dict(command=" ".join(["python"] + sys.argv), rounds=a.rounds, per=a.per, targetDelay=0.01, cases={}, racer_head_kernel={}, ratio_head_dqn_none_to_head_kernel={})
    for dS, hidden, B, nopt in SHAPES:
        kw = dict(dimS=dS, hidden=hidden, batchSize=B, maxTotObsNum=100000, randSeed=43, device_id=0)
        case = dict(dimS=dS, hidden=list(hidden), batch=B, options=nopt)
        for est in ("none", "retrace"):
            L = capi.create_dqn(api, 0.01, VALUES[nopt], returnsEstimator=est, **kw)
            case[est] = measure(L, dS, nopt, a); L.close()
            print("DQN %dx%d b%d, %3d options, %-8s eager step %.1f us; head_dqn %.1f us" % (hidden[0], hidden[1], B, nopt, est, case[est]["step_us"]["median"],
                                                                                        case[est]["launches_us"]["head_dqn"]["median"]), flush=True)
        res["cases"]["%dx%d-b%d-%d" % (hidden[0], hidden[1], B, nopt)] = case
        if hidden == (128, 128) and nopt in (128, 512):      # the per-sample-wavefront yardstick, measured in this call
            L = capi.create_discrete(api, VALUES[nopt], bounded=[0] * len(VALUES[nopt]), **kw)
            # (SMARTIES_HIP_NO_GRAPH is not needed: a timed call launches eagerly)
            m = measure(L, dS, nopt, a); L.close()
            res["racer_head_kernel"][str(nopt)] = m
            ratio = case["none"]["launches_us"]["head_dqn"]["median"] / m["launches_us"]["head_kernel"]["median"]
            res["ratio_head_dqn_none_to_head_kernel"][str(nopt)] = ratio
            print("RACER %3d options: head_kernel %.1f us; head_dqn (none) / head_kernel = %.2f" % (nopt, m["launches_us"]["head_kernel"]["median"], ratio), flush=True)
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
