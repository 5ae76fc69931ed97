#!/usr/bin/env python3
"""Device time of the discrete head at 18, 64, 128 and 512 options: batch 128, dense (128, 128), dimS 24.

Two figures per case, both medians over --rounds measurements with the least and the largest beside them:
  launch_with_head_us  hl_timing_get: events around the launches of eager training steps, --per steps per round; the launch that holds the
                       head of this net's step -- the wide fused kernel up to 32 options (fused_wide), the step chain up to 64 (step_chain),
                       beyond 64 the head launch (head_kernel: headw.hip's head_wide_kernel with the sampler's rider) -- and every other
                       timed launch of the step in launches_us
  head_launch_us       hl_kernel_profile(3): launchHead alone, without riders (head.hip's head_kernel_t up to 64 options, head_wide_kernel
                       beyond), captured --per times into a graph that is replayed 20 times between two events; step_us: the replayed step (7)
--root <tree> measures another checkout of the library (a parent commit: 18 and 64 options only, through hl_create).

  python tools/discrete_wide_timing.py --out profiles/discrete_wide_timing.json [--root <tree>] [--options 18 64]
"""
import argparse
import json
import os
import sys

import numpy as np

NAMES = ("step_tail_kernel", "fused_wide", "step_chain", "fwd_chain", "head_kernel", "gemm16_dx1", "dw_table_kernel", "post_kernel")
VALUES = {18: (18,), 64: (64,), 128: (128,), 512: (8, 8, 8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--options", type=int, nargs="+", default=[18, 64, 128, 512])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--per", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch  # (first, so that a single HIP runtime is resident in the process)
    torch.cuda.set_device(0)
    from smarties_amd import capi, load_hip
    api = load_hip()
    res = dict(command=" ".join(["python"] + sys.argv), batch=128, hidden=[128, 128], dimS=24, rounds=a.rounds, per=a.per, cases={})
    for nopt in a.options:
        values = VALUES[nopt]
        kw = dict(dimS=24, hidden=(128, 128), batchSize=128, maxTotObsNum=20000, randSeed=43, device_id=0)
        if len(values) == 1 and nopt <= 64:
            L = capi.Learner(api, capi.make_config(dimA=1, bounded=[0], adv_kind=capi.ADV_DISCRETE, n_options=nopt, **kw))
        else:
            L = capi.create_discrete(api, values, bounded=[0] * len(values), **kw)
        L.init_weights()
        rng = np.random.default_rng(nopt)
        shifts = np.concatenate([[1], np.cumprod(values)[:-1]])
        for e in range(40):
            n = 60
            mu = rng.uniform(0.5, 1.5, size=(n, nopt)); mu /= mu.sum(1, keepdims=True)
            lab = rng.integers(0, nopt, size=n)
            act = (lab[:, None] // shifts[None, :]) % np.asarray(values)[None, :] + 0.1
            act[-1] = 0.0; mu[-1] = 0.0
            R = rng.normal(size=n); R[0] = 0.0
            L.append_episode(rng.normal(size=(n, 24)).astype(np.float32), act, mu, R, (0.5 * rng.normal(size=n)).astype(np.float32), 0, e)
        L.initialize()
        L.step(4); L.sync()      # warm-up; the buffers then hold a minibatch and its forward pass
        head = [L.kernel_profile(3, a.per) for _ in range(a.rounds)]
        step = [L.kernel_profile(7, a.per) for _ in range(a.rounds)]
        timed = {k: [] for k in NAMES}
        for r in range(a.rounds):
            L.timing_enable(True); L.step(a.per + r); L.sync()      # (a call's length differs from the last one's: no graph is prepared for it)
            for k in NAMES:
                ms, cnt = L.timing_get(k)
                timed[k].append(ms * 1e3 * cnt / (a.per + r))
            L.timing_enable(False)
        us = {k: float(np.median(v)) for k, v in timed.items() if max(v) > 0}
        holder = [k for k in ("head_kernel", "step_chain", "fused_wide") if k in us][0]
        res["cases"][str(nopt)] = dict(values=list(values), launch_with_head=holder, launch_with_head_us=us[holder],
                                       launch_with_head_us_min_max=[min(timed[holder]), max(timed[holder])], launches_us=us,
                                       head_launch_us=float(np.median(head)), head_launch_us_min_max=[min(head), max(head)],
                                       step_us=float(np.median(step)), step_us_min_max=[min(step), max(step)])
        print("options %4d: %-11s %8.2f us (%.2f .. %.2f) timed in eager steps; head launch alone %8.2f us (%.2f .. %.2f); replayed step %8.2f us"
              % (nopt, holder, us[holder], min(timed[holder]), max(timed[holder]), np.median(head), min(head), max(head), np.median(step)), flush=True)
        L.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
