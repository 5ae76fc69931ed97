#!/usr/bin/env python3
"""Device time of the PPO head launch (headppo.hip: ppo_head_kernel), of ppo_adam, of the critic's launches and of the eager PPO step,
with cfg-NS's net: dense (256, 256), dimS 17.

  launches_us  hl_timing_get: events around the launches of eager steps, --per steps per round, median over --rounds (least, largest)
  step_us      host clock around hl_step + hl_sync, per step, median over --rounds (least, largest)
Cases: 6 continuous dimensions (batch 256); 128 and 512 options (batch 128).  Beside the discrete ones, from the same call: a DQN learner of
the same shape (returnsEstimator "GAE": one row set), whose head_dqn is the project's own point of comparison for an output layer + fp64
head + backward on 16 rows per workgroup.
A PPO learner steps nEpochs x nHorizon / batch times and is empty then: the horizon is --per batches, one epoch, refilled per round.
--bench-parent <tree>: also runs bench.py of this tree and of <tree> (a checkout of the parent commit with its library built) in turn,
--bench-rounds times each, and records every value.

  python tools/ppo_timing.py --out profiles/ppo_timing.json [--bench-parent <tree>]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("step_tail_kernel", "gemm16_fwd0", "gemm16_fwd1", "ppo_critic_fwd", "head_ppo", "head_dqn", "ppo_critic_dx", "ppo_critic_dw", "gemm16_dx1", "gemm16_dw",
         "ppo_adam", "dqn_adam_target", "post_kernel")
DS, HIDDEN, N = 17, (256, 256), 65


def bench(tree, steps, warmup):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                         capture_output=True, text=True, check=True).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["ms_per_step"] * 1e3


def fill(L, rng, dA, nOpt, steps, tag0):
    """episodes of N states until `steps` transitions are stored"""
    for e in range(steps // (N - 1)):
        if nOpt:
            mu = rng.random(size=(N, nOpt)) + 0.5; mu /= mu.sum(1, keepdims=True); act = rng.integers(0, nOpt, size=(N, 1)) + 0.5
        else:
            mu = np.concatenate([0.1 * rng.normal(size=(N, dA)), np.full((N, dA), 0.4472135955)], 1); act = mu[:, :dA] + 0.3 * rng.normal(size=(N, dA))
        L.append_episode(rng.normal(size=(N, DS)).astype(np.float32), act, mu, rng.normal(size=N), (0.5 * rng.normal(size=N)).astype(np.float32), e % 2, tag0 + e)


def measure(L, a, dA, nOpt, B, ppo):
    rng = np.random.default_rng(5)
    L.init_weights()
    horizon = a.per * B
    fill(L, rng, dA, nOpt, horizon, 0)
    L.initialize()
    mm = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    wall, timed = [], {k: [] for k in NAMES}
    def round_(k):      # one pass over the horizon; a PPO learner is empty behind it
        if ppo and L.counts()[0] == 0:
            fill(L, rng, dA, nOpt, horizon, 1000 * (k + 1))
        t0 = time.perf_counter(); L.step(a.per - 1); L.sync(); return (time.perf_counter() - t0) * 1e6 / (a.per - 1)      # (the last step of a horizon carries the statistics and the clear)
    round_(-1); L.step(1); L.sync()      # warm-up: every launch of the step has run
    for r in range(a.rounds):
        wall.append(round_(r)); L.step(1); L.sync()
    for r in range(a.rounds):      # (the timers synchronise around every launch: a run of their own)
        L.timing_enable(True); round_(a.rounds + r)
        for k in NAMES:
            ms, cnt = L.timing_get(k)
            timed[k].append(ms * 1e3 * cnt / (a.per - 1))
        L.timing_enable(False); L.step(1); L.sync()
    return dict(batch=B, step_us=mm(wall), launches_us={k: mm(v) for k, v in timed.items() if max(v) > 0})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--per", type=int, default=64)
    ap.add_argument("--bench-parent", default="")
    ap.add_argument("--bench-rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch  # (first, so that a single HIP runtime is resident in the process)
    torch.cuda.set_device(0)
    from smarties_amd import capi, load_hip
    api = load_hip()
    res = dict(command=" ".join(["python"] + sys.argv), rounds=a.rounds, per=a.per, dimS=DS, hidden=list(HIDDEN))
    for name, dA, nOpt, B in (("continuous6", 6, 0, 256), ("options128", 1, 128, 128), ("options512", 1, 512, 128)):
        kw = dict(dimS=DS, hidden=HIDDEN, batchSize=B, randSeed=43, device_id=0, returnsEstimator="GAE")
        L = capi.create_ppo(api, 0.01, 1, (nOpt,) if nOpt else None, maxTotObsNum=a.per * B, clipImpWeight=0.2, **(kw if nOpt else dict(kw, dimA=dA, bounded=[0] * dA)))
        res["ppo_" + name] = measure(L, a, dA, nOpt, B, True); L.close()
        line = "%s: PPO eager step %.1f us, head_ppo %.1f us, ppo_adam %.1f us" % (name, res["ppo_" + name]["step_us"]["median"],
               res["ppo_" + name]["launches_us"]["head_ppo"]["median"], res["ppo_" + name]["launches_us"]["ppo_adam"]["median"])
        if nOpt:
            L = capi.create_dqn(api, 0.01, (nOpt,), maxTotObsNum=100000, **kw)
            res["dqn_" + name] = measure(L, a, dA, nOpt, B, False); L.close()
            line += "; DQN head_dqn %.1f us" % res["dqn_" + name]["launches_us"]["head_dqn"]["median"]
        print(line, flush=True)
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
