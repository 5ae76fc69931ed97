"""What hl_rollout_step on a staging ring under the snapshot source (include/smarties_hip_rollout.h: hl_rollout_staging) buys and costs,
against the plain live rollout of the SAME build and process -- the live rollout is unchanged from the parent commit, so it is the
yardstick.  The nets and points of tools/rollout_timing.py:

    nets     lstm-2x32 (settings/RACER_RNN.json, dimS 6)      dense-2x256 (dimS 17, dimA 6)
    nEnv     64, 1024;  episodes end at random with probability 1/200 per step;  maxSteps 1000, a ring of 8000 rows

  1. idle      one call on a side stream with nothing queued on the learner, the two sources alternating call by call:
                 host_us    the call until it returns
                 device_us  between two HIP events recorded on the caller's stream around the call (the staged call's copy and
                            ingestion run behind what the caller's stream waits for)
               medians of --calls calls per source after --warmup, with the quartiles
  2. backlog   hl_step(STEPS) has just returned: microseconds until the caller's stream is synchronised behind one call; the sources
               alternate; median, minimum and maximum over --rounds rounds
  3. steps     microseconds per gradient step of hl_step(STEPS) .. hl_sync alone, and beside a host loop of staged calls back to back
               (call, synchronise the side stream, again) for the first 80 % of the time the steps take alone; the forms alternate
  4. launches  the library's event timers over 30 staged calls: rollout_stage_kernel beside ingest_dev_kernel for the same episodes

Each net runs in a child process of its own under its own time limit; nothing more is started on the device after a child that failed.
The child asks for 16 hardware queues if it is offered fewer (tools/act_snapshot_timing.py says why).

    python tools/rollout_snapshot_timing.py [--calls 200] [--warmup 50] [--rounds 7] [--steps 2000] [--out profiles/rollout_snapshot_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

if int(os.environ.get("GPU_MAX_HW_QUEUES") or 0) < 16:
    os.environ["GPU_MAX_HW_QUEUES"] = "16"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

NS = (64, 1024)
MAX_STEPS = 1000
RING_ROWS = 8 * MAX_STEPS
P_END = 1.0 / 200
TIMED_CALLS = 30
SOURCES = ("live", "snapshot")


def quart(vals):
    v = sorted(vals)
    return dict(median=v[len(v) // 2], p25=v[len(v) // 4], p75=v[(3 * len(v)) // 4])


def spread(vals):
    v = sorted(vals)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def child(name, calls, warmup, rounds, steps):
    import numpy as np
    import torch
    import rollout_timing
    from smarties_amd import capi, load_hip
    from oracle_api import fill_synth, synth_cfg
    api = load_hip()
    kw, sc = rollout_timing.nets()[name]
    kw = dict(kw, maxTotObsNum=1 << 23)
    side = torch.cuda.Stream()
    res = {}
    for n in NS:
        L = capi.Learner(api, capi.make_config(**kw)); L.init_weights()
        fill_synth(L, synth_cfg(**sc), 50); L.initialize(); L.step(10); L.sync()
        rng = np.random.default_rng(n)
        pool = [torch.from_numpy(rng.standard_normal((n, L.dS)).astype(np.float32)).cuda() for _ in range(8)]
        noise = [torch.from_numpy(np.clip(rng.standard_normal((n, L.dA)), -3, 3)).cuda() for _ in range(8)]
        rew = torch.from_numpy(rng.standard_normal(n)).cuda()
        out = torch.empty((n, L.dA), dtype=torch.float64, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        g = np.random.default_rng(11)
        n_flags = 4096
        f = (g.uniform(size=(n_flags, n)) < P_END).astype(np.int32) * (1 + (g.uniform(size=(n_flags, n)) < 0.5))
        end = torch.from_numpy(f.astype(np.int32)).cuda()
        rolls = dict(live=L.rollout(n, MAX_STEPS, seed=1), snapshot=L.rollout(n, MAX_STEPS, seed=2, staging_rows=RING_ROWS))
        count = dict(live=0, snapshot=0)
        torch.cuda.synchronize()
        L.policy_snapshot()

        def call(src):      # one call of the source's rollout on the side stream; every rollout sees the same inputs at its c-th call
            c = count[src]; count[src] += 1
            rolls[src].step(pool[c % 8], rew, end[c % n_flags], noise[c % 8], out=out, stream=side)

        # 1. idle
        t = {src: dict(host_us=[], device_us=[]) for src in SOURCES}
        for c in range(warmup + calls):
            for src in SOURCES:
                L.act_source(src)
                L.sync(); torch.cuda.synchronize()
                ev[0].record(side)
                t0 = time.perf_counter(); call(src); t1 = time.perf_counter()
                ev[1].record(side); ev[1].synchronize()
                if c >= warmup:
                    t[src]["host_us"].append((t1 - t0) * 1e6); t[src]["device_us"].append(ev[0].elapsed_time(ev[1]) * 1e3)
        us = dict(idle={src: {k: quart(v) for k, v in d.items()} for src, d in t.items()})
        # 2. behind a backlog of steps
        L.step(steps); L.sync(); side.synchronize()
        t = {src: [] for src in SOURCES}
        drain = {src: [] for src in SOURCES}
        for _ in range(rounds):
            for src in SOURCES:
                L.act_source(src)
                L.policy_snapshot()
                L.sync(); side.synchronize()
                L.step(steps)
                t0 = time.perf_counter()
                call(src)
                side.synchronize()
                t[src].append((time.perf_counter() - t0) * 1e6)
                L.sync()
                drain[src].append((time.perf_counter() - t0) * 1e6)
                L.scalars()      # raises on a device-side failure code
        us["backlog_us"] = {src: spread(v) for src, v in t.items()}
        us["backlog_drain_us"] = {src: spread(v) for src, v in drain.items()}
        # 3. the steps alone and beside staged calls
        L.act_source("snapshot")
        t = dict(alone=[], beside_staged_calls=[])
        k_calls, alone = [], None
        for r in range(rounds + 1):      # (round 0 sets the window of the loop and is not reported)
            for form in t:
                L.policy_snapshot()
                L.sync(); side.synchronize()
                t0 = time.perf_counter()
                L.step(steps)
                k = 0
                if form != "alone" and alone is not None:
                    while time.perf_counter() - t0 < 0.8 * alone:
                        call("snapshot"); side.synchronize(); k += 1
                L.sync()
                dt = time.perf_counter() - t0
                L.scalars()
                if form == "alone" and alone is None:
                    alone = dt
                if r > 0:
                    t[form].append(dt * 1e6 / steps)
                    if form != "alone":
                        k_calls.append(k)
            alone = sorted(t["alone"])[len(t["alone"]) // 2] * steps / 1e6 if t["alone"] else alone
        us["step_us"] = {k: spread(v) for k, v in t.items()}
        us["staged_calls_beside_the_steps"] = spread(k_calls)
        # 4. the copy beside the ingestion, from the library's event timers
        side.synchronize(); L.sync()
        before = rolls["snapshot"].stage_info()
        L.timing_enable(True)
        labels = ("rollout_stage_kernel", "ingest_dev_kernel")
        k0 = {k: L.timing_get(k) for k in labels}
        for _ in range(TIMED_CALLS):
            call("snapshot")
        side.synchronize(); L.sync(); torch.cuda.synchronize()
        k1 = {k: L.timing_get(k) for k in labels}
        L.timing_enable(False)
        after = rolls["snapshot"].stage_info()
        us["launch_us_per_call"] = {k: (k1[k][0] * k1[k][1] - k0[k][0] * k0[k][1]) * 1e3 / TIMED_CALLS for k in labels}
        us["launch_episodes_per_call"] = (after["episodes"] - before["episodes"]) / float(TIMED_CALLS)
        us["stage"] = after
        us["info"] = {src: rolls[src].info() for src in SOURCES}
        assert us["info"]["snapshot"]["episodes"] == after["episodes"]
        res[str(n)] = us
        L.close()
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--limit", type=int, default=240, help="seconds a net's child process may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.calls, a.warmup, a.rounds, a.steps)
    res = dict(calls=a.calls, warmup=a.warmup, rounds=a.rounds, steps=a.steps, max_steps=MAX_STEPS, ring_rows=RING_ROWS, p_end=P_END, nets={})
    for name in ("lstm-2x32", "dense-2x256"):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--calls", str(a.calls), "--warmup", str(a.warmup),
                            "--rounds", str(a.rounds), "--steps", str(a.steps)], stdout=subprocess.PIPE, text=True, timeout=a.limit)
        if p.returncode != 0:      # (nothing more is started on the device after a child that failed)
            sys.exit("%s: the child ended with status %d" % (name, p.returncode))
        res["nets"][name] = json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])
        for n, d in res["nets"][name].items():
            print("%-12s n=%5s  " % (name, n) + "   ".join(
                "%s host %.1f device %.1f backlog %.1f" % (s, d["idle"][s]["host_us"]["median"], d["idle"][s]["device_us"]["median"],
                                                           d["backlog_us"][s]["median"]) for s in SOURCES)
                  + "   step alone %.2f beside %.2f   stage %.1f ingest %.1f" % (
                      d["step_us"]["alone"]["median"], d["step_us"]["beside_staged_calls"]["median"],
                      d["launch_us_per_call"]["rollout_stage_kernel"], d["launch_us_per_call"]["ingest_dev_kernel"]), flush=True)
    res["staged_slower_than_live"] = [
        "%s n=%s %s" % (name, n, col) for name, d in res["nets"].items() for n, v in d.items() for col in ("host_us", "device_us", "backlog_us")
        if (v["backlog_us"]["snapshot"]["median"] > v["backlog_us"]["live"]["median"] if col == "backlog_us"
            else v["idle"]["snapshot"][col]["median"] > v["idle"]["live"][col]["median"])]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
