"""What acting on a policy snapshot (include/smarties_hip_dev.h: hl_policy_snapshot, hl_act_dev_source) buys and costs, against the live
source of the SAME build -- the live source is unchanged from the parent commit, so it is the yardstick -- on two nets:

  cfg-NS   dimS 17, dimA 6, SoftSign 2 x 256, batchSize 256; hl_select_actions_dev, 64 agents for the latencies
  atari    the stack of settings/RACER_atari.json (84 x 84 frames, nAppendedObs 3, conv 8 / 16 / 32 / 64, dense 64, 6 options), batchSize 128;
           hl_select_actions_sequences_dev on a [4][n][7056] buffer, 256 agents for the latencies

  1. latency        one acting call on a side stream until that stream is synchronised (host clock), live and snapshot alternating:
                      idle     the learner has nothing queued
                      backlog  hl_step(STEPS) has just returned; `drain` is the same clock at the return of hl_sync
  2. interference   microseconds per step of hl_step(STEPS) .. hl_sync alone, and with a host loop that issues snapshot acting calls of 64 and
                    of 1024 agents back to back (call, synchronise the side stream, again) for the first 80 % of the time the steps take alone;
                    the three forms alternate.  hl_get_scalars after every round: a device-side failure code ends the run.
  3. snapshot cost  the library's event timer around policy_snapshot_kernel (label policy_snapshot), average of 20 launches

Method: ONE process; every phase runs under a time limit of its own (a watchdog ends the process; nothing more is started on the device);
every shape and both sources are warmed up before anything is timed; reported are the median and the spread (min, max) over the rounds.
The process asks for 16 hardware queues before the runtime starts if it is offered fewer: the learner's stream, its sampler's stream, the
acting stream and the caller's streams each want one -- two streams that share a queue run one after the other, whatever the events say.

    python tools/act_snapshot_timing.py [--rounds 7] [--steps 2000] [--out profiles/act_snapshot_timing.json]
"""
import argparse
import faulthandler
import json
import os
import sys
import time

if int(os.environ.get("GPU_MAX_HW_QUEUES") or 0) < 16:
    os.environ["GPU_MAX_HW_QUEUES"] = "16"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

DS_ATARI, NAPP, WIN = 7056, 3, 4
INTERFERE_NS = (64, 1024)


class Phase:
    """a time limit of its own for a stretch of device work: the process ends when it runs out"""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        print("phase %s (limit %d s)" % (self.name, self.seconds), flush=True)
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()
        return False


def stat(vals):
    v = sorted(vals)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def measure(name, L, make_act, n_latency, rounds, steps):
    """make_act(n) -> a callable that enqueues one acting call for n agents on the side stream"""
    import torch
    side = torch.cuda.Stream()
    acts = {n: make_act(n, side) for n in sorted({n_latency} | set(INTERFERE_NS))}
    res = dict(agents=n_latency, steps=steps)

    def complete(n):      # one acting call, until the side stream is done: seconds
        t0 = time.perf_counter()
        acts[n]()
        side.synchronize()
        return time.perf_counter() - t0

    with Phase(name + ": warm-up", 240):
        L.step(10); L.policy_snapshot()
        for src in ("live", "snapshot"):
            L.act_source(src)
            for n in acts:
                for _ in range(3):
                    complete(n)
        L.step(steps); L.sync()
        L.scalars()

    with Phase(name + ": idle latency", 120):
        t = dict(live=[], snapshot=[])
        for _ in range(20 * rounds):
            for src in t:
                L.act_source(src)
                t[src].append(complete(n_latency) * 1e6)
        res["idle_us"] = {k: stat(v) for k, v in t.items()}

    with Phase(name + ": latency behind %d steps" % steps, 400):
        t = {src: dict(act=[], drain=[], enqueue=[]) for src in ("live", "snapshot")}
        for _ in range(rounds):
            for src in t:
                L.act_source(src)
                L.policy_snapshot()                    # (both sources pay it: the loop it belongs to takes one per call of hl_step)
                t0 = time.perf_counter()
                L.step(steps)
                t[src]["enqueue"].append((time.perf_counter() - t0) * 1e6)
                t[src]["act"].append(complete(n_latency) * 1e6)
                L.sync()
                t[src]["drain"].append((time.perf_counter() - t0) * 1e6)
                L.scalars()
        res["backlog_us"] = {src: {k: stat(v) for k, v in d.items()} for src, d in t.items()}

    with Phase(name + ": interference", 600):
        L.act_source("snapshot")
        t = {"alone": [], "64": [], "1024": []}
        calls = {"64": [], "1024": []}
        alone = None
        for r in range(rounds + 1):                    # (round 0 sets the window of the acting loops and is not reported)
            for form in t:
                L.policy_snapshot()
                L.sync()
                t0 = time.perf_counter()
                L.step(steps)
                k = 0
                if form != "alone" and alone is not None:
                    while time.perf_counter() - t0 < 0.8 * alone:
                        complete(int(form)); k += 1
                L.sync()
                dt = time.perf_counter() - t0
                L.scalars()                            # raises on a device-side failure code
                if form == "alone" and alone is None:
                    alone = dt
                if r > 0:
                    t[form].append(dt * 1e6 / steps)
                    if form != "alone":
                        calls[form].append(k)
            alone = sorted(t["alone"])[len(t["alone"]) // 2] * steps / 1e6 if t["alone"] else alone
        res["interference_us_per_step"] = {k: stat(v) for k, v in t.items()}
        res["interference_acting_calls"] = {k: stat(v) for k, v in calls.items()}
        res["device_failure_code"] = False

    with Phase(name + ": snapshot cost", 60):
        L.sync()
        L.timing_enable(True)
        for _ in range(20):
            L.policy_snapshot()
        ms, cnt = L.timing_get("policy_snapshot")
        L.timing_enable(False)
        assert cnt == 20, cnt
        res["policy_snapshot_us"] = ms * 1e3
        res["policy_snapshot_bytes"] = 4 * (L.nParams + 2 * L.dS)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--nets", default="cfg-NS,atari")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.rounds >= 5, "medians of at least five rounds"
    import numpy as np
    import torch
    from smarties_amd import capi, load_hip
    from oracle_api import fill_synth, synth_cfg
    api = load_hip()
    rng = np.random.default_rng(0)
    out = dict(rounds=a.rounds, steps=a.steps, hw_queues=int(os.environ["GPU_MAX_HW_QUEUES"]), nets={})

    if "cfg-NS" in a.nets.split(","):
        cfg = dict(dimS=17, dimA=6, hidden=(256, 256), nnFunc="SoftSign", batchSize=256, maxTotObsNum=1 << 19, randSeed=1)
        L = capi.Learner(api, capi.make_config(**cfg)); L.init_weights()
        fill_synth(L, synth_cfg(seed=3, dimS=17, dimA=6, lenMin=100, lenMax=300, pTerm=0.7), 50); L.initialize()

        def rows(n, side):
            st = torch.from_numpy(rng.standard_normal((n, L.dIn)).astype(np.float32)).cuda()
            noise = torch.from_numpy(np.clip(rng.standard_normal((n, L.dA)), -2, 2)).cuda()
            sel = (torch.empty((n, L.dA), dtype=torch.float64, device="cuda"), torch.empty((n, L.polDim), dtype=torch.float64, device="cuda"),
                   torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda"))
            torch.cuda.synchronize()
            return lambda: L.select_actions_dev(st, noise, out=sel, stream=side)

        out["nets"]["cfg-NS"] = dict(net="dimS 17, dimA 6, SoftSign 2x256, batchSize 256; hl_select_actions_dev", **measure("cfg-NS", L, rows, 64, a.rounds, a.steps))
        L.close()

    if "atari" in a.nets.split(","):
        cfg = dict(dimS=DS_ATARI, dimA=1, bounded=[0], adv_kind=capi.ADV_DISCRETE, n_options=6, nAppendedObs=NAPP, hidden=(64,), nnFunc="SoftSign",
                   batchSize=128, conv=[(84, 84, 4, 8, 8, 4), (20, 20, 8, 16, 6, 2), (8, 8, 16, 32, 4, 1), (5, 5, 32, 64, 3, 1)],
                   maxTotObsNum=2048, randSeed=1)
        L = capi.Learner(api, capi.make_config(**cfg)); L.init_weights()
        fill_synth(L, synth_cfg(seed=3, dimS=DS_ATARI, dimA=1, lenMin=20, lenMax=40, pTerm=0.5), 40); L.initialize()

        def windows(n, side):      # one frame per step in a [4][n][7056] buffer, agent e is column e
            buf = torch.from_numpy(rng.standard_normal((WIN, n, DS_ATARI), dtype=np.float32)).cuda()
            first = torch.arange(n, dtype=torch.int64, device="cuda")
            n_steps = torch.full((n,), WIN, dtype=torch.int32, device="cuda")
            noise = torch.from_numpy(rng.random(n)).cuda()
            sel = (torch.empty((n, L.dA), dtype=torch.float64, device="cuda"), torch.empty((n, L.polDim), dtype=torch.float64, device="cuda"),
                   torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda"))
            torch.cuda.synchronize()
            return lambda: L.select_actions_sequences_dev(buf, first, n_steps, n, noise, out=sel, stream=side)

        out["nets"]["atari"] = dict(net="RACER_atari.json: 84x84x(1+3), conv 8/16/32/64, dense 64, 6 options, batchSize 128; hl_select_actions_sequences_dev",
                                    **measure("atari", L, windows, 256, a.rounds, a.steps))
        L.close()

    for name, d in out["nets"].items():
        print(name)
        for k in ("idle_us", "backlog_us", "interference_us_per_step", "interference_acting_calls", "policy_snapshot_us"):
            print("  %-28s %s" % (k, json.dumps(d[k])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
