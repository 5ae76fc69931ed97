"""Cost of one simulator step through hl_rollout_step (include/smarties_hip_rollout.h) against the loop written by hand over
hl_select_actions_sequences_dev and hl_append_episodes_dev (tests/rollout.py: HandLoop -- slabs, lengths and terminal rows kept in torch,
the end flags brought to the host with .cpu()).  Those two calls are unchanged from the parent commit, so the hand loop IS the parent's way
of doing it.  Both are fed the same states, rewards, end flags and noise; episodes end at random with probability 1/200 per step.

    nets     lstm-2x32 (settings/RACER_RNN.json, dimS 6)      dense-2x256 (dimS 17, dimA 6)
    nEnv     64, 1024, 4096
    columns  rollout            hl_rollout_step with the caller's noise
             rollout_lib_noise  hl_rollout_step with the library's generator
             hand_loop          the loop over the existing calls
    per column   host_us    the call until it returns (both wait for the device inside: the rollout polls its bookkeeping stamp, the hand loop
                            copies the flags to the host)
                 device_us  between two HIP events recorded on the caller's stream around the call
    launches     per label of the library's event timers, the device time per rollout call (a run of its own with the timers on)

Every measurement is the median of --calls calls after --warmup calls.  Each net runs in a child process of its own under its own time limit;
nothing more is started on the device after a child that failed.

    python tools/rollout_timing.py [--calls 200] [--warmup 50] [--out profiles/rollout_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NS = (64, 1024, 4096)
MAX_STEPS = 1000
P_END = 1.0 / 200
LABELS = ("rollout_book_kernel", "rollout_noise_kernel", "act_seq_dev", "act_stack_dev", "act_forward_dev", "act_rows_dev", "act_head_kernel",
          "rollout_store_kernel", "ingest_dev_kernel")
TIMED_CALLS = 30


def nets():
    from smarties_amd import capi
    return {
        "lstm-2x32": (dict(dimS=6, dimA=2, bounded=[1, 0], hidden=(32, 32), nnFunc="Tanh", batchSize=128, maxTotObsNum=2097152, randSeed=1,
                           gamma=0.99, adv_kind=capi.ADV_GAUSSIAN, nn_type=capi.NN_LSTM, nnLambda=1e-6, explNoise=0.1, nnBPTTseq=16),
                      dict(seed=3, dimS=6, dimA=2, lenMin=100, lenMax=300, pTerm=0.7)),
        "dense-2x256": (dict(dimS=17, dimA=6, hidden=(256, 256), batchSize=256, maxTotObsNum=2097152, randSeed=1),
                        dict(seed=3, dimS=17, dimA=6, lenMin=100, lenMax=300, pTerm=0.7)),
    }


def child(name, calls, warmup):
    import numpy as np
    import torch
    import rollout as R
    from smarties_amd import capi, load_hip
    from oracle_api import fill_synth, synth_cfg
    api = load_hip()
    kw, sc = nets()[name]
    learners = []
    for _ in range(3):      # one learner per column: each replay takes in the same episodes
        L = capi.Learner(api, capi.make_config(**kw)); L.init_weights()
        fill_synth(L, synth_cfg(**sc), 50); L.initialize(); L.step(10); L.sync()
        learners.append(L)
    A, B, Cl = learners
    total = warmup + calls
    res = {}
    for n in NS:
        rng = np.random.default_rng(n)
        pool = [torch.from_numpy(rng.standard_normal((n, A.dS)).astype(np.float32)).cuda() for _ in range(8)]
        noise = [torch.from_numpy(np.clip(rng.standard_normal((n, A.dA)), -3, 3)).cuda() for _ in range(8)]
        rew = torch.from_numpy(rng.standard_normal(n)).cuda()
        out = torch.empty((n, A.dA), dtype=torch.float64, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def flags(seed, count):
            g = np.random.default_rng(seed)
            f = (g.uniform(size=(count, n)) < P_END).astype(np.int32) * (1 + (g.uniform(size=(count, n)) < 0.5))
            return torch.from_numpy(f.astype(np.int32)).cuda()

        def measure(step, seed):
            end = flags(seed, total)
            host, dev = [], []
            for c in range(total):
                torch.cuda.synchronize()
                ev[0].record()
                t0 = time.perf_counter(); step(pool[c % 8], rew, end[c], noise[c % 8]); t1 = time.perf_counter()
                ev[1].record(); ev[1].synchronize()
                if c >= warmup:
                    host.append((t1 - t0) * 1e6); dev.append(ev[0].elapsed_time(ev[1]) * 1e3)
            return dict(host_us=float(np.median(host)), device_us=float(np.median(dev)))

        roll, lib, hand = A.rollout(n, MAX_STEPS, seed=1), Cl.rollout(n, MAX_STEPS, seed=2), R.HandLoop(B, n, MAX_STEPS)
        us = dict(rollout=measure(lambda s, r, e, z: roll.step(s, r, e, z, out=out), 11),
                  rollout_lib_noise=measure(lambda s, r, e, z: lib.step(s, r, e, out=out), 11),
                  hand_loop=measure(lambda s, r, e, z: hand.step(s, r, e, z), 11))
        info = roll.info()
        assert info["episodes"] == hand.k and info["capped"] == hand.capped, (info, hand.k, hand.capped)      # the two did the same work
        us["episodes_per_call"] = info["episodes"] / float(info["calls"])
        us["no_room"] = info["no_room"]
        # the launches of a rollout call, from the library's event timers
        Cl.timing_enable(True)
        k0 = {k: Cl.timing_get(k) for k in LABELS}
        end = flags(12, TIMED_CALLS)
        for c in range(TIMED_CALLS):
            lib.step(pool[c % 8], rew, end[c], out=out)
        torch.cuda.synchronize()
        k1 = {k: Cl.timing_get(k) for k in LABELS}
        Cl.timing_enable(False)
        us["launch_us_per_call"] = {k: (k1[k][0] * k1[k][1] - k0[k][0] * k0[k][1]) * 1e3 / TIMED_CALLS for k in LABELS if k1[k][1] > k0[k][1]}
        res[str(n)] = us
        roll.close(); lib.close(); del hand
        torch.cuda.empty_cache()
    for L in learners:
        L.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--limit", type=int, default=240, help="seconds a net's child process may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.calls, a.warmup)
    res = dict(calls=a.calls, warmup=a.warmup, max_steps=MAX_STEPS, p_end=P_END, nets={})
    for name in nets():
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--calls", str(a.calls), "--warmup", str(a.warmup)],
                           stdout=subprocess.PIPE, text=True, timeout=a.limit)
        if p.returncode != 0:      # (nothing more is started on the device after a child that failed)
            sys.exit("%s: the child ended with status %d" % (name, p.returncode))
        res["nets"][name] = json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])
        for n, d in res["nets"][name].items():
            print("%-12s n=%5s  " % (name, n) + "   ".join("%s host %.1f device %.1f" % (k, d[k]["host_us"], d[k]["device_us"])
                                                             for k in ("rollout", "rollout_lib_noise", "hand_loop")), flush=True)
    res["rollout_slower_than_hand_loop"] = [
        "%s n=%s %s" % (name, n, col) for name, d in res["nets"].items() for n, v in d.items() for col in ("host_us", "device_us")
        if v["rollout"][col] > v["hand_loop"][col]]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
