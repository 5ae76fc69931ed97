"""Wall-clock cost of acting and episode ingestion from device memory (include/smarties_hip_dev.h) against the host-pointer calls of the
SAME build -- hl_forward and hl_append_episode are unchanged from the parent commit, so they are the baseline -- on the cfg-NS net
(dimS 17, dimA 6, SoftSign 2x256, batchSize 256):

  forward   n = 1024 and 16384 rows, the calls interleaved one after the other in the same process:
              host              hl_forward on rows in host memory, outputs in host memory (the bare C call)
              host_from_tensor  what a simulator on the GPU pays for that call: states.cpu(), hl_forward, the outputs back onto the device
              dev_enqueue       hl_forward_dev until it returns (it waits for nothing)
              dev_complete      hl_forward_dev and a synchronisation of the caller's stream: the outputs are there
              select_complete   hl_select_actions_dev (forward pass + the fp64 head kernel) and the same synchronisation; the host
                                route has no twin in this library's C-ABI (the head runs per agent in the caller's host code)
  ingest    64 episodes of 200 steps, two learners filled side by side:
              host_calls / dev_call          64 hl_append_episode calls on host arrays / ONE hl_append_episodes_dev call on a
                                             [200][64] rollout buffer (row_stride 64), until they return
              host_complete / dev_complete   the same followed by hl_get_episode_stats(0), which hands everything queued to the device
                                             (the host route's ingest launch, the table, the Retrace sweep of the new episodes) and waits

Method: every round is a child process of its own (a fresh HIP context); inside a child a measurement is the median of --calls calls
after --warmup calls, host and device calls alternating.  Reported: the median over the rounds' medians and their spread (min, max).

    python tools/act_dev_timing.py [--rounds 5] [--calls 100] [--out profiles/act_dev_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NS = (1024, 16384)
N_EP, EP_LEN = 64, 200
CFG = dict(dimS=17, dimA=6, hidden=(256, 256), nnFunc="SoftSign", batchSize=256, maxTotObsNum=1 << 19, randSeed=1)


def child(calls, warmup, ingest_calls):
    import numpy as np
    import torch
    from smarties_amd import capi, load_hip
    from oracle_api import fill_synth, synth_cfg
    api = load_hip()

    def learner():
        L = capi.Learner(api, capi.make_config(**CFG)); L.init_weights()
        fill_synth(L, synth_cfg(seed=3, dimS=CFG["dimS"], dimA=CFG["dimA"], lenMin=100, lenMax=300, pTerm=0.7), 50); L.initialize()
        L.step(10); L.sync()
        return L

    def median_us(fns):
        """fns: {name: callable}; the callables alternate, each timed on its own"""
        for _ in range(warmup):
            for f in fns.values():
                f()
        t = {k: [] for k in fns}
        for _ in range(calls):
            for k, f in fns.items():
                t0 = time.perf_counter(); f(); t[k].append(time.perf_counter() - t0)
        return {k: float(np.median(v) * 1e6) for k, v in t.items()}

    res = dict(forward_us={}, ingest_us={})
    L = learner()
    rng = np.random.default_rng(0)
    stream = torch.cuda.current_stream()
    for n in NS:
        st = rng.standard_normal((n, L.dIn)).astype(np.float32)
        st_d = torch.from_numpy(st).cuda()
        noise_d = torch.from_numpy(np.clip(rng.standard_normal((n, L.dA)), -2, 2)).cuda()
        out_d = torch.empty((n, L.nOut), dtype=torch.float64, device="cuda")
        sel = (torch.empty((n, L.dA), dtype=torch.float64, device="cuda"), torch.empty((n, L.polDim), dtype=torch.float64, device="cuda"),
               torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()

        def host_from_tensor():
            o = L.forward(st_d.cpu().numpy())
            torch.from_numpy(o).cuda()
            stream.synchronize()

        def dev_complete():
            L.forward_dev(st_d, out=out_d); stream.synchronize()

        def select_complete():
            L.select_actions_dev(st_d, noise_d, out=sel); stream.synchronize()

        us = median_us(dict(host=lambda: L.forward(st), host_from_tensor=host_from_tensor, dev_complete=dev_complete,
                            select_complete=select_complete))
        # (the enqueue alone is timed apart, with a synchronisation OUTSIDE the bracket so that the queue does not grow)
        t = []
        for _ in range(calls):
            t0 = time.perf_counter(); L.forward_dev(st_d, out=out_d); t.append(time.perf_counter() - t0)
            stream.synchronize()
        us["dev_enqueue"] = float(np.median(t) * 1e6)
        res["forward_us"][str(n)] = us
    L.close()

    # ingestion: two learners filled side by side with the same episodes
    LH, LD = learner(), learner()
    S = rng.standard_normal((EP_LEN, N_EP, LH.dS)).astype(np.float32); A = rng.standard_normal((EP_LEN, N_EP, LH.dA))
    MU = np.abs(rng.standard_normal((EP_LEN, N_EP, LH.polDim))) + 0.1; R = rng.standard_normal((EP_LEN, N_EP))
    V = rng.standard_normal((EP_LEN, N_EP)).astype(np.float32); ADV = rng.standard_normal((EP_LEN, N_EP)).astype(np.float32)
    host_eps = [tuple(np.ascontiguousarray(x[:, e]) for x in (S, A, MU, R, V, ADV)) for e in range(N_EP)]      # an episode's arrays, contiguous
    dev = [torch.from_numpy(x).cuda() for x in (S, A, MU, R, V, ADV)]
    torch.cuda.synchronize()
    nsteps, term, first = [EP_LEN] * N_EP, [0] * N_EP, list(range(N_EP))
    tag = [0]

    def host_append():
        for e, (s, a, mu, r, v, adv) in enumerate(host_eps):
            LH.append_episode(s, a, mu, r, v, 0, tag[0] + e, advantages=adv)

    def dev_append():
        LD.append_episodes_dev(nsteps, term, [tag[0] + e for e in range(N_EP)], first, N_EP, *dev)

    t = dict(host_calls=[], host_complete=[], dev_call=[], dev_complete=[])
    for i in range(2 + ingest_calls):
        tag[0] += N_EP
        t0 = time.perf_counter(); host_append(); t1 = time.perf_counter(); LH.episode_stats(0); t2 = time.perf_counter()
        t3 = time.perf_counter(); dev_append(); t4 = time.perf_counter(); LD.episode_stats(0); t5 = time.perf_counter()
        if i >= 2:
            t["host_calls"].append(t1 - t0); t["host_complete"].append(t2 - t0); t["dev_call"].append(t4 - t3); t["dev_complete"].append(t5 - t3)
    res["ingest_us"] = {k: float(np.median(v) * 1e6) for k, v in t.items()}
    LH.close(); LD.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ingest-calls", type=int, default=15)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.calls, a.warmup, a.ingest_calls)
    assert a.rounds >= 5, "medians of at least five runs"
    runs = []
    for r in range(a.rounds):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--warmup", str(a.warmup),
                            "--ingest-calls", str(a.ingest_calls)], stdout=subprocess.PIPE, text=True, timeout=300)
        if p.returncode != 0:      # (nothing more is started on the device after a child that failed)
            sys.exit("round %d: the child ended with status %d" % (r, p.returncode))
        runs.append(json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:]))
        print("round %d done" % r, flush=True)

    def stat(vals):
        v = sorted(vals)
        return dict(median=v[len(v) // 2], min=v[0], max=v[-1])

    res = dict(net="dimS 17, dimA 6, SoftSign 2x256, batchSize 256", rounds=a.rounds, calls=a.calls, warmup=a.warmup, ingest_calls=a.ingest_calls,
               episodes=N_EP, episode_steps=EP_LEN, forward_us={}, ingest_us={})
    for n in NS:
        res["forward_us"][str(n)] = {k: stat([x["forward_us"][str(n)][k] for x in runs]) for k in runs[0]["forward_us"][str(n)]}
    res["ingest_us"] = {k: stat([x["ingest_us"][k] for x in runs]) for k in runs[0]["ingest_us"]}
    for n, d in res["forward_us"].items():
        print("forward n=%6s  " % n + "   ".join("%s %.1f (%.1f .. %.1f)" % (k, v["median"], v["min"], v["max"]) for k, v in d.items()))
    print("ingest %d x %d  " % (N_EP, EP_LEN) + "   ".join("%s %.1f (%.1f .. %.1f)" % (k, v["median"], v["min"], v["max"]) for k, v in res["ingest_us"].items()))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
