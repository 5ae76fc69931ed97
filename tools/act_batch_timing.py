"""Wall-clock cost of acting with a recurrent net: hl_forward_sequence for one agent against hl_forward_sequences for n agents
(include/smarties_hip_act.h), on the shape of settings RACER_RNN (two LSTM layers of 32 cells, dimS 4, windows of 17 steps).

What is timed is the C call alone -- arguments and ctypes pointers are prepared before the clock starts --, since that is what an
environment-service thread waits for: the call returns when the outputs are in the caller's array (completion stamps polled
inside).  One process, the variants interleaved in rounds so that drift of the host hits all alike; per variant the median of
--calls calls (default 200) after --warmup calls.  A second pass with the library's timing taps on gives the device time of the
act_seq launch per n (HIP events around the launch).

    python tools/act_batch_timing.py [--calls 200] [--warmup 50] [--out profiles/act_batch_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch  # noqa: F401  (first, so that a single HIP runtime is resident in the process)
from smarties_amd import capi, load_hip
from oracle_api import fill_synth, synth_cfg

NS = (1, 16, 64, 256, 1024)
STEPS, DS = 17, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    api = load_hip()
    cfg = dict(dimS=DS, dimA=1, bounded=[1], hidden=(32, 32), nnFunc="Tanh", batchSize=128, maxTotObsNum=262144, randSeed=1, gamma=0.99,
               adv_kind=capi.ADV_GAUSSIAN, nn_type=capi.NN_LSTM, nnLambda=1e-6, explNoise=0.1, nnBPTTseq=16)
    L = capi.Learner(api, capi.make_config(**cfg)); L.init_weights()
    fill_synth(L, synth_cfg(seed=3, dimS=DS, dimA=1, lenMin=100, lenMax=300, pTerm=0.7), 50); L.initialize()
    L.step(10); L.sync()
    g = np.random.default_rng(0)
    pf, pd, pi = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    one_fn, many_fn = api.fn("forward_sequence"), api.fn("forward_sequences")
    st = g.standard_normal((max(NS) * STEPS, DS)).astype(np.float32)
    ns = np.full(max(NS), STEPS, np.int32)
    out = np.zeros((max(NS), L.nOut), np.float64)
    st_p, ns_p, out_p = st.ctypes.data_as(pf), ns.ctypes.data_as(pi), out.ctypes.data_as(pd)

    def call(n):      # n == 0: the single-agent entry point
        rc = one_fn(L.h, STEPS, st_p, out_p) if n == 0 else many_fn(L.h, n, ns_p, st_p, out_p)
        assert rc == 0, rc

    # the two entry points agree on what they compute (1e-5: the sums are formed in another order)
    call(0); ref = out[0].copy()
    call(max(NS)); assert np.abs(out[0] - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    variants = (0,) + NS
    for v in variants:
        for _ in range(a.warmup):
            call(v)
    times = {v: [] for v in variants}
    rounds = 10
    per = -(-a.calls // rounds)
    for _ in range(rounds):
        for v in variants:
            for _ in range(per):
                t0 = time.perf_counter(); call(v); times[v].append(time.perf_counter() - t0)
    us = {v: float(np.median(times[v]) * 1e6) for v in variants}
    p10 = {v: float(np.percentile(times[v], 10) * 1e6) for v in variants}
    p90 = {v: float(np.percentile(times[v], 90) * 1e6) for v in variants}
    # device time of the launch (taps on: events around every launch; the wall-clock numbers above were taken with them off)
    dev = {}
    for n in NS:
        L.timing_enable(True)
        for _ in range(50):
            call(n)
        ms, cnt = L.timing_get("act_seq")
        dev[n] = dict(launch_us=ms * 1e3, launches_per_call=cnt / 50.0)
        L.timing_enable(False)
    base = us[0]
    res = dict(shape="LSTM 2x32, dimS 4, 17-step windows", calls=len(times[0]), warmup=a.warmup, chunk=capi.ACT_SEQ_CHUNK,
               device=torch.cuda.get_device_name(0),
               forward_sequence_us=dict(median=base, p10=p10[0], p90=p90[0]),
               forward_sequences=[dict(n=n, median_us=us[n], p10_us=p10[n], p90_us=p90[n], per_agent_us=us[n] / n,
                                       ratio_to_single_call=us[n] / base, speedup_per_agent=base * n / us[n],
                                       kernel_us=dev[n]["launch_us"], launches_per_call=dev[n]["launches_per_call"]) for n in NS],
               bar="forward_sequences(64) <= 2 x forward_sequence", bar_ratio=us[64] / base, bar_met=bool(us[64] <= 2 * base))
    print("hl_forward_sequence, 1 agent:        %8.1f us  (p10 %.1f, p90 %.1f)" % (base, p10[0], p90[0]))
    for r in res["forward_sequences"]:
        print("hl_forward_sequences, %4d agents:   %8.1f us  (%.2f x the single call, %.2f us per agent, kernel %.1f us x %.0f)"
              % (r["n"], r["median_us"], r["ratio_to_single_call"], r["per_agent_us"], r["kernel_us"], r["launches_per_call"]))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
