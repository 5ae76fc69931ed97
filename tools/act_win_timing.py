"""Wall-clock cost of acting with the recurrent nets whose many-agent call is a chain of hl_forward_sequence's own window launches
(include/smarties_hip_act.h; smarties_amd/csrc/learner_act.h: actWinChain): hl_forward_sequence for one agent against
hl_forward_sequences for n agents, on two shapes --

  pomdp      the partially observable cart-pole of apps/cart_pole_many: dimS 6, one bounded action, an RNN encoder layer of 128 cells
             under two MGU layers of 128, windows of 17 steps, batchSize 128 (a chunk holds min(batchSize, HL_ACT_SEQ_CHUNK) = 128 agents)
  conv_lstm  the shape of tests/golden/conv_lstm.bin: two convolutions on 1 + 3 stacked 8 x 8 x 4 frames, an LSTM layer of 32 cells, four
             options, windows of 5 steps behind 3 context states, batchSize 16 (chunks of 16 agents)

Method as tools/act_tm_timing.py: what is timed is the C call alone -- arguments and ctypes pointers are prepared before the clock
starts --; one process, the variants interleaved in rounds so that drift of the host hits all alike; per variant the median of --calls
calls (default 200) after --warmup calls.  A second pass with the library's timing taps on gives the device time of a chunk's whole
chain ("act_win_chain": HIP events around the front, the window launches and the output launch) per n.  The yardstick is the
single-agent call of the same build: n times it is what the loop over the agents cost, which this call was before the chain.

    python tools/act_win_timing.py [--calls 200] [--warmup 50] [--out profiles/act_win_timing.json]
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

NS = (1, 4, 16, 64, 256)
SHAPES = {  # name: (description, configuration, states per window, episodes' lengths)
    "pomdp": ("RNN 128 encoder under MGU 2x128, dimS 6, dimA 1, 17-step windows, batchSize 128",
              dict(dimS=6, dimA=1, bounded=[1], hidden=(128, 128), encoder=[128], encoder_rnn=1, nnFunc="Tanh", batchSize=128,
                   maxTotObsNum=262144, randSeed=1, gamma=0.99, adv_kind=capi.ADV_GAUSSIAN, nn_type=capi.NN_MGU, nnLambda=1e-6, explNoise=0.1,
                   nnBPTTseq=16), 17, (100, 300)),
    "conv_lstm": ("conv 8x8x16 -> 32 k4, -> 64 k3, LSTM 32, dimS 256 (1 + 3 stacked), 4 options, 5-step windows + 3 context states, batchSize 16",
                  dict(dimS=256, dimA=1, adv_kind=capi.ADV_DISCRETE, n_options=4, nAppendedObs=3, conv=[(8, 8, 16, 32, 4, 1), (5, 5, 32, 64, 3, 1)],
                       hidden=(32,), nnFunc="Tanh", batchSize=16, maxTotObsNum=2000, randSeed=3, nn_type=capi.NN_LSTM, nnBPTTseq=4), 8, (10, 40)),
}


def measure(api, name, calls, warmup):
    what, cfg, steps, (len_min, len_max) = SHAPES[name]
    dS, batch = cfg["dimS"], cfg["batchSize"]
    L = capi.Learner(api, capi.make_config(**cfg)); L.init_weights()
    fill_synth(L, synth_cfg(seed=3, dimS=dS, dimA=cfg["dimA"], lenMin=len_min, lenMax=len_max, pTerm=0.7), 50); L.initialize()
    L.step(10); L.sync()
    g = np.random.default_rng(0)
    pf, pd, pi = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    one_fn, many_fn = api.fn("forward_sequence"), api.fn("forward_sequences")
    st = g.standard_normal((max(NS) * steps, dS)).astype(np.float32)
    ns = np.full(max(NS), steps, np.int32)
    out = np.zeros((max(NS), L.nOut), np.float64)
    st_p, ns_p, out_p = st.ctypes.data_as(pf), ns.ctypes.data_as(pi), out.ctypes.data_as(pd)

    def call(n):      # n == 0: the single-agent entry point
        rc = one_fn(L.h, steps, st_p, out_p) if n == 0 else many_fn(L.h, n, ns_p, st_p, out_p)
        assert rc == 0, rc

    # the two entry points give the same bits (the same kernels, the agent as one of the workgroups)
    call(0); ref = out[0].copy()
    call(max(NS)); assert np.array_equal(out[0], ref)
    variants = (0,) + NS
    for v in variants:
        for _ in range(warmup):
            call(v)
    times = {v: [] for v in variants}
    rounds = 10
    per = -(-calls // rounds)
    for _ in range(rounds):
        for v in variants:
            for _ in range(per):
                t0 = time.perf_counter(); call(v); times[v].append(time.perf_counter() - t0)
    us = {v: float(np.median(times[v]) * 1e6) for v in variants}
    p10 = {v: float(np.percentile(times[v], 10) * 1e6) for v in variants}
    p90 = {v: float(np.percentile(times[v], 90) * 1e6) for v in variants}
    # device time of a chunk's chain (taps on: events around it; the wall-clock numbers above were taken with them off); the library's
    # average runs over all chains since the taps were first switched on, so the sums are differenced per n
    dev = {}
    for n in NS:
        L.timing_enable(True)
        ms0, c0 = L.timing_get("act_win_chain")
        for _ in range(50):
            call(n)
        ms1, c1 = L.timing_get("act_win_chain")
        dev[n] = dict(chain_us=(ms1 * c1 - ms0 * c0) / max(c1 - c0, 1) * 1e3, chains_per_call=(c1 - c0) / 50.0)
        L.timing_enable(False)
    L.close()
    base = us[0]
    res = dict(shape=what, calls=len(times[0]), warmup=warmup, chunk=min(batch, capi.ACT_SEQ_CHUNK),
               forward_sequence_us=dict(median=base, p10=p10[0], p90=p90[0]),
               forward_sequences=[dict(n=n, median_us=us[n], p10_us=p10[n], p90_us=p90[n], per_agent_us=us[n] / n, loop_us=base * n,
                                       ratio_to_single_call=us[n] / base, speedup_over_loop=base * n / us[n],
                                       chain_us=dev[n]["chain_us"], chains_per_call=dev[n]["chains_per_call"]) for n in NS],
               bar="forward_sequences(64) < 64 x forward_sequence (the loop this call was)", bar_ratio=us[64] / (64 * base),
               bar_met=bool(us[64] < 64 * base))
    print("%s: %s" % (name, what))
    print("  hl_forward_sequence, 1 agent:        %8.1f us  (p10 %.1f, p90 %.1f)" % (base, p10[0], p90[0]))
    for r in res["forward_sequences"]:
        print("  hl_forward_sequences, %4d agents:   %8.1f us  (loop %.1f us: %.2f x faster, %.2f us per agent, chain %.1f us x %.0f)"
              % (r["n"], r["median_us"], r["loop_us"], r["speedup_over_loop"], r["per_agent_us"], r["chain_us"], r["chains_per_call"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    api = load_hip()
    res = dict(device=torch.cuda.get_device_name(0), shapes={name: measure(api, name, a.calls, a.warmup) for name in SHAPES})
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
