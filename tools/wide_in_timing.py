"""Cost of a training step of recurrent nets on wide inputs (smarties_amd/csrc/rectm.hip: tm_win_product_kernel in front of the
time-step-major forward chain whose first layer reduces over its recurrent weights alone).

V-RACER on two LSTM layers of 128 cells, dimA 6, batch 128, windows of 16 + 1 steps, three appended observations; the state width sets
the stacked input: 256 x 4 = 1024 (the widest the forward tiles stage themselves: the route these nets had before, the reference point),
260 x 4 = 1040, 512 x 4 = 2048 and 2048 x 4 = 8192 (the input product as a launch of its own).  One process, one learner per variant;
every call is the replayed graph of --per steps (hl_prepare_steps) and the variants are interleaved in rounds, so that drift of the
device hits all alike.  A figure is the median over the rounds of (wall-clock time of a call, synchronised) / --per, i.e. the sustained
time per step, over --rounds x --per >= 200 steps after --warmup calls.  A second pass with the library's timing taps on (eager steps,
HIP events around the launches) gives the device time of the prepare launch, the product launch, the forward chain, the backward chain
and the weight-gradient launch per step.

    python tools/wide_in_timing.py [--rounds 12] [--per 20] [--warmup 3] [--out profiles/wide_in_timing.json]
"""
import argparse
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

DA, BATCH, BPTT, NAPP, CELLS = 6, 128, 16, 3, 128
PEAK_FP32_MFMA = 157.3e12
STATES = [256, 260, 512, 2048]      # x (1 + NAPP) = 1024, 1040, 2048, 8192 inputs
TAPS = ("rec_prepare", "rec_in_product", "rec_forward", "rec_backward", "big_dw")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--per", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.rounds * a.per >= 200, "a figure is the median of at least 200 steps"
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    api = load_hip()
    Ls = {}
    for dS in STATES:
        cfg = dict(dimS=dS, dimA=DA, hidden=(CELLS, CELLS), nnFunc="Tanh", batchSize=BATCH, maxTotObsNum=32768, randSeed=1,
                   nn_type=capi.NN_LSTM, nnBPTTseq=BPTT, nAppendedObs=NAPP)
        L = capi.Learner(api, capi.make_config(**cfg)); L.init_weights()
        fill_synth(L, synth_cfg(seed=3, dimS=dS, dimA=DA, lenMin=100, lenMax=300, pTerm=0.7), 40); L.initialize()
        L.prepare_steps(a.per)
        Ls[dS] = L
    for L in Ls.values():
        for _ in range(a.warmup):
            L.step(a.per)
        L.sync()
    times = {dS: [] for dS in STATES}
    for _ in range(a.rounds):
        for dS in STATES:
            L = Ls[dS]
            t0 = time.perf_counter(); L.step(a.per); L.sync(); times[dS].append((time.perf_counter() - t0) / a.per)
    res = dict(config="V-RACER, LSTM 2 x %d cells, dimA %d, batch %d, nnBPTTseq %d, nAppendedObs %d, hl_prepare_steps(%d)" % (CELLS, DA, BATCH, BPTT, NAPP, a.per),
               device=torch.cuda.get_device_name(0), steps_per_figure=a.rounds * a.per, warmup_steps=a.warmup * a.per,
               peak_fp32_mfma_tflops=PEAK_FP32_MFMA / 1e12, variants=[])
    for dS in STATES:
        L = Ls[dS]
        n_in = dS * (1 + NAPP)
        L.timing_enable(True)
        L.step(1); L.step(a.per); L.sync()
        dev = {}
        for k in TAPS:
            ms, n = L.timing_get(k)
            dev[k] = dict(us=ms * 1e3, launches=int(n))
        L.timing_enable(False)
        t = np.asarray(times[dS]) * 1e6
        rows = BATCH * (BPTT + 2)      # the product covers every window row, the next state's included
        flop = 2.0 * rows * n_in * 4 * CELLS
        p_us = dev["rec_in_product"]["us"]
        r = dict(dimS=dS, stacked_input=n_in, route="input product launch" if dev["rec_in_product"]["launches"] else "forward tiles stage the whole row",
                 step_us_median=float(np.median(t)), step_us_p10=float(np.percentile(t, 10)), step_us_p90=float(np.percentile(t, 90)),
                 rec_prepare_us=dev["rec_prepare"]["us"], rec_in_product_us=p_us, rec_forward_us=dev["rec_forward"]["us"],
                 rec_backward_us=dev["rec_backward"]["us"], big_dw_us=dev["big_dw"]["us"], timed_calls=dev["rec_forward"]["launches"],
                 in_product_gflop=flop / 1e9, in_product_mfma_peak_fraction=flop / (p_us * 1e-6) / PEAK_FP32_MFMA if p_us > 0 else None)
        res["variants"].append(r)
        print("inputs %5d (%s): %8.1f us per step (p10 %.1f, p90 %.1f); prepare %.1f, product %.1f, forward chain %.1f, backward %.1f, dW %.1f us"
              % (n_in, r["route"], r["step_us_median"], r["step_us_p10"], r["step_us_p90"], r["rec_prepare_us"], p_us, r["rec_forward_us"],
                 r["rec_backward_us"], r["big_dw_us"]))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
