"""Cost of a training step of wide recurrent stacks on the time-step-major launches (smarties_amd/csrc/rectm.hip): plain RNN layers
(rnn_tm_fwd_kernel / rnn_tm_bwd_kernel) beside LSTM layers of the same number of cells, 2 x 272 and 2 x 512.

V-RACER, dimS 17 / dimA 6, batch 128, windows of 16 + 1 steps.  One process, one learner per variant; every call is the replayed
graph of --per steps (hl_prepare_steps) and the variants are interleaved in rounds, so that drift of the device hits all alike.  A
figure is the median over the rounds of (wall-clock time of a call, synchronised) / --per, i.e. the sustained time per step, over
--rounds x --per >= 200 steps after --warmup calls.  A second pass with the library's timing taps on (eager steps, HIP events
around the launches) gives the device time of the recurrent forward chain, the backward chain and the weight-gradient launch.

The achieved fraction of the fp32 MFMA peak (157.3 TFLOP/s) counts the products of the recurrent layers only -- forward, error
back-propagation and weight gradients -- over the device time of those three.

    python tools/rnn_tm_timing.py [--rounds 12] [--per 20] [--warmup 3] [--out profiles/rnn_tm_timing.json]
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

DS, DA, BATCH, BPTT = 17, 6, 128, 16
PEAK_FP32_MFMA = 157.3e12
VARIANTS = [("rnn", 272), ("rnn", 512), ("lstm", 272), ("lstm", 512)]


def rec_flop(kind, cells):
    """floating-point operations of the recurrent layers' products in one step: two layers, BATCH windows of BPTT + 1 rows"""
    g, rows, total, n_in = (1 if kind == "rnn" else 4), BATCH * (BPTT + 1), 0, DS
    for j in range(2):
        total += 2 * rows * (n_in + cells) * g * cells                               # forward
        total += 2 * rows * ((n_in if j > 0 else 0) + cells) * g * cells             # errors below and to the step before
        total += 2 * rows * (n_in + cells + 1) * g * cells                           # weight and bias gradients
        n_in = cells
    return total


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
    sc = synth_cfg(seed=3, dimS=DS, dimA=DA, lenMin=100, lenMax=300, pTerm=0.7)
    Ls = {}
    for kind, cells in VARIANTS:
        cfg = dict(dimS=DS, dimA=DA, hidden=(cells, cells), nnFunc="Tanh", batchSize=BATCH, maxTotObsNum=262144, randSeed=1,
                   nn_type=capi.NN_RNN if kind == "rnn" else capi.NN_LSTM, nnBPTTseq=BPTT)
        L = capi.Learner(api, capi.make_config(**cfg)); L.init_weights()
        fill_synth(L, sc, 100); L.initialize()
        L.prepare_steps(a.per)
        Ls[(kind, cells)] = L
    for L in Ls.values():
        for _ in range(a.warmup):
            L.step(a.per)
        L.sync()
    times = {v: [] for v in VARIANTS}
    for _ in range(a.rounds):
        for v in VARIANTS:
            L = Ls[v]
            t0 = time.perf_counter(); L.step(a.per); L.sync(); times[v].append((time.perf_counter() - t0) / a.per)
    res = dict(config="V-RACER, dimS %d, dimA %d, batch %d, nnBPTTseq %d, two layers, hl_prepare_steps(%d)" % (DS, DA, BATCH, BPTT, a.per),
               device=torch.cuda.get_device_name(0), steps_per_figure=a.rounds * a.per, warmup_steps=a.warmup * a.per,
               peak_fp32_mfma_tflops=PEAK_FP32_MFMA / 1e12, variants=[])
    for v in VARIANTS:
        L = Ls[v]
        L.timing_enable(True)
        L.step(1); L.step(a.per); L.sync()
        dev = {}
        for k in ("rec_forward", "rec_backward", "big_dw"):
            ms, n = L.timing_get(k)
            dev[k] = dict(us=ms * 1e3, launches=int(n))
        L.timing_enable(False)
        t = np.asarray(times[v]) * 1e6
        rec_us = sum(d["us"] for d in dev.values())
        flop = rec_flop(*v)
        res["variants"].append(dict(type=v[0], cells=v[1], step_us_median=float(np.median(t)), step_us_p10=float(np.percentile(t, 10)),
                                    step_us_p90=float(np.percentile(t, 90)), rec_forward_us=dev["rec_forward"]["us"],
                                    rec_backward_us=dev["rec_backward"]["us"], big_dw_us=dev["big_dw"]["us"], timed_calls=dev["rec_forward"]["launches"],
                                    rec_gflop_per_step=flop / 1e9, mfma_peak_fraction=flop / (rec_us * 1e-6) / PEAK_FP32_MFMA if rec_us > 0 else None))
        r = res["variants"][-1]
        print("%-4s 2 x %3d: %8.1f us per step (p10 %.1f, p90 %.1f); forward %.1f, backward %.1f, dW %.1f us; %.3f GFLOP, %.1f %% of the fp32 MFMA peak"
              % (v[0], v[1], r["step_us_median"], r["step_us_p10"], r["step_us_p90"], r["rec_forward_us"], r["rec_backward_us"], r["big_dw_us"],
                 r["rec_gflop_per_step"], 100 * (r["mfma_peak_fraction"] or 0)))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
