"""Cost of recurrent image agents: LSTM layers of 512 cells behind a convolutional stack (smarties_amd/csrc/rectm.hip behind conv.hip: the
stack over the B x (nnBPTTseq + 2) window rows, the prepare launch that joins its feature rows to the first layer's operand rows,
tm_win_product_kernel, the time-step-major chain, the gradient into the feature rows, the weight gradients, the convolutions' backward pass).

Two nets, discrete RACER with 6 options, 84 x 84 frames x (1 + 3 appended), nnBPTTseq 16:
    atari    the RACER_atari.json stack (a feature row of 576 floats) + LSTM 512, batch 128
    nature   the Nature stack of Network/Builder.cpp:189-194 (3136 floats) + LSTM 512, batch 32
One process.  Per net: the time of an eager step (wall clock around --per steps ending in a synchronisation, median over --rounds), then
the device time per step of every launch group from the library's timing taps (HIP events around the launches), then acting for 1 and
64 agents on windows of nnBPTTseq + 1 + 3 states (hl_forward_sequences, wall clock per call: the call returns with the outputs).
The input product and the gradient into the feature rows are also given as a fraction of the 157.3 TFLOP/s fp32 MFMA peak (operations
from the shapes: 2 x rows x inputs x 4 x cells each, over the launch's device time).

At 576 inputs both forms of the gradient into the feature rows serve: the table's GEMM_X problem (gemm16.hip), which these nets keep, and
tm_conv_dx_kernel (SMARTIES_HIP_GENERIC bit 2048).  Two atari learners, one per form, step in alternation, --rounds rounds of --per steps with
the taps on; a figure is the median over the rounds of the launch's mean device time, with the 10th and 90th percentile beside it.

    python tools/conv_rec_wide_timing.py [--rounds 10] [--per 10] [--warmup 2] [--out FILE]

(--out: where the result is also written as a file, profiles/conv_rec_wide_timing.json for the committed one; without it the JSON line is printed only)
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

PEAK_FP32_MFMA = 157.3e12
DS, NAPP, BPTT, CELLS, NOPT = 84 * 84, 3, 16, 512, 6
ATARI = [(84, 84, 4, 8, 8, 4), (20, 20, 8, 16, 6, 2), (8, 8, 16, 32, 4, 1), (5, 5, 32, 64, 3, 1)]
NATURE = [(84, 84, 4, 32, 8, 4), (20, 20, 32, 64, 4, 2), (9, 9, 64, 64, 3, 1)]
NETS = {"atari": (ATARI, 576, 128), "nature": (NATURE, 3136, 32)}
# launch groups of a step: the taps of smarties_amd/csrc/step_exec.h summed per group
GROUPS = {
    "sampler_and_rows": ["step_tail_kernel", "window_rows", "stack_gather", "extras_copy"],
    "conv_front": ["conv_fwd%d" % l for l in range(4)] + ["conv_fwd_tail"],
    "join": ["rec_prepare"],
    "product": ["rec_in_product"],
    "chain_forward": ["rec_forward"],
    "head": ["head_kernel", "panel_head"],
    "chain_backward": ["rec_backward"],
    "dx": ["gemm16_dx1"],
    "dw": ["big_dw", "gemm16_dw", "splitk_reduce", "dw_wide", "dw_direct"],
    "conv_backward": ["conv_back", "conv_dw", "conv_dw_all", "conv_dw_rows", "conv_dw_dense", "conv_reduce_adam"] + ["conv_dx%d" % l for l in range(1, 4)],
    "bookkeeping": ["post_kernel"],
}


def learner(api, net, generic=0):
    conv, _, batch = NETS[net]
    before = os.environ.get("SMARTIES_HIP_GENERIC")
    os.environ["SMARTIES_HIP_GENERIC"] = str(generic)      # (read by hl_create)
    L = capi.Learner(api, capi.make_config(dimS=DS, dimA=1, adv_kind=capi.ADV_DISCRETE, n_options=NOPT, nAppendedObs=NAPP, conv=conv, hidden=(CELLS,),
                                           nnFunc="Tanh", batchSize=batch, maxTotObsNum=4000, randSeed=1, nn_type=capi.NN_LSTM, nnBPTTseq=BPTT))
    if before is None:
        os.environ.pop("SMARTIES_HIP_GENERIC")
    else:
        os.environ["SMARTIES_HIP_GENERIC"] = before
    L.init_weights()
    fill_synth(L, synth_cfg(seed=3, dimS=DS, dimA=1, lenMin=40, lenMax=80, pTerm=0.7), 24)
    L.initialize()
    return L


def taps(L, per):
    """device microseconds per step of every group, from `per` eager steps with the taps on"""
    L.timing_enable(True)
    L.step(per); L.sync()
    out = {}
    for g, names in GROUPS.items():
        us = 0.0
        for n in names:
            ms, cnt = L.timing_get(n)
            us += ms * 1e3 * cnt / per
        out[g] = us
    L.timing_enable(False)
    return out


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--per", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    api = load_hip()
    res = dict(config="discrete RACER, %d options, 84 x 84 x (1 + %d) frames, LSTM %d, nnBPTTseq %d; eager steps" % (NOPT, NAPP, CELLS, BPTT),
               device=torch.cuda.get_device_name(0), rounds=a.rounds, steps_per_round=a.per, warmup_steps=a.warmup * a.per,
               peak_fp32_mfma_tflops=PEAK_FP32_MFMA / 1e12, nets={})
    rng = np.random.default_rng(0)
    for net, (_, n_in, batch) in NETS.items():
        L = learner(api, net)
        for _ in range(a.warmup):
            L.step(a.per)
        L.sync()
        wall = []
        for _ in range(a.rounds):
            t0 = time.perf_counter(); L.step(a.per); L.sync(); wall.append((time.perf_counter() - t0) / a.per * 1e6)
        groups = [taps(L, a.per) for _ in range(a.rounds)]
        g = {k: spread([x[k] for x in groups]) for k in GROUPS}
        rows = batch * (BPTT + 2)      # every window row, the next state's included
        flop = 2.0 * rows * n_in * 4 * CELLS
        acting = {}
        for agents in (1, 64):
            wins = [rng.normal(size=(BPTT + 1 + NAPP, DS)).astype(np.float32) for _ in range(agents)]
            for _ in range(3):
                L.forward_sequences(wins)
            t = []
            for _ in range(max(a.rounds, 10)):
                t0 = time.perf_counter(); L.forward_sequences(wins); t.append((time.perf_counter() - t0) * 1e6)
            acting["agents_%d_call_us" % agents] = spread(t)
        r = dict(feature_row=n_in, batch=batch, window_rows=rows, step_us_wall=spread(wall), device_us_per_step=g,
                 product_gflop=flop / 1e9, product_mfma_peak_fraction=flop / (g["product"]["median"] * 1e-6) / PEAK_FP32_MFMA,
                 dx_form="tm_conv_dx_kernel" if n_in > 1024 else "GEMM_X problem (gemm16.hip)",
                 dx_gflop=flop / 1e9, dx_mfma_peak_fraction=flop / (g["dx"]["median"] * 1e-6) / PEAK_FP32_MFMA, acting=acting)
        res["nets"][net] = r
        print("%-6s step %.0f us (wall, p10 %.0f p90 %.0f); device: %s" % (net, r["step_us_wall"]["median"], r["step_us_wall"]["p10"], r["step_us_wall"]["p90"],
              ", ".join("%s %.1f" % (k, v["median"]) for k, v in g.items())), flush=True)
        print("       product %.3f of the fp32 MFMA peak, dX (%s) %.3f; acting 1 agent %.0f us, 64 agents %.0f us per call"
              % (r["product_mfma_peak_fraction"], r["dx_form"], r["dx_mfma_peak_fraction"], acting["agents_1_call_us"]["median"], acting["agents_64_call_us"]["median"]), flush=True)
        L.close()
    # both forms of the gradient into the feature rows at 576 inputs, in alternation
    pair = {"gemm_x": learner(api, "atari", 0), "tm_conv_dx": learner(api, "atari", 2048)}
    for L in pair.values():
        for _ in range(a.warmup):
            L.step(a.per)
        L.sync()
    dx = {k: [] for k in pair}
    for _ in range(a.rounds):
        for k, L in pair.items():
            L.timing_enable(True); L.step(a.per); L.sync()
            ms, cnt = L.timing_get("gemm16_dx1")
            assert cnt == a.per, (k, cnt)
            dx[k].append(ms * 1e3)
            L.timing_enable(False)
    cmp_ = {k: spread(v) for k, v in dx.items()}
    cmp_["ratio_tm_conv_dx_over_gemm_x"] = cmp_["tm_conv_dx"]["median"] / cmp_["gemm_x"]["median"]
    res["dx_forms_at_576_inputs"] = cmp_
    print("dX at 576 inputs, 2304 rows, 2048 gate columns: GEMM_X %.1f us (p10 %.1f p90 %.1f), tm_conv_dx_kernel %.1f us (p10 %.1f p90 %.1f): ratio %.2f"
          % (cmp_["gemm_x"]["median"], cmp_["gemm_x"]["p10"], cmp_["gemm_x"]["p90"], cmp_["tm_conv_dx"]["median"], cmp_["tm_conv_dx"]["p10"], cmp_["tm_conv_dx"]["p90"],
             cmp_["ratio_tm_conv_dx_over_gemm_x"]), flush=True)
    for L in pair.values():
        L.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
