"""Eager step time of a convolutional net of general geometry (convg.hip) and of the RACER_atari.json stack, which keeps conv.hip's and
convt.hip's kernels, on the GPU; writes profiles/convg_timing.json (--out).

    same84   three 3 x 3 layers of 32 channels, stride 1, padding 1 on 84 x 84 x (1 + 3) frames, one dense layer of 32, batch 128
    atari    the RACER_atari.json stack as shipped, dense 512, batch 128

Per net: --rounds rounds of --per eager steps (hl_step(1) each, one synchronise per round) behind --warmup rounds, host clock; then the
device-event taps of the conv launches over one more round.  For same84 the achieved fraction of the fp32 MFMA peak of the middle layer's
forward launch (convg_fwd1), counting the minibatch rows only -- the launch also computes the truncated next-state rows, so the true
fraction is higher."""
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
DS, NAPP, BATCH = 84 * 84, 3, 128
SAME84 = [(84, 84, 4, 32, 3, 1, (1, 1)), (84, 84, 32, 32, 3, 1, (1, 1)), (84, 84, 32, 32, 3, 1, (1, 1))]
ATARI = [(84, 84, 4, 8, 8, 4), (20, 20, 8, 16, 6, 2), (8, 8, 16, 32, 4, 1), (5, 5, 32, 64, 3, 1)]
NETS = {"same84": (SAME84, 32), "atari": (ATARI, 512)}
TAPS = (["conv_fwd%d" % l for l in range(4)] + ["conv_dx%d" % l for l in range(1, 4)] + ["convg_%s%d" % (k, l) for k in ("fwd", "prep", "dx", "dw") for l in range(3)]
        + ["conv_fwd_tail", "conv_back", "conv_dw", "conv_dw_all", "conv_dw_rows", "conv_dw_dense", "conv_reduce_adam"])


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--per", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    api = load_hip()
    res = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, steps_per_round=a.per, warmup_rounds=a.warmup, batch=BATCH,
               peak_fp32_mfma_tflops=PEAK_FP32_MFMA / 1e12, nets={})
    for net, (conv, dense) in NETS.items():
        L = capi.Learner(api, capi.make_config(dimS=DS, dimA=1, adv_kind=capi.ADV_DISCRETE, n_options=6, nAppendedObs=NAPP, conv=conv, hidden=(dense,),
                                               nnFunc="Tanh", batchSize=BATCH, maxTotObsNum=4000, randSeed=1))
        L.init_weights()
        fill_synth(L, synth_cfg(seed=3, dimS=DS, dimA=1, lenMin=40, lenMax=80, pTerm=0.7), 24)
        L.initialize()
        wall = []
        for r in range(a.warmup + a.rounds):
            t0 = time.perf_counter()
            for _ in range(a.per):
                L.step(1)
            L.sync()
            if r >= a.warmup:
                wall.append((time.perf_counter() - t0) / a.per * 1e6)
        L.timing_enable(True)
        for _ in range(a.per):
            L.step(1)
        L.sync()
        taps = {}
        for n in TAPS:
            ms, cnt = L.timing_get(n)
            if cnt:
                taps[n] = dict(us_per_launch=ms * 1e3, launches_per_step=cnt / a.per)
        L.timing_enable(False)
        out = dict(eager_step_us=spread(wall), conv_launches=taps)
        if net == "same84" and "convg_fwd1" in taps:
            flop = 2.0 * BATCH * 84 * 84 * 32 * (32 * 9)      # minibatch rows only
            out["convg_fwd1_fraction_of_fp32_mfma_peak_minibatch_rows_only"] = flop / (taps["convg_fwd1"]["us_per_launch"] * 1e-6) / PEAK_FP32_MFMA
        res["nets"][net] = out
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
