"""Wall-clock cost of acting from device memory for conv stacks of general geometry (hl_forward_sequences_dev through actconvg.hip:
act_convg_dev_kernel, one launch per conv layer) against the only acting route the commit before had for these nets, hl_forward fed from
host tensors over the training forward launches, in the SAME run, n = 1, 16 and 256 agents:

    same84      three 3 x 3 layers of 32 channels, stride 1, padding 1 on 84 x 84 x (1 + 3) frames, dense 32 (profiles/convg_timing.json).
                Its feature row is 32 x 84 x 84 = 225 792 floats, beyond HL_ACT_DEV_MAX_ROW = 8192: the device route declines it, and
                the refusal is what the file records for it
    same84-s8   the same three layers and an 8 x 8 layer of stride 8, padding 1 behind them (32 x 10 x 10 = 3200 features): the stack the route serves
    same-3x3    the net of that name of tests/test_convg_cpu.py

    host              hl_forward on the agents' stacked rows in host memory (numpy), outputs in host memory
    host_from_tensor  what a simulator on the GPU pays for that call: the frames to the host, stacked there, hl_forward, the outputs back
    dev_complete      hl_forward_sequences_dev on the [T][n][dimS] buffer and a synchronisation of the caller's stream
and the device time of one call's act_convg_dev launches from the library's event timers (all layers of all chunks together: the
layers share one label) with the share of the fp32 MFMA peak the stack's multiply-adds reach in it.

Method: every round is a child process of its own (a fresh HIP context); inside a child a measurement is the median of --calls calls
after --warmup calls, host and device calls alternating.  Reported: the median over the rounds' medians and their spread (min, max).

    python tools/act_convg_timing.py [--rounds 5] [--calls 10] [--out profiles/act_convg_dev_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

PEAK_FP32_MFMA = 157.3e12
NS = (1, 16, 256)
SAME84 = [(84, 84, 4, 32, 3, 1, (1, 1)), (84, 84, 32, 32, 3, 1, (1, 1)), (84, 84, 32, 32, 3, 1, (1, 1))]
BIG = dict(dimS=84 * 84, dimA=1, adv_kind=2, n_options=6, nAppendedObs=3, hidden=(32,), nnFunc="Tanh", batchSize=128, maxTotObsNum=4000, randSeed=1)
COLUMNS = ("host", "host_from_tensor", "dev_complete")
KERNEL_CALLS = 10


def nets():
    from smarties_amd import capi
    from test_convg_cpu import NETS
    big = dict(BIG, adv_kind=capi.ADV_DISCRETE)
    small, sc, eps = NETS["same-3x3"]
    return {"same84": (dict(big, conv=SAME84), dict(seed=3, dimS=84 * 84, dimA=1, lenMin=40, lenMax=80, pTerm=0.7), 24),
            "same84-s8": (dict(big, conv=SAME84 + [(84, 84, 32, 32, 8, 8, (1, 1))]), dict(seed=3, dimS=84 * 84, dimA=1, lenMin=40, lenMax=80, pTerm=0.7), 24),
            "same-3x3": (small, sc, eps)}


def stack_flop(conv):
    """multiply-adds x 2 of one agent's conv stack"""
    total = 0
    for c in conv:
        W, H, C, F, k, s = c[:6]
        p = c[6] if len(c) > 6 else (0, 0)
        kx, ky = k if isinstance(k, tuple) else (k, k)
        sx, sy = s if isinstance(s, tuple) else (s, s)
        total += 2 * F * ((H + 2 * p[1] - ky) // sy + 1) * ((W + 2 * p[0] - kx) // sx + 1) * C * kx * ky
    return total


def child(net, calls, warmup):
    import numpy as np
    import torch
    from smarties_amd import capi, load_hip
    from oracle_api import fill_synth, synth_cfg
    kw, sc, eps = nets()[net]
    L = capi.Learner(load_hip(), capi.make_config(**kw)); L.init_weights()
    fill_synth(L, synth_cfg(**sc), eps); L.initialize()
    L.step(3); L.sync()
    dS, nApp = kw["dimS"], kw.get("nAppendedObs", 0)
    T = 1 + nApp
    res = {}
    rng = np.random.default_rng(0)
    stream = torch.cuda.current_stream()
    for n in NS:
        buf = rng.standard_normal((T, n, dS), dtype=np.float32)       # the rollout buffer [T][nEnv][dimS]: one frame per step, agent e is column e
        buf_d = torch.from_numpy(buf).cuda()
        first_d = torch.arange(n, dtype=torch.int64, device="cuda")
        steps_d = torch.full((n,), T, dtype=torch.int32, device="cuda")
        out_d = torch.empty((n, L.nOut), dtype=torch.float64, device="cuda")

        def stacked(b):      # newest state first, as hl_forward reads a row
            return np.ascontiguousarray(b[::-1].transpose(1, 0, 2).reshape(n, T * dS))

        rows = stacked(buf)
        host = L.forward(rows)
        try:
            dev = L.forward_sequences_dev(buf_d, first_d, steps_d, n).cpu().numpy()
        except capi.HlError as e:
            print("RESULT " + json.dumps(dict(declined=str(e))))
            return
        assert np.abs(dev - host).max() <= 2e-5 * np.abs(host).max(), n      # (two routes, two orders of the sums: the tests' bar, twice)

        def host_from_tensor():
            torch.from_numpy(L.forward(stacked(buf_d.cpu().numpy()))).cuda()
            stream.synchronize()

        def dev_complete():
            L.forward_sequences_dev(buf_d, first_d, steps_d, n, out=out_d); stream.synchronize()

        fns = dict(host=lambda: L.forward(rows), host_from_tensor=host_from_tensor, dev_complete=dev_complete)
        for _ in range(warmup):
            for f in fns.values():
                f()
        t = {k: [] for k in fns}
        for _ in range(calls):
            for k, f in fns.items():
                t0 = time.perf_counter(); f(); t[k].append(time.perf_counter() - t0)
        us = {k: float(np.median(v) * 1e6) for k, v in t.items()}
        L.timing_enable(True)
        ms0, c0 = L.timing_get("act_convg_dev")
        for _ in range(KERNEL_CALLS):
            L.forward_sequences_dev(buf_d, first_d, steps_d, n, out=out_d)
        stream.synchronize()
        ms1, c1 = L.timing_get("act_convg_dev")
        L.timing_enable(False)
        us["kernel_act_convg_dev"] = (ms1 * c1 - ms0 * c0) * 1e3 / KERNEL_CALLS      # all layer launches of one call (the timers keep average and count)
        us["layer_launches_per_call"] = (c1 - c0) / KERNEL_CALLS
        res[str(n)] = us
    L.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.calls, a.warmup)
    assert a.rounds >= 5, "medians of at least five runs"

    def stat(vals):
        v = sorted(vals)
        return dict(median=v[len(v) // 2], min=v[0], max=v[-1])

    res = dict(rounds=a.rounds, calls=a.calls, warmup=a.warmup, peak_fp32_mfma_tflops=PEAK_FP32_MFMA / 1e12, nets={})
    for net, (kw, _, _) in nets().items():
        runs = []
        for r in range(a.rounds):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", net, "--calls", str(a.calls), "--warmup", str(a.warmup)],
                               stdout=subprocess.PIPE, text=True, timeout=280)
            if p.returncode != 0:      # (nothing more is started on the device after a child that failed)
                sys.exit("%s round %d: the child ended with status %d" % (net, r, p.returncode))
            runs.append(json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:]))
            print("%s round %d done" % (net, r), flush=True)
            if "declined" in runs[-1]:
                break
        if "declined" in runs[-1]:
            res["nets"][net] = runs[-1]
            continue
        out = {}
        for n in NS:
            out[str(n)] = {k: stat([x[str(n)][k] for x in runs]) for k in COLUMNS + ("kernel_act_convg_dev", "layer_launches_per_call")}
            k_us = out[str(n)]["kernel_act_convg_dev"]["median"]
            out[str(n)]["stack_fraction_of_fp32_mfma_peak"] = n * stack_flop(kw["conv"]) / (k_us * 1e-6) / PEAK_FP32_MFMA
            out[str(n)]["dev_complete_over_host_from_tensor"] = out[str(n)]["dev_complete"]["median"] / out[str(n)]["host_from_tensor"]["median"]
        res["nets"][net] = out
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
