"""Wall-clock cost of acting from device memory on the Nature-DQN stack (Network/Builder.cpp:189-194: 84 x 84 frames, nAppendedObs 3, conv
32 / 64 / 64, dense 512, 6 options, batchSize 128) -- the device calls of include/smarties_hip_dev.h serve it through the banded conv-stack
kernel and the panelled row-block kernel of smarties_amd/csrc/actband.hip -- against what a simulator on the GPU pays today for the same
windows: the frames to the host and hl_forward_sequences there, which runs this net over the training buffers and is untouched by the
device route, so its figure is the parent commit's.  The simulator stores ONE frame per step in a [T][n][7056] buffer, n = 64, 256 and
1024 agents, the calls interleaved one after the other in the same process:

    host_from_tensor  the [4][n] frames to the host, turned agent-major there, hl_forward_sequences, the outputs back onto the device
    dev_enqueue       hl_forward_sequences_dev on the [4][n] buffer (row_stride n, first_row = env, n_steps = 4) until it returns
    dev_complete      hl_forward_sequences_dev and a synchronisation of the caller's stream: the outputs are there
and, apart from those, the device time of one call's launches from the library's event timers (kernel_us: act_conv_band_dev, the ONE
launch of the banded kernel; act_rows_panel_dev, the ceil(n / HL_ACT_ROWS_CHUNK) launches of the dense layers behind it together).

The price of banding itself (banding_us): on the stack of settings/RACER_atari.json, which the resident kernel serves, the device time of
act_conv_dev (as shipped) beside act_conv_band_dev of a twin created with SMARTIES_HIP_GENERIC=8192 (three bands of 7, 7 and 6 output rows).

Method: every round is a child process of its own (a fresh HIP context); inside a child a measurement is the median of --calls calls
after --warmup calls, host and device calls alternating.  Reported: the median over the rounds' medians and their spread (min, max).

    python tools/act_band_timing.py [--rounds 5] [--calls 10] [--out profiles/act_band_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NS = (64, 256, 1024)
DS, NAPP = 7056, 3
WIN = 1 + NAPP
SHAPE = "Nature-DQN stack: 84x84x(1+3), conv 32/64/64, dense 512, 6 options, batchSize 128; one frame per step in a [4][n][7056] buffer"
BANDING_SHAPE = "RACER_atari.json: 84x84x(1+3), conv 8/16/32/64, dense 64; act_conv_dev as shipped, act_conv_band_dev under SMARTIES_HIP_GENERIC=8192"
COLUMNS = ("host_from_tensor", "dev_enqueue", "dev_complete")
KERNELS = ("act_conv_band_dev", "act_rows_panel_dev")
BANDING = ("act_conv_dev", "act_conv_band_dev")
KERNEL_CALLS = 10
NATURE = [(84, 84, 4, 32, 8, 4), (20, 20, 32, 64, 4, 2), (9, 9, 64, 64, 3, 1)]
ATARI = [(84, 84, 4, 8, 8, 4), (20, 20, 8, 16, 6, 2), (8, 8, 16, 32, 4, 1), (5, 5, 32, 64, 3, 1)]


def child(calls, warmup):
    import numpy as np
    import torch
    from smarties_amd import capi, load_hip
    from oracle_api import fill_synth, synth_cfg
    api = load_hip()

    def learner(conv, hidden, func, generic=None):
        os.environ.pop("SMARTIES_HIP_GENERIC", None)
        if generic:
            os.environ["SMARTIES_HIP_GENERIC"] = generic      # (read at hl_create)
        cfg = dict(dimS=DS, dimA=1, bounded=[0], adv_kind=capi.ADV_DISCRETE, n_options=6, nAppendedObs=NAPP, hidden=hidden, nnFunc=func,
                   batchSize=128, conv=conv, maxTotObsNum=2048, randSeed=1)
        L = capi.Learner(api, capi.make_config(**cfg)); L.init_weights()
        os.environ.pop("SMARTIES_HIP_GENERIC", None)
        fill_synth(L, synth_cfg(seed=3, dimS=DS, dimA=1, lenMin=20, lenMax=40, pTerm=0.5), 40); L.initialize()
        L.step(5); L.sync()
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

    def kernel_us(L, names, call, stream):
        """the launches of one call alone, from the library's event timers (the timers keep average and count)"""
        L.timing_enable(True)
        k0 = [L.timing_get(k) for k in names]
        for _ in range(KERNEL_CALLS):
            call()
        stream.synchronize()
        k1 = [L.timing_get(k) for k in names]
        L.timing_enable(False)
        return {name: (ms1 * c1 - ms0 * c0) * 1e3 / KERNEL_CALLS for name, (ms0, c0), (ms1, c1) in zip(names, k0, k1)}

    L = learner(NATURE, (512,), "Tanh")
    A, B = learner(ATARI, (64,), "SoftSign"), learner(ATARI, (64,), "SoftSign", "8192")
    res = {}
    rng = np.random.default_rng(0)
    stream = torch.cuda.current_stream()
    for n in NS:
        buf = rng.standard_normal((WIN, n, DS), dtype=np.float32)       # the rollout buffer [T][nEnv][dimS]: one frame per step, agent e is column e
        buf_d = torch.from_numpy(buf).cuda()
        first_d = torch.arange(n, dtype=torch.int64, device="cuda")
        steps_d = torch.full((n,), WIN, dtype=torch.int32, device="cuda")
        out_h = np.zeros((n, L.nOut))
        out_d = torch.empty((n, L.nOut), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        steps_h = np.full(n, WIN, np.int32)
        fwd = api.fn("forward_sequences")

        def host_call(states):      # the bare C call on windows laid back to back (the wrapper's list handling is not the library's cost)
            rc = fwd(L.h, n, steps_h.ctypes.data_as(C.POINTER(C.c_int32)), states.ctypes.data_as(C.POINTER(C.c_float)),
                     out_h.ctypes.data_as(C.POINTER(C.c_double)))
            assert rc == 0

        # (the two routes sum in different orders: the bound the tests hold both to against the oracle, twice)
        host_call(np.ascontiguousarray(buf.transpose(1, 0, 2)))
        dev = L.forward_sequences_dev(buf_d, first_d, steps_d, n).cpu().numpy()
        assert np.abs(dev - out_h).max() <= 2e-5 * np.abs(out_h).max(), n

        def host_from_tensor():
            host_call(np.ascontiguousarray(buf_d.cpu().numpy().transpose(1, 0, 2)))      # agent-major: the windows back to back
            torch.from_numpy(out_h).cuda()
            stream.synchronize()

        def dev_complete():
            L.forward_sequences_dev(buf_d, first_d, steps_d, n, out=out_d); stream.synchronize()

        us = median_us(dict(host_from_tensor=host_from_tensor, dev_complete=dev_complete))
        # (the enqueue alone is timed apart, with a synchronisation OUTSIDE the bracket so that the queue does not grow)
        t = []
        for _ in range(calls):
            t0 = time.perf_counter(); L.forward_sequences_dev(buf_d, first_d, steps_d, n, out=out_d); t.append(time.perf_counter() - t0)
            stream.synchronize()
        us["dev_enqueue"] = float(np.median(t) * 1e6)
        for k, v in kernel_us(L, KERNELS, lambda: L.forward_sequences_dev(buf_d, first_d, steps_d, n, out=out_d), stream).items():
            us["kernel_" + k] = v
        # the same frames through the RACER_atari.json stack, resident and banded: the same bits, two kernels
        a = A.forward_sequences_dev(buf_d, first_d, steps_d, n).cpu().numpy()
        b = B.forward_sequences_dev(buf_d, first_d, steps_d, n).cpu().numpy()
        assert np.array_equal(a, b), n
        out_a = torch.empty((n, A.nOut), dtype=torch.float64, device="cuda")
        us["banding_act_conv_dev"] = kernel_us(A, BANDING[:1], lambda: A.forward_sequences_dev(buf_d, first_d, steps_d, n, out=out_a), stream)[BANDING[0]]
        us["banding_act_conv_band_dev"] = kernel_us(B, BANDING[1:], lambda: B.forward_sequences_dev(buf_d, first_d, steps_d, n, out=out_a), stream)[BANDING[1]]
        res[str(n)] = us
        del buf_d, buf
    for X in (L, A, B):
        X.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.calls, a.warmup)
    assert a.rounds >= 5, "medians of at least five runs"
    runs = []
    for r in range(a.rounds):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--warmup", str(a.warmup)],
                           stdout=subprocess.PIPE, text=True, timeout=240)
        if p.returncode != 0:      # (nothing more is started on the device after a child that failed)
            sys.exit("round %d: the child ended with status %d" % (r, p.returncode))
        runs.append(json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:]))
        print("round %d done" % r, flush=True)

    def stat(vals):
        v = sorted(vals)
        return dict(median=v[len(v) // 2], min=v[0], max=v[-1])

    res = dict(shape=SHAPE, banding_shape=BANDING_SHAPE, rounds=a.rounds, calls=a.calls, warmup=a.warmup, forward_us={})
    for n in NS:
        res["forward_us"][str(n)] = {k: stat([x[str(n)][k] for x in runs]) for k in COLUMNS}
    res["kernel_us"] = {str(n): {k: stat([x[str(n)]["kernel_" + k] for x in runs]) for k in KERNELS} for n in NS}
    res["banding_us"] = {str(n): {k: stat([x[str(n)]["banding_" + k] for x in runs]) for k in BANDING} for n in NS}
    for key in ("forward_us", "kernel_us", "banding_us"):
        for n, d in res[key].items():
            print("%s n=%5s  " % (key, n) + "   ".join("%s %.1f (%.1f .. %.1f)" % (k, v["median"], v["min"], v["max"]) for k, v in d.items()))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
