"""Wall-clock cost of acting from device memory for a recurrent net on wide inputs (hl_forward_sequences_dev of
include/smarties_hip_dev.h: the time-step-major chain behind lstm_tm_prepare_acts_dev_kernel) against hl_forward_sequences of the SAME
build -- the host call's code is unchanged from the parent commit, so it is the baseline -- on the shape README.md quotes for wide
inputs (two LSTM layers of 128 cells on 1040 inputs, nnBPTTseq 16, batch 128), n = 16, 64 and 256 agents with full windows of 17 states,
the calls interleaved one after the other in the same process:

    host              hl_forward_sequences on windows back to back in host memory (numpy), outputs in host memory (the bare C call)
    host_from_tensor  what a simulator on the GPU pays for that call: the [17][n] rollout buffer to the host, turned agent-major there,
                      hl_forward_sequences, the outputs back onto the device
    dev_enqueue       hl_forward_sequences_dev on the [17][n] buffer (row_stride n) until it returns (it waits for nothing)
    dev_complete      hl_forward_sequences_dev and a synchronisation of the caller's stream: the outputs are there
and, apart from those, the device time of one call's launches from the library's event timers (kernel_us: act_tm_chain, the host call's
chains over its chunks together; act_tm_dev, the device call's one bracket over all its chunks).

Method: every round is a child process of its own (a fresh HIP context); inside a child a measurement is the median of --calls calls
after --warmup calls, host and device calls alternating.  Reported: the median over the rounds' medians and their spread (min, max).

    python tools/act_wide_dev_timing.py [--rounds 5] [--calls 50] [--out profiles/act_wide_dev_timing.json]
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

NS = (16, 64, 256)
DS, WIN = 1040, 17
SHAPE = "LSTM 2x128, dimS 1040, 17-step windows, batch 128"
COLUMNS = ("host", "host_from_tensor", "dev_enqueue", "dev_complete")
BRACKETS = ("act_tm_chain", "act_tm_dev")
KERNEL_CALLS = 20


def child(calls, warmup):
    import numpy as np
    import torch
    from smarties_amd import capi, load_hip
    from oracle_api import fill_synth, synth_cfg
    api = load_hip()
    cfg = dict(dimS=DS, dimA=2, bounded=[1, 0], hidden=(128, 128), nnFunc="Tanh", batchSize=128, maxTotObsNum=65536, randSeed=1, gamma=0.99,
               adv_kind=capi.ADV_GAUSSIAN, nn_type=capi.NN_LSTM, nnLambda=1e-6, explNoise=0.1, nnBPTTseq=WIN - 1)
    L = capi.Learner(api, capi.make_config(**cfg)); L.init_weights()
    fill_synth(L, synth_cfg(seed=3, dimS=DS, dimA=2, lenMin=40, lenMax=120, pTerm=0.7), 40); L.initialize()
    L.step(5); L.sync()

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

    res = {}
    rng = np.random.default_rng(0)
    stream = torch.cuda.current_stream()
    for n in NS:
        buf = rng.standard_normal((WIN, n, DS)).astype(np.float32)      # the rollout buffer [T][nEnv][dimS]: agent e is column e
        buf_d = torch.from_numpy(buf).cuda()
        first_d = torch.arange(n, dtype=torch.int64, device="cuda")
        steps_d = torch.full((n,), WIN, dtype=torch.int32, device="cuda")
        out_h = np.zeros((n, L.nOut))
        out_d = torch.empty((n, L.nOut), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        # the bare C call on windows laid back to back (the wrapper's list handling is not the library's cost)
        packed = np.ascontiguousarray(buf.transpose(1, 0, 2))
        steps_h = np.full(n, WIN, np.int32)
        fwd = api.fn("forward_sequences")

        def host_call(states):
            rc = fwd(L.h, n, steps_h.ctypes.data_as(C.POINTER(C.c_int32)), states.ctypes.data_as(C.POINTER(C.c_float)),
                     out_h.ctypes.data_as(C.POINTER(C.c_double)))
            assert rc == 0

        host_call(packed)
        assert np.array_equal(L.forward_sequences_dev(buf_d, first_d, steps_d, n).cpu().numpy(), out_h)

        def host_from_tensor():
            host_call(np.ascontiguousarray(buf_d.cpu().numpy().transpose(1, 0, 2)))      # agent-major: the windows back to back
            torch.from_numpy(out_h).cuda()
            stream.synchronize()

        def dev_complete():
            L.forward_sequences_dev(buf_d, first_d, steps_d, n, out=out_d); stream.synchronize()

        us = median_us(dict(host=lambda: host_call(packed), host_from_tensor=host_from_tensor, dev_complete=dev_complete))
        # (the enqueue alone is timed apart, with a synchronisation OUTSIDE the bracket so that the queue does not grow)
        t = []
        for _ in range(calls):
            t0 = time.perf_counter(); L.forward_sequences_dev(buf_d, first_d, steps_d, n, out=out_d); t.append(time.perf_counter() - t0)
            stream.synchronize()
        us["dev_enqueue"] = float(np.median(t) * 1e6)
        # the launches alone, from the library's event timers (apart from the wall-clock loops: the events cost a few microseconds per call)
        L.timing_enable(True)
        k0 = [L.timing_get(k) for k in BRACKETS]
        for _ in range(KERNEL_CALLS):
            host_call(packed)
        for _ in range(KERNEL_CALLS):
            L.forward_sequences_dev(buf_d, first_d, steps_d, n, out=out_d)
        stream.synchronize()
        k1 = [L.timing_get(k) for k in BRACKETS]
        L.timing_enable(False)
        for name, (ms0, c0), (ms1, c1) in zip(BRACKETS, k0, k1):
            us["kernel_" + name] = (ms1 * c1 - ms0 * c0) * 1e3 / KERNEL_CALLS      # all brackets of one call (the timers keep average and count)
        res[str(n)] = us
    L.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.calls, a.warmup)
    assert a.rounds >= 5, "medians of at least five runs"
    runs = []
    for r in range(a.rounds):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--warmup", str(a.warmup)],
                           stdout=subprocess.PIPE, text=True, timeout=300)
        if p.returncode != 0:      # (nothing more is started on the device after a child that failed)
            sys.exit("round %d: the child ended with status %d" % (r, p.returncode))
        runs.append(json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:]))
        print("round %d done" % r, flush=True)

    def stat(vals):
        v = sorted(vals)
        return dict(median=v[len(v) // 2], min=v[0], max=v[-1])

    res = dict(shape=SHAPE, rounds=a.rounds, calls=a.calls, warmup=a.warmup, forward_us={})
    for n in NS:
        res["forward_us"][str(n)] = {k: stat([x[str(n)][k] for x in runs]) for k in COLUMNS}
    # device time of a call's launches: the host call's chains (prepare, product, diagonals up to the longest window, output layer per chunk of
    # staged windows) and the device call's (the same over all 17 steps, windows gathered by the prepare launch)
    res["kernel_us"] = {str(n): {k: stat([x[str(n)]["kernel_" + k] for x in runs]) for k in BRACKETS} for n in NS}
    for n, d in res["forward_us"].items():
        print("n=%5s  " % n + "   ".join("%s %.1f (%.1f .. %.1f)" % (k, v["median"], v["min"], v["max"]) for k, v in d.items()))
    for n, d in res["kernel_us"].items():
        print("n=%5s  " % n + "   ".join("%s %.1f (%.1f .. %.1f)" % (k, v["median"], v["min"], v["max"]) for k, v in d.items()))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
