"""Acting on a policy snapshot while gradient steps run (include/smarties_hip_dev.h: hl_policy_snapshot, hl_policy_snapshot_info,
hl_act_dev_source; smarties_amd/csrc/learner_dev.h, actdev.hip: policy_snapshot_kernel), on the GPU: the snapshot source's outputs are the
live source's at snapshot time bit for bit, on every route the device calls take; a snapshot holds its own standardisation; acting from
it needs no host wait and leaves training as it was; the overlapped loop act | append -> snapshot -> step equals its serial restatement;
an acting call does not queue behind a backlog of steps; the refusals.
(On the commit before the feature every test here ends at the first call: the library has no such symbol.)"""
import time

import numpy as np
import pytest

from acting import _same_replay, _same_training_state, _side_stream
from oracle_api import fill_synth, synth_cfg
from smarties_amd import capi

pytestmark = pytest.mark.gpu

DENSE = dict(dimS=17, dimA=6, hidden=(64, 64), batchSize=32, maxTotObsNum=4096, randSeed=3)
# net -> (configuration, SMARTIES_HIP_GENERIC or None, [(kind, n, longest window, row_stride)]): the smallest nets that take each route
NETS = {
    # n = 5: the one-kernel route (a workgroup per row); n = 80: the row-block route, five blocks of 16 rows
    "dense": (DENSE, None, [("rows", 5, 0, 0), ("rows", 80, 0, 0)]),
    # appended observations: act_stack_dev_kernel in front, windows shorter than the stack, exactly it, longer
    "stacked": (dict(dimS=6, dimA=2, bounded=[1, 0], nAppendedObs=2, hidden=(32,), nnFunc="Tanh", batchSize=8, maxTotObsNum=4000, randSeed=5),
                None, [("windows", 7, 5, 7)]),
    "discrete": (dict(dimS=6, dimA=1, bounded=[0], adv_kind=capi.ADV_DISCRETE, n_options=5, hidden=(32, 32), nnFunc="Tanh", batchSize=8,
                      maxTotObsNum=4000, randSeed=5), None, [("rows", 37, 0, 0)]),
    # the batched window kernel; windows of 1 .. 8 states against nnBPTTseq + 1 = 5: truncation is included
    "lstm": (dict(dimS=6, dimA=2, bounded=[1, 0], hidden=(16, 16), nnFunc="Tanh", batchSize=16, maxTotObsNum=5000, randSeed=51,
                  adv_kind=capi.ADV_GAUSSIAN, nn_type=capi.NN_LSTM, nnBPTTseq=4), None, [("windows", 9, 8, 3)]),
    # the two-layer strided net of tests/test_hip_act_conv_dev.py: the conv-stack kernel, then the row-block kernel on the feature rows
    "conv": (dict(dimS=576, dimA=2, bounded=[1, 0], conv=[(12, 12, 4, 8, 3, 1), (10, 10, 8, 16, 4, 2)], hidden=(32,), nnFunc="Tanh",
                  batchSize=8, maxTotObsNum=1500, randSeed=5), None, [("windows", 5, 3, 2)]),
    # the panelled row-block kernel (panels of 64 columns are forced; 17 inputs: one partial panel), two blocks of rows
    "panelled": (DENSE, "8192", [("rows", 20, 0, 0)]),
}


def _learner(hip_api, kw, n_eps=30):
    L = capi.Learner(hip_api, capi.make_config(**kw))
    L.init_weights()
    if n_eps:
        fill_synth(L, synth_cfg(seed=21, dimS=kw["dimS"], dimA=kw["dimA"], lenMin=5, lenMax=30, pTerm=0.5), n_eps)
        L.initialize()
    return L


def _inputs(L, calls, seed=7):
    """device tensors of every call of a net, made once: rows [n][dIn], or a strided buffer in which window i of 1 + i % longest states
    starts at row i longest stride + i % stride; the noise of the head"""
    import torch
    rng = np.random.default_rng(seed)
    out = []
    for kind, n, longest, stride in calls:
        noise = rng.uniform(size=n) if L.nOptions else np.clip(rng.normal(size=(n, L.dA)), -2, 2)
        if kind == "rows":
            arrs = ((rng.normal(size=(n, L.dIn)) * 1.5 + 0.2).astype(np.float32),)
        else:
            states = (rng.normal(size=(n * longest * stride + stride, L.dS)) * 1.5 + 0.2).astype(np.float32)
            first = np.array([i * longest * stride + i % stride for i in range(n)], np.int64)
            arrs = (states, first, np.array([1 + i % longest for i in range(n)], np.int32))
        out.append((kind, stride, [torch.from_numpy(a).cuda() for a in arrs], torch.from_numpy(noise).cuda()))
    torch.cuda.synchronize()
    return out


def _act(L, inputs, side):
    """every acting call of the net on the side stream -- the forward call, the head with noise and its evaluation form --: a flat list
    of numpy arrays, read in that stream's order"""
    import torch
    res = []
    with torch.cuda.stream(side):
        for kind, stride, arrs, noise in inputs:
            if kind == "rows":
                got = [L.forward_dev(arrs[0], stream=side)]
                got += list(L.select_actions_dev(arrs[0], noise, stream=side)) + list(L.select_actions_dev(arrs[0], None, stream=side))
            else:
                st, first, n_steps = arrs
                got = [L.forward_sequences_dev(st, first, n_steps, stride, stream=side)]
                got += list(L.select_actions_sequences_dev(st, first, n_steps, stride, noise, stream=side))
                got += list(L.select_actions_sequences_dev(st, first, n_steps, stride, None, stream=side))
            res += [t.cpu().numpy() for t in got]
    return res


def _equal(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. the snapshot source gives the live outputs of snapshot time, on every route ----------------------------------------------------
@pytest.mark.parametrize("name", list(NETS))
def test_snapshot_outputs_are_the_live_outputs_at_snapshot_time(hip_api, name, monkeypatch):
    kw, generic, calls = NETS[name]
    monkeypatch.delenv("SMARTIES_HIP_GENERIC", raising=False)
    if generic:
        monkeypatch.setenv("SMARTIES_HIP_GENERIC", generic)      # read when the learner is created
    L = _learner(hip_api, kw)
    side, inputs = _side_stream(), _inputs(L, calls)
    L.step(3)
    ref = _act(L, inputs, side)
    assert all(np.isfinite(x).all() for x in ref)
    assert L.policy_snapshot_info() == (0, -1)
    L.policy_snapshot()
    assert L.policy_snapshot_info() == (1, 3)
    L.step(5)
    after = _act(L, inputs, side)
    assert not np.array_equal(after[0], ref[0]), "five steps left the outputs as they were: the comparison below would show nothing"
    L.act_source("snapshot")
    got = _act(L, inputs, side)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g, r), (name, i)
    assert _equal(_act(L, inputs, side), ref)                  # ... and again, from the scratch the first pass left
    L.act_source("live")
    assert _equal(_act(L, inputs, side), after)
    assert L.policy_snapshot_info() == (1, 3) and L.counts()[2] == 8      # the lag an RL user logs: 8 - 3 steps
    L.policy_snapshot()                                        # the other buffer; the one just read is left alone
    assert L.policy_snapshot_info() == (2, 8)
    L.act_source("snapshot")
    assert _equal(_act(L, inputs, side), after)
    L.sync()


# ---- 2. a snapshot holds its own standardisation ---------------------------------------------------------------------------------------
def test_snapshot_holds_its_own_standardisation_and_weights(hip_api):
    L = _learner(hip_api, DENSE)
    side, inputs = _side_stream(), _inputs(L, NETS["dense"][2])
    L.step(3)
    ref = _act(L, inputs, side)
    L.policy_snapshot()
    m, s, r = L.get_scaling()
    L.set_scaling(m + np.float32(0.75), s * np.float32(0.5), r)
    L.act_source("snapshot")
    assert _equal(_act(L, inputs, side), ref)
    L.act_source("live")
    live = _act(L, inputs, side)
    assert not np.array_equal(live[0], ref[0])
    w, m1, m2 = L.get_params()
    L.set_params(w * np.float32(0.5), m1, m2)                  # ... and its own weights
    L.act_source("snapshot")
    assert _equal(_act(L, inputs, side), ref)
    L.act_source("live")
    assert not np.array_equal(_act(L, inputs, side)[0], live[0])


# ---- 3. no host wait, and training is unchanged ----------------------------------------------------------------------------------------
def test_acting_from_snapshots_between_queued_steps_leaves_training_unchanged(hip_api):
    import torch
    A, B = _learner(hip_api, DENSE), _learner(hip_api, DENSE)
    side, inputs = _side_stream(), _inputs(A, [("rows", 80, 0, 0)])
    st, noise = inputs[0][2][0], inputs[0][3]

    def act(L):      # tensors: nothing is read back here
        with torch.cuda.stream(side):
            return [L.forward_dev(st, stream=side)] + list(L.select_actions_dev(st, noise, stream=side))

    A.act_source("snapshot")
    outA = []
    A.policy_snapshot(); A.step(4); outA.append(act(A))
    A.policy_snapshot(); A.step(4); outA.append(act(A))
    A.policy_snapshot(); outA.append(act(A))
    assert A.policy_snapshot_info() == (3, 8)
    side.synchronize(); A.sync()      # A's first host wait (and B steps only once A has finished: one stepping learner per device at a time)
    outB = []
    outB.append(act(B)); B.sync(); B.step(4)
    outB.append(act(B)); B.sync(); B.step(4)
    outB.append(act(B)); B.sync()
    side.synchronize()
    for k, (a, b) in enumerate(zip(outA, outB)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), k
    assert not torch.equal(outA[0][0], outA[1][0]) and not torch.equal(outA[1][0], outA[2][0])
    _same_training_state(A, B)                                 # weights, both moments, the generator, beta
    assert bytes(A.scalars()) == bytes(B.scalars())            # (hl_get_scalars fails on a device-side failure code)
    A.step(2); A.sync(); B.step(2)
    _same_training_state(A, B)


# ---- 4. the overlapped loop equals its serial restatement ------------------------------------------------------------------------------
_INGEST = []


def _ingest_stream():
    import torch
    if not _INGEST:      # (one for the file, as _side_stream: a used stream keeps a hardware queue of the process)
        _INGEST.append(torch.cuda.Stream())
    return _INGEST[0]


def test_overlapped_loop_equals_its_serial_restatement(hip_api):
    """Pipeline A, per iteration `it`: act rollout it + 1 from the snapshot on the `act` stream (beside the steps queued by iteration
    it - 1) | append(it) on the `ingest` stream -> policy_snapshot() -> step(k).  The snapshot an iteration acts from was taken by the
    iteration before, between that iteration's append and its steps: the policy is one call stale.  Serial B has the same data flow with
    live acting, so it acts rollout it + 2 where A takes the snapshot rollout it + 2 is acted from: append(it) -> act rollout it + 2 ->
    step(k), rollouts 0 and 1 acted before the loop.  (Acting rollout it + 1 at that point instead would hand B a policy k steps fresher
    than A's: another data flow, not a restatement.)"""
    import torch
    import torch.nn.functional as F
    kw = dict(dimS=8, dimA=2, bounded=[1, 0], hidden=(32, 32), nnFunc="Tanh", batchSize=8, maxTotObsNum=4000, randSeed=5)
    nEnv, T, iters, k, dS, dA = 16, 8, 4, 5, 8, 2
    A, B = _learner(hip_api, kw, n_eps=10), _learner(hip_api, kw, n_eps=10)
    rng = np.random.default_rng(9)
    noise = torch.from_numpy(np.clip(rng.normal(size=(iters + 1, T, nEnv, dA)), -2, 2)).cuda()      # all of it drawn ahead
    start = torch.from_numpy(rng.normal(size=(nEnv, dS)).astype(np.float32)).cuda()

    def buffers():      # two rollout buffers [T + 1][nEnv]: states, actions, policies, rewards, values, advantages
        z = lambda shape, dt: torch.zeros((T + 1, nEnv) + shape, dtype=dt, device="cuda")
        return [(z((dS,), torch.float32), z((dA,), torch.float64), z((2 * dA,), torch.float64), z((), torch.float64), z((), torch.float32),
                 z((), torch.float32)) for _ in range(2)]

    def rollout(L, bufs, r, stream):      # the deterministic elementwise simulator, on the current stream
        S, Ac, MU, R, V, ADV = bufs[r % 2]
        S[0] = start if r == 0 else bufs[(r - 1) % 2][0][T]
        for t in range(T):
            L.select_actions_dev(S[t], noise[r, t], out=(Ac[t], MU[t], V[t], ADV[t]), stream=stream)
            S[t + 1] = 0.9 * S[t] + 0.1 * torch.tanh(F.pad(Ac[t].float(), (0, dS - dA)))
            R[t + 1] = -(S[t + 1].double() ** 2).sum(dim=1)

    def append(L, bufs, it, stream):
        S, Ac, MU, R, V, ADV = bufs[it % 2]
        L.append_episodes_dev([T + 1] * nEnv, [1] * nEnv, [1000 + it * nEnv + e for e in range(nEnv)], list(range(nEnv)), nEnv,
                              S, Ac, MU, R, V, ADV, stream=stream)

    bufA, bufB = buffers(), buffers()
    torch.cuda.synchronize()
    # A: overlapped
    act, ingest = _side_stream(), _ingest_stream()
    rolled = [torch.cuda.Event() for _ in range(iters + 1)]
    appended = [torch.cuda.Event() for _ in range(iters)]
    A.policy_snapshot()
    A.act_source("snapshot")
    with torch.cuda.stream(act):
        rollout(A, bufA, 0, act)
        rolled[0].record(act)
    for it in range(iters):
        with torch.cuda.stream(act):
            if it >= 1:
                act.wait_event(appended[it - 1])               # rollout it + 1 takes the buffer append(it - 1) read
            rollout(A, bufA, it + 1, act)
            rolled[it + 1].record(act)
        with torch.cuda.stream(ingest):
            ingest.wait_event(rolled[it])
            append(A, bufA, it, ingest)
            appended[it].record(ingest)
        A.policy_snapshot()
        A.step(k)
    assert A.policy_snapshot_info() == (iters + 1, (iters - 1) * k)
    act.synchronize(); ingest.synchronize(); A.sync()          # (B steps only once A has finished: one stepping learner per device at a time)
    # B: serial, live, everything on torch's current stream
    cur = torch.cuda.current_stream()
    rollout(B, bufB, 0, cur)
    rollout(B, bufB, 1, cur)
    for it in range(iters):
        append(B, bufB, it, cur)
        if it + 2 <= iters:
            rollout(B, bufB, it + 2, cur)
        B.step(k)
    act.synchronize(); ingest.synchronize(); torch.cuda.synchronize(); A.sync(); B.sync()
    for a, b in zip(bufA, bufB):                               # rollouts iters - 1 and iters as the buffers hold them
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert not torch.equal(bufA[0][1][:T], bufA[1][1][:T])
    _same_training_state(A, B)
    assert A.counts() == B.counts() and A.counts()[2] == iters * k
    _same_replay(A, B)                                         # every stored episode, the last one among them


# ---- 5. acting does not queue behind training ------------------------------------------------------------------------------------------
def test_snapshot_acting_does_not_queue_behind_a_backlog_of_steps(hip_api, capsys):
    import torch
    L = _learner(hip_api, DENSE, n_eps=40)
    side, inputs = _side_stream(), _inputs(L, [("rows", 64, 0, 0)])
    st, noise = inputs[0][2][0], inputs[0][3]
    out = L.select_actions_dev(st, noise)
    L.step(990)      # (the 1000th, 2000th and 3000th step of a learner sweep the replay and may wait for the device: the backlog below ends 990 steps behind one)
    L.policy_snapshot()
    for src in ("snapshot", "live"):      # both sources warmed up: scratch, the acting stream
        L.act_source(src)
        with torch.cuda.stream(side):
            L.select_actions_dev(st, noise, out=out, stream=side)
    L.prepare_steps(100)
    side.synchronize(); L.sync()
    stamps = {}
    for src in ("snapshot", "live"):
        L.act_source(src)
        for _ in range(30):
            L.step(100)
        t0 = time.perf_counter()
        with torch.cuda.stream(side):
            L.select_actions_dev(st, noise, out=out, stream=side)
        side.synchronize()
        t1 = time.perf_counter() - t0
        L.sync()
        t2 = time.perf_counter() - t0
        stamps[src] = (t1, t2)
    with capsys.disabled():
        print("\nacting behind 3000 queued steps, seconds until (the side stream, hl_sync) returned: %r" % (stamps,))
    t1, t2 = stamps["snapshot"]
    assert t1 < t2 / 2, stamps
    t1, t2 = stamps["live"]
    assert t1 >= t2 / 2, stamps      # the test discriminates, and a backlog existed
    L.scalars()                      # no device-side failure code


def test_the_first_snapshot_call_runs_on_the_acting_stream(hip_api):
    """The acting stream is created inside the first call under the snapshot source, and that call's launches must already run on it --
    not on the legacy default stream, which a context built before the stream existed would name.  The default stream waits for the
    work of every BLOCKING stream of the process; torch's and the library's streams are all non-blocking, so the test makes one through
    the HIP runtime the process holds, queues about half a second of products on it, and the first call must be done while they run.
    An LSTM's window call: it allocates nothing (an allocation waits for the default stream whatever stream the launches take)."""
    import ctypes as C
    import torch
    kw, _, calls = NETS["lstm"]
    L = _learner(hip_api, kw)
    side, inputs = _side_stream(), _inputs(L, calls)
    stride, (st, first, n_steps) = inputs[0][1], inputs[0][2]
    out = torch.empty((n_steps.numel(), L.nOut), dtype=torch.float64, device="cuda")
    L.step(2)
    want = L.forward_sequences_dev(st, first, n_steps, stride).cpu().numpy()
    L.policy_snapshot()
    L.act_source("snapshot")
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))      # (the copy already mapped)
    raw = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(raw)) == 0
    blocking = torch.cuda.ExternalStream(raw.value)
    a = torch.randn((4096, 4096), device="cuda")
    b, c = torch.eye(4096, device="cuda"), torch.empty_like(a)
    with torch.cuda.stream(blocking):
        torch.mm(a, b, out=c)
    L.sync(); torch.cuda.synchronize()
    with torch.cuda.stream(blocking):
        for _ in range(400):
            torch.mm(a, b, out=c)
    with torch.cuda.stream(side):
        L.forward_sequences_dev(st, first, n_steps, stride, out=out, stream=side)      # the FIRST call under the snapshot source
    side.synchronize()
    busy = not blocking.query()
    blocking.synchronize()
    assert hip.hipStreamDestroy(raw) == 0
    assert np.array_equal(out.cpu().numpy(), want)
    assert busy, "the first snapshot call waited for a blocking stream's work: it ran on the default stream"


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_snapshot_source_refusals(hip_api):
    import torch
    G = _learner(hip_api, DENSE)
    st = torch.zeros((3, G.dIn), dtype=torch.float32, device="cuda")
    G.act_source("snapshot")
    for call in (lambda: G.forward_dev(st), lambda: G.select_actions_dev(st)):
        with pytest.raises(capi.HlError) as e:
            call()                                            # before any snapshot
        assert e.value.status == 4 and "hl_policy_snapshot" in str(e.value)
    assert hip_api.fn("act_dev_source")(G.h, 2) == 1          # an unknown source: HL_ERR_BAD_ARG
    with pytest.raises(capi.HlError) as e:
        G.act_source(-1)
    assert e.value.status == 1
    with pytest.raises(ValueError):
        G.act_source("stale")
    G.policy_snapshot()
    assert torch.isfinite(G.forward_dev(st)).all()            # the source set above held through the refused ones
    G.step_begin()
    with pytest.raises(capi.HlError) as e:
        G.forward_dev(st)
    assert e.value.status == 4                                # HL_ERR_STATE, as for the live source
    G.step_end()
    assert G.forward_dev(torch.empty((0, G.dIn), dtype=torch.float32, device="cuda")).shape == (0, G.nOut)      # n == 0: HL_OK
    assert torch.isfinite(G.forward_dev(st)).all()
    with pytest.raises(capi.HlError) as e:                    # a net the live source refuses is refused alike
        G.forward_sequences_dev(st, torch.zeros(3, dtype=torch.int64, device="cuda"), torch.ones(3, dtype=torch.int32, device="cuda"), 0)
    assert e.value.status == 1                                # row_stride below 1
    # recurrent nets on wide inputs act over the training buffers: the live source only
    W = _learner(hip_api, dict(dimS=272, dimA=2, bounded=[1, 0], hidden=(16, 16), nnFunc="Tanh", batchSize=6, maxTotObsNum=8000, randSeed=5,
                               nn_type=capi.NN_LSTM, adv_kind=capi.ADV_GAUSSIAN, nnBPTTseq=3), n_eps=20)
    states = torch.from_numpy(np.random.default_rng(1).normal(size=(12, 272)).astype(np.float32)).cuda()
    first = torch.tensor([0, 4, 8], dtype=torch.int64, device="cuda")
    n_steps = torch.tensor([1, 4, 3], dtype=torch.int32, device="cuda")
    W.policy_snapshot()
    W.act_source("snapshot")
    for call in (lambda: W.forward_sequences_dev(states, first, n_steps, 1), lambda: W.select_actions_sequences_dev(states, first, n_steps, 1)):
        with pytest.raises(capi.HlError) as e:
            call()
        assert e.value.status == 8 and "HL_ACT_LIVE" in str(e.value)
    W.act_source("live")
    assert torch.isfinite(W.forward_sequences_dev(states, first, n_steps, 1)).all()
    R = _learner(hip_api, NETS["lstm"][0], n_eps=0)            # a net the row calls refuse under either source
    R.act_source("snapshot")
    with pytest.raises(capi.HlError) as e:
        R.forward_dev(torch.zeros((3, R.dIn), dtype=torch.float32, device="cuda"))
    assert e.value.status == 8
