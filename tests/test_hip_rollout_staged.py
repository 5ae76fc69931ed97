"""hl_rollout_step under the snapshot source (include/smarties_hip_rollout.h: hl_rollout_staging, hl_rollout_stage_info), on the GPU: a
rollout with a staging ring on the acting stream equals the plain live rollout while its snapshot is fresh; order, batches and the wrap of
the ring; the overlapped loop equals its synchronised form; the call does not queue behind a backlog of gradient steps; the refusals and a
change of source with episodes in flight.
(On the commit before the feature every test here ends at the first staging call: the library has no such symbol.)"""
import time

import numpy as np
import pytest

import rollout as R
import rollout_staged as S
from acting import WIDE_SHAPES, _same_replay, _same_training_state, _side_stream, _synth_learner, _wide_cfg
from smarties_amd import capi

pytestmark = pytest.mark.gpu
N_ENV, MAX_STEPS, CALLS = S.N_ENV, S.MAX_STEPS, S.CALLS
RING = 28


def _noise(rng, calls, n_env, L):
    import torch
    if L.nOptions:
        return torch.from_numpy(rng.uniform(size=(calls, n_env))).cuda()
    return torch.from_numpy(np.clip(rng.normal(size=(calls, n_env, L.dA)), -3, 3)).cuda()


def _drive(hip_api, name, source_of_call=None):
    """CALLS calls of the toy simulator on one learner, step(1) after every tenth.  source_of_call None: a plain rollout under the live
    source on torch's current stream.  Else: a rollout with a ring of RING rows, calls on the side stream under source_of_call(call); a
    new snapshot behind every step.  Returns the learner, the rollout, every call's actions and the slabs at calls 19 / 39 / 59"""
    import torch
    kw, sc, n_eps = S.NETS[name]
    L = _synth_learner(hip_api, kw, sc, n_eps=n_eps)
    staged = source_of_call is not None
    roll = L.rollout(N_ENV, MAX_STEPS, seed=1, tag_base=5000, staging_rows=RING if staged else None)
    sim = R.ToySim(N_ENV, L.dS, L.dA, S.LENGTHS)
    noise = _noise(np.random.default_rng(9), CALLS, N_ENV, L)
    stream = _side_stream() if staged else torch.cuda.current_stream()
    torch.cuda.synchronize()
    if staged:
        L.policy_snapshot()
    actions, slabs = [], {}
    with torch.cuda.stream(stream):
        for call in range(CALLS):
            if staged:
                L.act_source(source_of_call(call))
            s, r, end, ended = sim.observe(MAX_STEPS)
            a = roll.step(s, r, end, noise[call], stream=stream)
            actions.append(a)
            sim.advance(a, ended)
            if call % 10 == 9:
                L.step(1)
                if staged:
                    L.policy_snapshot()
            if call in (19, 39, 59):
                slabs[call] = [roll.read(e) for e in range(N_ENV)]
    stream.synchronize(); L.sync()      # (the next learner steps only once this one has finished)
    return L, roll, actions, slabs


def _same_run(a, b):
    import torch
    (A, rollA, actA, slabA), (B, rollB, actB, slabB) = a, b
    for call in range(CALLS):
        assert torch.equal(actA[call], actB[call]), call
    for call in (19, 39, 59):
        for e in range(N_ENV):
            assert slabA[call][e][0] == slabB[call][e][0], (call, e)
            for x, y in zip(slabA[call][e][1:], slabB[call][e][1:]):
                assert np.array_equal(x, y), (call, e)
    assert rollA.info() == rollB.info()
    _same_replay(A, B)
    _same_training_state(A, B)


# ---- 4. snapshot equals live while the snapshot is fresh ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.NETS))
def test_staged_snapshot_rollout_equals_the_live_rollout_while_the_snapshot_is_fresh(hip_api, name):
    a = _drive(hip_api, name)
    b = _drive(hip_api, name, lambda call: "snapshot")
    _same_run(a, b)
    B, roll = b[0], b[1]
    info, stage = roll.info(), roll.stage_info()
    assert info["calls"] == CALLS and info["episodes"] > 10 and info["no_room"] == 0
    assert B.episode_info(0)[0] == 5000 + info["episodes"] - 1      # the newest episode carries the last tag
    assert stage["episodes"] == info["episodes"] and stage["rows"] == info["steps"] and stage["wraps"] >= 1
    want = S.expected_stage_counts(RING, S.toy_schedule(S.LENGTHS, MAX_STEPS, CALLS))
    assert {k: stage[k] for k in want} == want
    assert a[1].stage_info() == dict(capacity=0, batches=0, episodes=0, rows=0, wraps=0, stalls=0)      # the plain rollout has no ring


# ---- 5. order, batches and wrap ----------------------------------------------------------------------------------------------------------
def test_staged_episodes_keep_the_ascending_environment_order_across_batches_and_a_wrap(hip_api):
    """the environments and flags of tests/test_hip_rollout.py's order test, under the snapshot source with a ring of 96 rows: 70
    episodes of 2 states leave in batches of 24, 24 and 22 (48 rows are half the ring), the third starts again at row 0"""
    import torch
    n_env = 1100
    L = _synth_learner(hip_api, S.DENSE16, dict(seed=3, dimS=6, dimA=3, lenMin=5, lenMax=30, pTerm=0.3), n_eps=5)
    before = L.counts()
    roll = L.rollout(n_env, 3, seed=2, tag_base=70000, staging_rows=96)
    perm = np.random.default_rng(3).permutation(n_env)
    fixed = [0, 63, 64, 1023, 1024, 1099]
    chosen = np.array(sorted(fixed + [int(e) for e in perm if e not in fixed][:64]))
    assert chosen.size == 70
    rng = np.random.default_rng(5)
    s = torch.from_numpy(rng.normal(size=(n_env, 6)).astype(np.float32)).cuda()
    r = torch.arange(n_env, dtype=torch.float64, device="cuda")
    end = torch.zeros(n_env, dtype=torch.int32, device="cuda")
    flags = np.zeros(n_env, np.int32)
    flags[chosen] = 1 + (np.arange(70) % 2)      # terminal and truncated in turn
    end1, half = torch.from_numpy(flags).cuda(), s * 0.5
    side = _side_stream()
    torch.cuda.synchronize()
    L.policy_snapshot(); L.act_source("snapshot")
    with torch.cuda.stream(side):
        a0 = roll.step(s, r, end, stream=side)
        assert roll.info()["episodes"] == 0 and bool((a0 != 0).all())
        a1 = roll.step(half, r, end1, stream=side)
        zero = (a1 == 0).all(dim=1).cpu().numpy()
    side.synchronize(); L.sync()
    info, stage = roll.info(), roll.stage_info()
    assert (info["calls"], info["episodes"], info["steps"], info["capped"], info["no_room"]) == (2, 70, 140, 0, 0)
    assert (stage["capacity"], stage["batches"], stage["episodes"], stage["rows"], stage["wraps"]) == (96, 3, 70, 140, 1)
    assert np.array_equal(np.flatnonzero(zero), chosen)
    after = L.counts()
    assert after[1] == before[1] + 70 and after[0] == before[0] + 70
    for k, env in enumerate(chosen):
        pos = 69 - k      # position 0 is the newest episode
        assert L.episode_info(pos) == (70000 + k, 2, int(flags[env] == 1)), (k, env)
        assert L.episode_stats(pos)[0] == np.float32(env), (k, env)


# ---- 6. overlapped equals synchronised ---------------------------------------------------------------------------------------------------
def test_overlapped_staged_loop_equals_its_synchronised_form(hip_api):
    """4 iterations of { 8 rollout calls on the side stream; policy_snapshot; step(5) } around a deterministic elementwise simulator on
    the device.  A: a ring of 2 maxSteps rows and no host synchronisation inside the loop -- the calls of iteration it + 1 run beside the
    steps of iteration it, the ring wraps and may stall.  B: a ring that holds every slab, and a full device synchronisation after every
    call.  Same data flow, so the same bits"""
    import torch
    import torch.nn.functional as F
    kw = dict(dimS=8, dimA=2, bounded=[1, 0], hidden=(32, 32), nnFunc="Tanh", batchSize=8, maxTotObsNum=4000, randSeed=5)
    n_env, T, iters, per, k, dS, dA = 16, 8, 4, 8, 5, 8, 2
    calls = iters * per
    rng = np.random.default_rng(9)
    noise = torch.from_numpy(np.clip(rng.normal(size=(calls, n_env, dA)), -2, 2)).cuda()      # all of it drawn ahead
    start = torch.from_numpy(rng.normal(size=(n_env, dS)).astype(np.float32)).cuda()
    # environment e's episodes have 2 + (e + episode) % 7 states: 2 .. 8, the last by the cap where its flag is left out
    flags, restart = np.zeros((calls, n_env), np.int32), np.zeros((calls, n_env), bool)
    t, ep = np.zeros(n_env, int), np.zeros(n_env, int)
    for c in range(calls):
        for e in range(n_env):
            n_states = 2 + (e + ep[e]) % 7
            if t[e] + 1 == n_states:
                flags[c, e] = 0 if (n_states == T and e % 2) else 1 + (e + ep[e]) % 2
                restart[c, e] = True
                t[e], ep[e] = 0, ep[e] + 1
            else:
                t[e] += 1
    assert restart.sum() > 60 and restart.sum(axis=1).max() >= 3
    flags_d, restart_d = torch.from_numpy(flags).cuda(), torch.from_numpy(restart).cuda()
    side = _side_stream()

    def run(ring_rows, synchronise):
        L = _synth_learner(hip_api, kw, dict(seed=21, dimS=dS, dimA=dA, lenMin=5, lenMax=30, pTerm=0.5), n_eps=10)
        roll = L.rollout(n_env, T, seed=3, tag_base=1000, staging_rows=ring_rows)
        torch.cuda.synchronize()
        L.policy_snapshot(); L.act_source("snapshot")
        actions = []
        with torch.cuda.stream(side):
            s, r = start.clone(), torch.zeros(n_env, dtype=torch.float64, device="cuda")
        for it in range(iters):
            with torch.cuda.stream(side):
                for c in range(it * per, (it + 1) * per):
                    a = roll.step(s, r, flags_d[c], noise[c], stream=side)
                    actions.append(a)
                    nxt = 0.9 * s + 0.1 * torch.tanh(F.pad(a.float(), (0, dS - dA)))
                    r = -(nxt.double() ** 2).sum(dim=1)
                    s = torch.where(restart_d[c][:, None], start + 0.01 * nxt, nxt)
                    if synchronise:
                        torch.cuda.synchronize(); L.sync()
            L.policy_snapshot()
            L.step(k)
        side.synchronize(); L.sync()
        slabs = [roll.read(e) for e in range(n_env)]
        return L, roll, actions, slabs

    A, rollA, actA, slabA = run(2 * T, False)
    A.scalars()                      # no device-side failure code
    B, rollB, actB, slabB = run(n_env * T, True)
    for c in range(calls):
        assert torch.equal(actA[c], actB[c]), c
    assert not torch.equal(actA[per], actA[calls - 1])
    for e in range(n_env):
        assert slabA[e][0] == slabB[e][0], e
        for x, y in zip(slabA[e][1:], slabB[e][1:]):
            assert np.array_equal(x, y), e
    assert rollA.info() == rollB.info() and rollA.info()["episodes"] == int(restart.sum()) and rollA.info()["no_room"] == 0
    sa, sb = rollA.stage_info(), rollB.stage_info()
    assert sa["episodes"] == sb["episodes"] == rollA.info()["episodes"] and sa["wraps"] > sb["wraps"] and sb["stalls"] == 0
    _same_replay(A, B)
    _same_training_state(A, B)
    assert A.counts()[2] == iters * k and A.policy_snapshot_info() == (iters + 1, (iters - 1) * k)


# ---- 7. the call does not queue behind a backlog -----------------------------------------------------------------------------------------
def test_staged_rollout_call_does_not_queue_behind_a_backlog_of_steps(hip_api, capsys):
    """the form of tests/test_hip_act_snapshot.py's backlog test.  6 environments end 6 episodes of 2 states in the timed call; the ring
    has 2 maxSteps = 8 rows, a batch 4 of them: three batches, the third starts again at row 0 while the first is still waiting for its
    ingestion behind 3000 queued steps -- a stall, which holds back the acting stream's next launch and not the caller's stream"""
    import torch
    dense = dict(dimS=17, dimA=6, hidden=(64, 64), batchSize=32, maxTotObsNum=4096, randSeed=3)
    L = _synth_learner(hip_api, dense, dict(seed=21, dimS=17, dimA=6, lenMin=5, lenMax=30, pTerm=0.5), n_eps=40)
    n_env, T = 6, 4
    rolls = {"snapshot": L.rollout(n_env, T, seed=1, tag_base=100000, staging_rows=2 * T), "live": L.rollout(n_env, T, seed=1, tag_base=200000)}
    side = _side_stream()
    rng = np.random.default_rng(4)
    s = torch.from_numpy(rng.normal(size=(n_env, 17)).astype(np.float32)).cuda()
    r = torch.arange(n_env, dtype=torch.float64, device="cuda")
    run_on = torch.zeros(n_env, dtype=torch.int32, device="cuda")
    all_end = torch.tensor([1, 2, 1, 2, 1, 2], dtype=torch.int32, device="cuda")
    out = torch.empty((n_env, 6), dtype=torch.float64, device="cuda")
    L.step(990)      # (the 1000th, 2000th and 3000th step of a learner sweep the replay and may wait for the device: the backlog below ends 990 steps behind one)
    L.policy_snapshot()
    for src in ("snapshot", "live"):      # both sources warmed up with each rollout's first state: scratch, the acting stream
        L.act_source(src)
        with torch.cuda.stream(side):
            rolls[src].step(s, r, run_on, out=out, stream=side)
    L.prepare_steps(100)
    side.synchronize(); L.sync()
    stamps = {}
    for src in ("snapshot", "live"):
        L.act_source(src)
        n_before = L.counts()[1]
        for _ in range(30):
            L.step(100)
        t0 = time.perf_counter()
        with torch.cuda.stream(side):
            rolls[src].step(s, r, all_end, out=out, stream=side)
        side.synchronize()
        t1 = time.perf_counter() - t0
        L.sync()
        t2 = time.perf_counter() - t0
        stamps[src] = (t1, t2)
        # after the sync all episodes are in the replay, in order
        info = rolls[src].info()
        assert (info["calls"], info["episodes"], info["steps"], info["no_room"]) == (2, n_env, 2 * n_env, 0), (src, info)
        assert L.counts()[1] == n_before + n_env
        base = {"snapshot": 100000, "live": 200000}[src]
        for e in range(n_env):
            pos = n_env - 1 - e
            assert L.episode_info(pos) == (base + e, 2, int(e % 2 == 0)), (src, e)
            assert L.episode_stats(pos)[0] == np.float32(e), (src, e)
    stage = rolls["snapshot"].stage_info()
    with capsys.disabled():
        print("\nrollout call behind 3000 queued steps, seconds until (the side stream, hl_sync) returned: %r; staging: %r" % (stamps, stage))
    t1, t2 = stamps["snapshot"]
    assert t1 < t2 / 2, stamps
    t1, t2 = stamps["live"]
    assert t1 >= t2 / 2, stamps      # the parent's behaviour: the test discriminates, and a backlog existed
    assert (stage["batches"], stage["episodes"], stage["rows"], stage["wraps"]) == (3, n_env, 2 * n_env, 1)
    assert stage["stalls"] >= 1, stage
    assert rolls["live"].stage_info()["batches"] == 0
    L.scalars()                      # no device-side failure code


# ---- 8. refusals, and a change of source with episodes in flight ---------------------------------------------------------------------------
def test_refusals_of_the_staging_calls(hip_api):
    import torch
    G = _synth_learner(hip_api, S.LSTM, S.SYNTH6, n_eps=10)
    roll = G.rollout(4, 5)
    for rows in (9, 0, -1, 2**31):
        with pytest.raises(capi.HlError) as e:
            roll.staging(rows)
        assert e.value.status == 1, rows                                       # HL_ERR_BAD_ARG: fewer than 2 maxSteps rows, 2^31 and more
    assert roll.stage_info()["capacity"] == 0
    roll.staging(10)
    assert roll.stage_info() == dict(capacity=10, batches=0, episodes=0, rows=0, wraps=0, stalls=0)
    with pytest.raises(capi.HlError) as e:
        roll.staging(20)
    assert e.value.status == 4                                                 # HL_ERR_STATE: it has a ring
    s = torch.zeros((4, 6), dtype=torch.float32, device="cuda")
    r = torch.zeros(4, dtype=torch.float64, device="cuda")
    end = torch.zeros(4, dtype=torch.int32, device="cuda")
    G.act_source("snapshot")
    with pytest.raises(capi.HlError) as e:
        roll.step(s, r, end)
    assert e.value.status == 4 and "hl_policy_snapshot" in str(e.value)         # before any snapshot
    assert roll.info()["calls"] == 0
    G.policy_snapshot()
    G.step_begin()
    with pytest.raises(capi.HlError) as e:
        roll.step(s, r, end)
    assert e.value.status == 4                                                 # between the two halves of a step
    G.step_end()
    assert roll.info()["calls"] == 0
    assert bool(torch.isfinite(roll.step(s, r, end)).all())
    bare = G.rollout(4, 5)
    with pytest.raises(capi.HlError) as e:
        bare.step(s, r, end)                                                   # a rollout without a ring: refused as before
    assert e.value.status == 8 and "HL_ACT_LIVE" in str(e.value)
    assert roll.info()["calls"] == 1 and bare.info()["calls"] == 0
    # a recurrent net on wide inputs acts over the training buffers: no ring, the live source only
    W = _synth_learner(hip_api, _wide_cfg(WIDE_SHAPES[0]), None, n_eps=0)
    wide = W.rollout(4, 5)
    with pytest.raises(capi.HlError) as e:
        wide.staging(10)
    assert e.value.status == 8 and "HL_ACT_LIVE" in str(e.value)
    assert wide.stage_info()["capacity"] == 0
    # hl_destroy with a staged rollout still open releases ring and events with it
    G.close()
    with pytest.raises(ValueError):
        roll.stage_info()


def test_a_change_of_source_with_episodes_in_flight_reproduces_the_live_rollout(hip_api):
    """calls 0 .. 19 under the snapshot source, 20 .. 39 live, 40 .. 59 snapshot, all on the side stream, against the plain live rollout:
    at both changes environments are in the middle of an episode and earlier ones are still on their way through the ring"""
    name = "lstm-16x16-bptt3"
    a = _drive(hip_api, name)
    b = _drive(hip_api, name, lambda call: "live" if 20 <= call < 40 else "snapshot")
    _same_run(a, b)
    sched = S.toy_schedule(S.LENGTHS, MAX_STEPS, CALLS)
    assert any(sched[c] for c in (19, 20, 39, 40))
    stage = b[1].stage_info()
    staged = sum(len(x) for c, x in enumerate(sched) if not 20 <= c < 40)
    assert stage["episodes"] == staged and 0 < staged < b[1].info()["episodes"]      # the live calls staged nothing
