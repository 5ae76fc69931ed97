"""The rollout buffer of a vectorised simulator on the learner's GPU (include/smarties_hip_rollout.h): hl_rollout_step against the loop
written by hand over hl_select_actions_sequences_dev and hl_append_episodes_dev, the order and the chunks of the ingestion, the library's
noise against its numpy restatement, the two flags, training left untouched, the refusals."""
import numpy as np
import pytest

import rollout as R
from acting import FALLBACK, _rec_cfg, _same_replay, _same_training_state, _synth_learner
from smarties_amd import capi

LSTM = dict(dimS=6, dimA=2, bounded=[1, 0], hidden=(16, 16), nnFunc="Tanh", batchSize=8, maxTotObsNum=4000, randSeed=5,
            nn_type=capi.NN_LSTM, nnBPTTseq=3)
SYNTH6 = dict(seed=21, dimS=6, dimA=2, lenMin=5, lenMax=30, pTerm=0.5)
DENSE16 = dict(dimS=6, dimA=3, bounded=[0, 0, 0], hidden=(16,), nnFunc="Tanh", batchSize=8, maxTotObsNum=8000, randSeed=5)
DISCRETE = dict(dimS=6, dimA=1, bounded=[0], hidden=(32, 32), nnFunc="Tanh", batchSize=8, maxTotObsNum=4000, randSeed=5,
                adv_kind=capi.ADV_DISCRETE, n_options=4)
# name -> (configuration, synthetic replay, episodes)
LOOP_NETS = {
    "lstm-16x16-bptt3": (LSTM, SYNTH6, 10),      # the window (4 states) is shorter than the episodes
    "lstm-16x16-app2": (dict(LSTM, nAppendedObs=2), SYNTH6, 10),
    "dense-24x16-app3": (dict(dimS=9, dimA=3, bounded=[0, 1, 0], hidden=(24, 16), nnFunc="Tanh", batchSize=8, maxTotObsNum=4000, randSeed=5,
                              nAppendedObs=3), dict(seed=3, dimS=9, dimA=3, lenMin=5, lenMax=30, pTerm=0.3), 10),
    "discrete-4": (DISCRETE, dict(seed=21, dimS=6, dimA=1, lenMin=5, lenMax=30, pTerm=0.5), 10),
    # the "strided" net of tests/test_hip_act_conv_dev.py: 8 channels (half a channel tile), stride 2
    "conv-strided": (dict(dimA=2, bounded=[1, 0], batchSize=8, maxTotObsNum=1500, randSeed=5, dimS=576,
                          conv=[(12, 12, 4, 8, 3, 1), (10, 10, 8, 16, 4, 2)], hidden=(32,), nnFunc="Tanh"),
                     dict(seed=21, dimS=576, dimA=2, lenMin=4, lenMax=12, pTerm=0.5), 30),
}
N_ENV, MAX_STEPS = 5, 7
# per environment the (states, end flag) of its episodes, gone round; (0, 0): never flagged, so the cap closes it at 7.  Environments 0 and 3
# end together in the third call; lengths 2 .. 7, terminal and truncated ends mixed; (7, 1): a flag on the cap's own step
LENGTHS = [[(3, 1), (5, 2), (2, 1), (7, 2)], [(4, 2), (4, 1), (6, 1)], [(0, 0)], [(3, 1), (2, 2), (7, 1), (5, 1)], [(6, 2), (3, 1), (4, 2)]]


def _noise(rng, calls, n_env, L):
    import torch
    if L.nOptions:
        return torch.from_numpy(rng.uniform(size=(calls, n_env))).cuda()
    return torch.from_numpy(np.clip(rng.normal(size=(calls, n_env, L.dA)), -3, 3)).cuda()


def _same_slabs(roll, hand, n_env):
    import torch
    lens = hand.len.cpu().numpy()
    for e in range(n_env):
        got = roll.read(e)
        assert got[0] == lens[e], e
        for g, w in zip(got[1:], hand.slab(e)):
            assert np.array_equal(g, w), e


# ---- 1. the loop equals the loop written by hand ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LOOP_NETS))
def test_rollout_step_equals_the_loop_over_the_existing_calls_bit_for_bit(hip_api, name):
    import torch
    kw, sc, n_eps = LOOP_NETS[name]
    A, B = [_synth_learner(hip_api, kw, sc, n_eps=n_eps) for _ in range(2)]
    roll, hand = A.rollout(N_ENV, MAX_STEPS, seed=1, tag_base=5000), R.HandLoop(B, N_ENV, MAX_STEPS, tag_base=5000)
    sim = R.ToySim(N_ENV, A.dS, A.dA, LENGTHS)
    noise = _noise(np.random.default_rng(9), 60, N_ENV, A)
    together = 0
    for call in range(60):
        s, r, end, ended = sim.observe(MAX_STEPS)
        together += sum(ended) >= 2
        a = roll.step(s, r, end, noise[call])
        b = hand.step(s, r, end, noise[call])
        assert torch.equal(a, b), call
        assert all(bool((a[e] == 0).all()) == ended[e] for e in range(N_ENV)), call
        sim.advance(a, ended)
        if call % 10 == 9:
            A.step(1); B.step(1)
        if call in (19, 39, 59):
            _same_slabs(roll, hand, N_ENV)
    assert together >= 1
    info = roll.info()
    assert info["calls"] == 60 and info["episodes"] == hand.k > 10 and info["capped"] == hand.capped >= 8 and info["no_room"] == 0
    _same_replay(A, B)
    _same_training_state(A, B)
    assert A.episode_info(0)[0] == 5000 + hand.k - 1      # the newest episode carries the last tag


# ---- 2. order and chunks of the ingestion ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_episodes_are_ingested_in_ascending_environment_order_across_chunks(hip_api):
    """1100 environments (more than one pass of the bookkeeping workgroup), 70 of them -- more than one ingest launch holds -- end in the
    second call: the replay's 70 newest episodes carry consecutive tags in ascending environment order (the terminal reward names the
    environment)"""
    import torch
    n_env = 1100
    L = _synth_learner(hip_api, DENSE16, dict(seed=3, dimS=6, dimA=3, lenMin=5, lenMax=30, pTerm=0.3), n_eps=5)
    before = L.counts()
    roll = L.rollout(n_env, 3, seed=2, tag_base=70000)
    perm = np.random.default_rng(3).permutation(n_env)
    fixed = [0, 63, 64, 1023, 1024, 1099]
    chosen = np.array(sorted(fixed + [int(e) for e in perm if e not in fixed][:64]))
    assert chosen.size == 70
    rng = np.random.default_rng(5)
    s = torch.from_numpy(rng.normal(size=(n_env, 6)).astype(np.float32)).cuda()
    r = torch.arange(n_env, dtype=torch.float64, device="cuda")
    end = torch.zeros(n_env, dtype=torch.int32, device="cuda")
    a0 = roll.step(s, r, end)
    assert roll.info()["episodes"] == 0 and bool((a0 != 0).all())
    flags = np.zeros(n_env, np.int32)
    flags[chosen] = 1 + (np.arange(70) % 2)      # terminal and truncated in turn
    a1 = roll.step(s * 0.5, r, torch.from_numpy(flags).cuda())
    info = roll.info()
    assert (info["calls"], info["episodes"], info["steps"], info["capped"], info["no_room"]) == (2, 70, 140, 0, 0)
    zero = (a1 == 0).all(dim=1).cpu().numpy()
    assert np.array_equal(np.flatnonzero(zero), chosen)
    after = L.counts()
    assert after[1] == before[1] + 70 and after[0] == before[0] + 70
    for k, env in enumerate(chosen):
        pos = 69 - k      # position 0 is the newest episode
        assert L.episode_info(pos) == (70000 + k, 2, int(flags[env] == 1)), (k, env)
        assert L.episode_stats(pos)[0] == np.float32(env), (k, env)


# ---- 3. the library's noise -----------------------------------------------------------------------------------------------------------------
def _given_weights(L, seed=1):
    w = np.random.default_rng(seed).uniform(-0.1, 0.1, L.get_params()[0].shape).astype(np.float32)
    L.set_params(w, np.zeros_like(w), np.zeros_like(w))


def _drive(roll, n_env, calls, ends, dS, seed):
    """`calls` steps of a rollout with the library's noise; ends: {call: environments flagged terminal}.  Per call and environment
    (episode, t, row of actions, row of policies) of the running ones, read from the slabs"""
    import torch
    rng = np.random.default_rng(seed)
    episode, t = [0] * n_env, [0] * n_env
    seen = []
    for call in range(calls):
        flags = np.zeros(n_env, np.int32)
        flags[list(ends.get(call, ()))] = 1
        s = torch.from_numpy(rng.normal(size=(n_env, dS)).astype(np.float32)).cuda()
        roll.step(s, torch.zeros(n_env, dtype=torch.float64, device="cuda"), torch.from_numpy(flags).cuda(), store=False)
        for e in range(n_env):
            if flags[e]:
                episode[e] += 1; t[e] = 0
                continue
            n, _, A, MU, _, _, _ = roll.read(e)
            assert n == t[e] + 1
            seen.append((call, e, episode[e], t[e], A[t[e]].copy(), MU[t[e]].copy()))
            t[e] += 1
    return seen


@pytest.mark.gpu
def test_library_noise_equals_its_restatement_and_depends_on_its_counter_alone(hip_api):
    """dNoise == NULL on a continuous head (dimA 3, given weights, unbounded components): (action - mean) / stdev equals the numpy
    restatement for (seed, env, episode, t, component) within 1e-12 -- the device's fp64 log, cos and sqrt against numpy's --, lies within
    +-3, and is the same value in a rollout of 3 and of 40 environments in which other environments end at other times"""
    seed = 0x5DEECE66D1234567
    L = _synth_learner(hip_api, DENSE16, None, n_eps=0)
    _given_weights(L)
    small, large = L.rollout(3, 12, seed=seed), L.rollout(40, 12, seed=seed)
    few = _drive(small, 3, 8, {2: [2], 5: [0]}, 6, seed=1)
    many = _drive(large, 40, 8, {1: [5, 17], 2: [2, 30], 4: [39], 5: [0, 1]}, 6, seed=2)      # (other states: the noise does not read them)
    worst = 0.0
    draws = {}
    for call, e, ep, t, a, mu in few + many:
        z = (a - mu[:3]) / mu[3:]
        want = R.noise_np(seed, e, ep, t, np.arange(3))
        worst = max(worst, float(np.abs(z - want).max()))
        assert np.all(np.abs(z) <= 3.0 + 1e-12)
        draws.setdefault((e, ep, t), []).append(z)
    print("largest difference between the device's noise and the restatement: %g" % worst)
    assert worst <= 1e-12, "largest difference between the device's noise and the restatement: %g" % worst
    shared = [k for k, v in draws.items() if len(v) == 2]
    assert len(shared) >= 15 and any(ep == 1 for _, ep, _ in shared)
    # the same (environment, episode, step) in both rollouts: the recovered values agree to the rounding of the recovery (other means)
    for k in shared:
        assert np.abs(draws[k][0] - draws[k][1]).max() <= 1e-14, k


@pytest.mark.gpu
def test_library_uniforms_of_a_discrete_head_give_the_label_they_imply(hip_api):
    """the discrete head's uniform cannot be read back from the label; the label must be the one the restated uniform implies on the stored
    probabilities (inverse CDF in option order, sums in fp64 as the head forms them)"""
    seed = 77
    L = _synth_learner(hip_api, DISCRETE, None, n_eps=0)
    _given_weights(L, seed=3)
    roll = L.rollout(40, 12, seed=seed)
    labels = set()
    for call, e, ep, t, a, mu in _drive(roll, 40, 8, {2: [2, 30], 5: [0, 1]}, 6, seed=4):
        u = float(R.noise_np(seed, e, ep, t, 0, discrete=True))
        cdf, label = 0.0, -1
        for j in range(4):
            cdf += mu[j]
            if label < 0 and cdf > u:
                label = j
        label = 3 if label < 0 else label
        assert a[0] == label + 0.1, (call, e, u, mu)
        labels.add(label)
    assert len(labels) >= 3


# ---- 4. the flags -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_evaluation_and_no_store_flags(hip_api):
    import torch
    A, B = [_synth_learner(hip_api, LSTM, SYNTH6, n_eps=10) for _ in range(2)]
    roll, hand = A.rollout(N_ENV, MAX_STEPS), R.HandLoop(B, N_ENV, MAX_STEPS)
    sim = R.ToySim(N_ENV, A.dS, A.dA, LENGTHS)
    before = A.counts()
    n_ended = 0
    for call in range(16):
        s, r, end, ended = sim.observe(MAX_STEPS)
        a = roll.step(s, r, end, evaluate=True, store=False)      # bit 0: select_actions_sequences_dev(noise=None); bit 1: nothing is ingested
        b = hand.step(s, r, end, noise=None, store=False)
        assert torch.equal(a, b), call
        n_ended += sum(ended)
        sim.advance(a, ended)
    assert n_ended >= 8
    _same_slabs(roll, hand, N_ENV)      # the slabs were reused: later episodes lie over the earlier ones
    info = roll.info()
    assert (info["calls"], info["episodes"], info["steps"]) == (16, 0, 0) and info["capped"] == hand.capped >= 2
    assert A.counts() == before
    _same_replay(A, B)
    # evaluate with a given noise array: the flag wins
    s, r, end, ended = sim.observe(MAX_STEPS)
    noise = _noise(np.random.default_rng(1), 1, N_ENV, A)[0]
    assert torch.equal(roll.step(s, r, end, noise, evaluate=True, store=False), hand.step(s, r, end, noise=None, store=False))


# ---- 5. training is untouched -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_rollout_between_steps_leaves_training_untouched(hip_api):
    """One learner drives a rollout (library noise, nothing stored) between its steps -- where the next minibatch is already drawn --, its
    twin never acts: weights, both moments, generator state and beta stay equal, eager steps and the replayed-graph form"""
    import torch
    synth = dict(seed=43, dimS=6, dimA=2, lenMin=5, lenMax=40, pTerm=0.5)
    A, B = [_synth_learner(hip_api, _rec_cfg(capi.NN_LSTM, (32, 32)), synth) for _ in range(2)]
    n_env = 70
    roll = A.rollout(n_env, 6, seed=4)
    rng = np.random.default_rng(2)
    s = torch.from_numpy(rng.normal(size=(n_env, 6)).astype(np.float32)).cuda()
    r = torch.ones(n_env, dtype=torch.float64, device="cuda")
    end = torch.from_numpy((np.arange(n_env) % 4 == 1).astype(np.int32)).cuda()

    def act():
        for _ in range(3):
            assert bool(torch.isfinite(roll.step(s, r, end, store=False)).all())

    for _ in range(3):
        A.step(1); B.step(1)
        act()
    A.step(4); B.step(4)
    _same_training_state(A, B)
    A.prepare_steps(3); B.prepare_steps(3)
    for _ in range(2):
        A.step(3); B.step(3)
        act()
    A.step(3); B.step(3)
    _same_training_state(A, B)
    _same_replay(A, B)
    assert roll.info()["calls"] == 15 and roll.info()["episodes"] == 0


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_of_the_rollout_calls(hip_api):
    import torch
    wide = _synth_learner(hip_api, FALLBACK["lstm-512"][0], None, n_eps=0)
    with pytest.raises(capi.HlError) as e:
        wide.rollout(4, 5)
    assert e.value.status == 8 and "hl_forward_sequences" in str(e.value)      # HL_ERR_UNSUPPORTED, the window call's message
    G = _synth_learner(hip_api, LSTM, SYNTH6, n_eps=10)
    roll = G.rollout(4, 5)
    s = torch.zeros((4, 6), dtype=torch.float32, device="cuda")
    r = torch.zeros(4, dtype=torch.float64, device="cuda")
    end = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert bool(torch.isfinite(roll.step(s, r, end)).all())
    G.policy_snapshot(); G.act_source("snapshot")
    with pytest.raises(capi.HlError) as e:
        roll.step(s, r, end)
    assert e.value.status == 8 and "HL_ACT_LIVE" in str(e.value)
    G.act_source("live")
    G.step_begin()
    with pytest.raises(capi.HlError) as e:
        roll.step(s, r, end)
    assert e.value.status == 4                                                 # HL_ERR_STATE
    G.step_end()
    assert bool(torch.isfinite(roll.step(s, r, end)).all())
    assert roll.info()["calls"] == 2                                           # the refused calls did not run
    with pytest.raises(ValueError):
        roll.step(s.cpu(), r, end)                                             # not on the GPU
    with pytest.raises(TypeError):
        roll.step(s.double(), r, end)                                          # dtype
    with pytest.raises(TypeError):
        roll.step(s, r.float(), end)
    with pytest.raises(TypeError):
        roll.step(s, r, end.long())
    with pytest.raises(TypeError):
        roll.step(s, r, end, noise=torch.zeros((4, 2), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        roll.step(torch.zeros((4, 12), dtype=torch.float32, device="cuda")[:, :6], r, end)      # not contiguous
    with pytest.raises(ValueError):
        roll.step(s[:3], r, end)                                               # too small
    with pytest.raises(capi.HlError) as e:
        G.rollout(0, 5)
    assert e.value.status == 1                                                 # HL_ERR_BAD_ARG
    with pytest.raises(capi.HlError):
        G.rollout(4, 1)
    # hl_destroy with a rollout still open destroys it; the library is as usable as before
    G.close()
    with pytest.raises(ValueError):
        roll.step(s, r, end)
    H = _synth_learner(hip_api, LSTM, SYNTH6, n_eps=10)
    again = H.rollout(4, 5)
    assert bool(torch.isfinite(again.step(s, r, end)).all())
    again.close()
    H.step(1)
