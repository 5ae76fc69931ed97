"""Acting from device memory for conv stacks of general geometry (smarties_amd/csrc/actconvg.hip: act_convg_dev_kernel, one launch per conv
layer on maps in device scratch; learner_act.h / learner_dev.h: the route ACT_DEV_SEQ_CONVG), on the GPU: the six small nets of
tests/test_convg_cpu.py and the five general-geometry nets of tests/blocks.py against the fp64 build of the CPU restatement, the bits across layouts, permutations, n and chunks of agents, the
head and the snapshot source, training left untouched, the rollout buffer, the refusals that remain.
(On the commit before the feature every device window call on these nets returns HL_ERR_UNSUPPORTED.)"""
import numpy as np
import pytest

import rollout as R
from acting import (N_AGENTS, TOL32, _bare, _call_dev, _check_heads, _columns, _count, _packed, _pair, _rows, _same_replay,
                    _same_training_state, _side_stream, _stacked, _synth_learner, _window_args)
from oracle_api import synth_cfg
from parity import assert_columns, relinf, twin64
from smarties_amd import capi
import blocks
from test_convg_cpu import NETS as CPU_NETS

pytestmark = pytest.mark.gpu
NAMES = ["same-3x3", "stride3", "aniso", "general-then-classic", "wide-channels", "frames-extras"]
# the geometries tests/blocks.py states for the training kernels' per-block comparison, here under the acting kernel's own band plan (it
# prefers 72 KB) and staging (quads inside an image row, single loads at its ends, a slot table): rows of 132, a stride of 8, a padding of K - 1
NAMES_BLOCKS = list(blocks.CONVG_NEW)
NETS = dict(CPU_NETS, **{n: (blocks.SHAPES[n]["kw"], blocks.SHAPES[n]["sc"], blocks.SHAPES[n]["n_eps"]) for n in NAMES_BLOCKS})
CPU_BAR = ()      # nets whose fp32 restatement loses more than TOL32 / 3 row-wise on these rows: none (the docstring of the first test)
QUIET = ("act_conv_dev", "act_conv_band_dev", "conv_fwd0", "conv_fwd1", "convg_fwd0", "convg_fwd1")


def _windows(kw, n=N_AGENTS):
    """n windows of lengths 1, 2 and nAppendedObs + 3 in turn, and the stacked rows hl_forward reads"""
    nApp = kw.get("nAppendedObs", 0)
    rng = np.random.default_rng(11)
    wins = [_rows(rng, (1, 2, nApp + 3)[i % 3], kw["dimS"]) for i in range(n)]
    return wins, _stacked(wins, nApp)


def _learner(hip_api, name, monkeypatch, chunk=None):
    kw, sc_kw, n_eps = NETS[name]
    monkeypatch.delenv("SMARTIES_HIP_GENERIC", raising=False)
    monkeypatch.delenv("SMARTIES_HIP_ACT_CONVG_CHUNK", raising=False)
    if chunk:
        monkeypatch.setenv("SMARTIES_HIP_ACT_CONVG_CHUNK", str(chunk))
    return _synth_learner(hip_api, kw, sc_kw, n_eps)


@pytest.mark.parametrize("name", NAMES + NAMES_BLOCKS)
def test_general_conv_stacks_act_from_device_windows(hip_api, name, monkeypatch):
    """The fp32 restatement against its fp64 build on these 37 rows after three steps (CPU), worst row-wise relinf: 2.1e-7 same-3x3, 1.7e-7 stride3,
    1.4e-7 aniso, 4.1e-7 general-then-classic, 6.1e-7 wide-channels, 3.7e-7 frames-extras; of NAMES_BLOCKS 2.9e-7 convg-wide-rows-132x2-b16,
    1.4e-7 convg-no-tap-classes-b8, 2.6e-7 convg-stride8x5-k9x8-b8, 2.8e-7 convg-stride7x5-k8x6-b8, 2.6e-7 convg-65-256-1x1-b41 -- every net
    within TOL32 / 3 = 3.3e-6, so every net is held to TOL32 row by row."""
    import torch
    kw, sc_kw, n_eps = NETS[name]
    monkeypatch.delenv("SMARTIES_HIP_GENERIC", raising=False)
    monkeypatch.delenv("SMARTIES_HIP_ACT_CONVG_CHUNK", raising=False)
    G, O = _pair(hip_api, kw, synth_cfg(**sc_kw), n_eps)
    G.step(3); O.step(3)
    wins, rows = _windows(kw)
    ref32, ref64 = O.forward(rows), twin64(O).forward(rows)
    side, n, nL = _side_stream(), N_AGENTS, len(kw["conv"])
    G.timing_enable(True)

    def counted(L, call, launches):
        c0 = [_count(L, k) for k in ("act_convg_dev",) + QUIET]
        got = call()
        torch.cuda.synchronize()
        d = [_count(L, k) - c for k, c in zip(("act_convg_dev",) + QUIET, c0)]
        assert d == [launches] + [0] * len(QUIET), (name, d)
        return got

    both = [counted(G, lambda: _call_dev(G, side, layout, np.arange(n)), nL) for layout in (_packed(wins), _columns(wins))]
    full = both[0]
    err = [relinf(full[i], ref64[i]) for i in range(n)]
    print("%s: worst row %d relinf %.3g (fp32 restatement %.3g)" % (name, int(np.argmax(err)), max(err), max(relinf(ref32[i], ref64[i]) for i in range(n))))
    assert full.shape == (n, G.nOut)
    if name in CPU_BAR:
        assert_columns(full, ref64, TOL32, name, ref32, cpu_bar=True)
    else:
        assert max(err) < TOL32, (name, int(np.argmax(err)))
    assert np.array_equal(both[0], both[1]), name                            # packed and as columns of a [T][nEnv] buffer
    perm = np.random.default_rng(3).permutation(n)
    assert np.array_equal(_call_dev(G, side, _columns(wins), perm), full[perm]), name
    one = counted(G, lambda: _call_dev(G, side, _packed(wins[:1]), np.arange(1)), nL)
    assert np.array_equal(one[0], full[0]), name
    G.timing_enable(False)
    # n = 5 in chunks of 2 on a twin with the same weights: three chunks' launches, the bits of one chunk
    T = _learner(hip_api, name, monkeypatch, chunk=2)
    T.step(3)
    assert np.array_equal(T.get_params()[0], G.get_params()[0])
    T.timing_enable(True)
    five = counted(T, lambda: _call_dev(T, side, _packed(wins[:5]), np.arange(5)), 3 * nL)
    T.timing_enable(False)
    assert np.array_equal(five, _call_dev(G, side, _packed(wins[:5]), np.arange(5))) and np.array_equal(five, full[:5]), name


@pytest.mark.parametrize("name", ["same-3x3", "frames-extras"])
def test_head_and_snapshot_source_read_the_sources_blob(hip_api, name, monkeypatch):
    import torch
    kw = NETS[name][0]
    G = _learner(hip_api, name, monkeypatch)
    G.step(2)
    wins, _ = _windows(kw)
    side, layout, order = _side_stream(), _columns(wins), np.arange(N_AGENTS)
    rng = np.random.default_rng(5)
    nOpt = kw.get("n_options", 0)
    noise = rng.uniform(0, 1, N_AGENTS) if nOpt else np.clip(rng.normal(size=(N_AGENTS, kw["dimA"])), -2, 2)
    first = _call_dev(G, side, layout, order)
    got = _call_dev(G, side, layout, order, select=torch.from_numpy(noise).cuda())
    _check_heads(dict(kw, bounded=()), first, noise, [torch.from_numpy(x) for x in got])
    torch.cuda.synchronize()
    G.policy_snapshot(); G.act_source("snapshot")
    G.step(5)
    assert np.array_equal(_call_dev(G, side, layout, order), first), name     # the snapshot, not the live weights or a prepared copy
    G.act_source("live")
    now = _call_dev(G, side, layout, order)
    assert not np.array_equal(now, first)
    torch.cuda.synchronize()
    G.policy_snapshot(); G.act_source("snapshot")
    assert np.array_equal(_call_dev(G, side, layout, order), now), name
    G.act_source("live")


def test_acting_through_the_new_route_leaves_training_untouched(hip_api, monkeypatch):
    import torch
    kw = NETS["general-then-classic"][0]
    A, B = [_learner(hip_api, "general-then-classic", monkeypatch) for _ in range(2)]
    wins, _ = _windows(kw)
    side, layout = _side_stream(), _columns(wins)
    noise = torch.from_numpy(np.clip(np.random.default_rng(2).normal(size=(N_AGENTS, kw["dimA"])), -2, 2)).cuda()
    for _ in range(4):
        assert np.isfinite(_call_dev(A, side, layout, np.arange(N_AGENTS))).all()
        assert all(np.isfinite(x).all() for x in _call_dev(A, side, layout, np.arange(N_AGENTS), select=noise))
        A.step(1); B.step(1)
    _same_training_state(A, B)
    _same_replay(A, B)


def test_rollout_buffer_serves_a_general_stack_live_and_staged(hip_api, monkeypatch):
    import torch
    n_env, max_steps, calls = 3, 8, 4
    A, B, S = [_learner(hip_api, "frames-extras", monkeypatch) for _ in range(3)]
    roll, hand = A.rollout(n_env, max_steps, seed=1, tag_base=5000), R.HandLoop(B, n_env, max_steps, tag_base=5000)
    S.policy_snapshot(); S.act_source("snapshot")
    staged = S.rollout(n_env, max_steps, seed=1, tag_base=5000, staging_rows=4 * max_steps)
    sim = R.ToySim(n_env, A.dS, A.dA, [[(0, 0)]] * n_env)
    noise = torch.from_numpy(np.random.default_rng(9).uniform(size=(calls, n_env))).cuda()
    for call in range(calls):
        s, r, end, ended = sim.observe(max_steps)
        a = roll.step(s, r, end, noise[call])
        assert torch.equal(a, hand.step(s, r, end, noise[call])), call      # (HandLoop acts through select_actions_sequences_dev)
        assert torch.equal(a, staged.step(s, r, end, noise[call])), call
        assert not any(ended) and bool((a != 0).all())
        sim.advance(a, ended)
    torch.cuda.synchronize()
    assert roll.info()["calls"] == calls == staged.info()["calls"]


def test_what_stays_refused(hip_api, monkeypatch):
    import torch
    G = _learner(hip_api, "same-3x3", monkeypatch)
    with pytest.raises(capi.HlError) as e:
        G.forward_dev(torch.zeros((3, G.dIn), dtype=torch.float32, device="cuda"))
    assert e.value.status == 8 and "hl_forward_sequences_dev" in str(e.value), str(e.value)
    with pytest.raises(capi.HlError) as e:      # (a dense layer of 2064 behind a padded layer: hl_create is what names the bound)
        wide = _bare(hip_api, dict(NETS["same-3x3"][0], hidden=(2064,)))
        wide.forward_sequences_dev(*_window_args(wide), 1)
    assert e.value.status == 8 and "2048" in str(e.value), str(e.value)
