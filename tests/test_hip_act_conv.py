"""hl_forward's route for feed-forward nets behind convolutions (smarties_amd/csrc/actconv.hip: act_conv_kernel, the conv stack of one
row per workgroup with every map in LDS; the dense layers behind through act_rows_kernel on the feature rows): two launches per chunk,
the training buffers, the prepared filter layouts and a minibatch drawn ahead left alone.

GPU suite: every row against the CPU oracle's ol_forward (bound TOL32, relative-infinity), for the shapes where the kernel's tails,
strides, extras and row walks can go wrong; the byte cap of a chunk; row independence bit for bit, also through the window calls; the
launches; the training path left untouched; weights given without a step; the fallbacks (SMARTIES_HIP_GENERIC=2, an image beyond the
LDS, rows beyond HL_ACT_CONV_MAX_ROW_BYTES -- the RACER_atari.json stack runs the route with SMARTIES_HIP_GENERIC=4096, which holds
that switch open); refusals.
CPU suite (the last test): the staging constant and the kernel's resource remarks."""
import os
import re
import sys

import numpy as np
import pytest

from acting import ILL_COLUMNS, LDS_NETS, NETS, TOL32, _compare_step, _conv_pair as _pair, _count, _row_bytes, _rows, _training_forwards
from parity import COL_ROWS, assert_columns, relinf, twin64
from smarties_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cap(dIn):
    return max(16, min(capi.ACT_ROWS_CHUNK, capi.ACT_CONV_STAGE_BYTES // (4 * dIn)) // 16 * 16)


def _check_rows(name, n, out, ref):
    assert out.shape == (n, ref.shape[1])
    err = [relinf(out[i], ref[i]) for i in range(n)]
    worst = int(np.argmax(err))
    print("%s n=%d: worst row %d relinf %.3g" % (name, n, worst, err[worst]))
    assert err[worst] < TOL32, (name, n, worst, out[worst], ref[worst])


# ---- 1. parity with the oracle, row by row -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NETS))
def test_conv_rows_match_oracle_row_by_row(hip_api, name, monkeypatch):
    if _row_bytes(NETS[name]) > capi.ACT_CONV_MAX_ROW_BYTES:      # (app3-extra, atari) the switch held open: the kernel is held to the oracle there too
        monkeypatch.setenv("SMARTIES_HIP_GENERIC", "4096")
    G, O = _pair(hip_api, name)
    G.step(3); O.step(3)
    ns = (1, 17) if name == "atari" else (1, 17, 81, capi.ACT_ROWS_CHUNK + 1)      # one row, ragged row blocks, walked rows, two chunks
    st = _rows(np.random.default_rng(11), max(ns), G.dIn)
    ref = O.forward(st)
    ref64 = twin64(O).forward(st)
    G.timing_enable(True)
    for n in ns:
        n0 = _count(G, "act_conv")
        out = G.forward(st[:n])
        assert _count(G, "act_conv") - n0 == -(-n // _cap(G.dIn)), (name, n)      # (the route under test served the call)
        _check_rows(name, n, out, ref)
        if n >= COL_ROWS:
            assert_columns(out, ref64[:n], TOL32, (name, n), ref[:n], cpu_bar=name in ILL_COLUMNS)
    G.timing_enable(False)


# ---- 2. the byte cap of a chunk ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_chunks_hold_no_more_rows_than_the_staging_bytes(hip_api, monkeypatch):
    monkeypatch.setenv("SMARTIES_HIP_GENERIC", "4096")      # (rows beyond HL_ACT_CONV_MAX_ROW_BYTES: the switch held open)
    G, O = _pair(hip_api, "atari")
    G.step(2); O.step(2)
    cap = _cap(G.dIn)
    assert cap == 288
    st = _rows(np.random.default_rng(3), cap + 1, G.dIn)
    G.timing_enable(True)
    c0, r0 = _count(G, "act_conv"), _count(G, "act_rows")
    out = G.forward(st)
    assert _count(G, "act_conv") - c0 == 2 and _count(G, "act_rows") - r0 == 2
    G.timing_enable(False)
    for i in (0, cap - 1, cap):
        assert relinf(out[i], O.forward(st[i:i + 1])[0]) < TOL32, i
    rows = np.r_[0:16, cap - 15:cap + 1]      # (the oracle's forward through this stack takes its time: both ends of the first chunk, the second's row)
    assert_columns(out[rows], twin64(O).forward(st[rows]), TOL32, "two chunks", O.forward(st[rows]), cpu_bar=True)


# ---- 3. row independence, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["strided", "extras6"])
def test_a_rows_output_does_not_depend_on_its_place_or_on_n(hip_api, name):
    G = _pair(hip_api, name, oracle=False)
    G.step(3)
    rng = np.random.default_rng(13)
    st = _rows(rng, 300, G.dIn)
    out300 = G.forward(st)
    assert np.array_equal(G.forward(st[:1]), out300[:1])
    perm = rng.permutation(300)
    assert np.array_equal(G.forward(st[perm]), out300[perm])


@pytest.mark.gpu
def test_windows_of_a_conv_net_inherit_the_route(hip_api):
    G = _pair(hip_api, "app3", oracle=False)
    G.step(3)
    rng = np.random.default_rng(3)
    lengths = [1, 2, 5, 8, 3]
    wins = [_rows(rng, lengths[i % 5], 200) for i in range(23)]
    rows = np.stack([np.concatenate([w[max(len(w) - 1 - j, 0)] for j in range(4)]) for w in wins])
    G.timing_enable(True)
    n0 = _count(G, "act_conv")
    out = G.forward_sequences(wins)
    assert _count(G, "act_conv") - n0 == 1
    G.timing_enable(False)
    assert np.array_equal(out, G.forward(rows))
    for i, w in enumerate(wins):
        assert np.array_equal(out[i], G.forward_sequence(w)), i


# ---- 4. launches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_launches_per_chunk_and_no_training_forward(hip_api):
    G = _pair(hip_api, "strided", oracle=False)
    G.step(2)
    st = _rows(np.random.default_rng(6), 2 * capi.ACT_ROWS_CHUNK + 40, G.dIn)
    assert _cap(G.dIn) == capi.ACT_ROWS_CHUNK
    G.forward(st[:3])
    G.timing_enable(True)
    G.step(1)                                                   # (the training forward launches run under these names)
    fwd = _training_forwards(G)
    assert fwd[0] > 0 and fwd[1] > 0
    for n, want in ((1, 1), (65, 1), (len(st), 3)):
        c0, r0 = _count(G, "act_conv"), _count(G, "act_rows")
        G.forward(st[:n])
        assert _count(G, "act_conv") - c0 == want and _count(G, "act_rows") - r0 == want, n
    assert _training_forwards(G) == fwd
    G.timing_enable(False)


# ---- 5. training is untouched ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["strided", "extras6"])
def test_conv_acting_leaves_training_untouched(hip_api, name):
    """After a step the next minibatch is already drawn: acting in between must neither consume nor disturb it (same sample indices
    as the oracle in the following step), eager steps and the replayed-graph form."""
    G, O = _pair(hip_api, name)
    st = _rows(np.random.default_rng(2), 40, G.dIn)
    for _ in range(3):
        G.step(1); O.step(1)
        _compare_step(G, O)
        out = G.forward(st)
        assert relinf(out[-1], O.forward(st[-1:])[0]) < TOL32
    G.step(4); O.step(4)
    _compare_step(G, O)
    G.prepare_steps(3)
    for _ in range(2):
        G.step(3); O.step(3)
        _compare_step(G, O)
        out = G.forward(st)
        assert relinf(out[0], O.forward(st[:1])[0]) < TOL32
    G.step(3); O.step(3)
    _compare_step(G, O)
    assert np.array_equal(G.get_rng_state(), O.get_rng_state())
    assert relinf(G.get_params()[0], O.get_params()[0]) < 2 * TOL32


@pytest.mark.gpu
def test_conv_acting_keeps_the_minibatch_drawn_ahead(hip_api):
    """The stand-alone sampling launch (launchSample, step_exec.h: timed under the name step_tail_kernel) runs as often with an acting call between two steps as without: the
    route over the training buffers drops the minibatch drawn ahead and draws it again, one launch more."""
    G = _pair(hip_api, "strided", oracle=False)
    T = _pair(hip_api, "strided", oracle=False)
    st = _rows(np.random.default_rng(2), 40, G.dIn)
    for L in (G, T):
        L.step(2)
        L.timing_enable(True)
    g0, t0 = _count(G, "step_tail_kernel"), _count(T, "step_tail_kernel")
    G.step(1); G.forward(st); G.step(1)
    T.step(1); T.step(1)
    assert _count(G, "step_tail_kernel") - g0 == _count(T, "step_tail_kernel") - t0
    for L in (G, T):
        L.timing_enable(False)
    assert np.array_equal(G.get_rng_state(), T.get_rng_state())
    assert np.array_equal(G.get_params()[0], T.get_params()[0])


# ---- 6. weights given without a step: the reference filter layout, not the training kernels' prepared copies -------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["strided", "odd"])
def test_given_weights_serve_acting_without_a_step(hip_api, name):
    G, O = _pair(hip_api, name, weights=lambda L: np.random.default_rng(1).uniform(-0.1, 0.1, L.get_params()[0].shape).astype(np.float32))
    st = _rows(np.random.default_rng(9), 20, G.dIn)
    _check_rows(name, 20, G.forward(st), O.forward(st))
    G.step(2); O.step(2)
    w = np.random.default_rng(2).uniform(-0.1, 0.1, G.get_params()[0].shape).astype(np.float32)
    for L in (G, O):
        L.set_params(w, np.zeros_like(w), np.zeros_like(w))
    _check_rows(name, 20, G.forward(st), O.forward(st))


# ---- 7. fallbacks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_generic_bit_2_keeps_the_training_buffer_route(hip_api, monkeypatch):
    st = _rows(np.random.default_rng(8), 40, 576)
    outs = {}
    for env in (None, "2"):
        monkeypatch.delenv("SMARTIES_HIP_GENERIC", raising=False)
        if env:
            monkeypatch.setenv("SMARTIES_HIP_GENERIC", env)
        G = _pair(hip_api, "strided", oracle=False)
        G.step(3)
        G.timing_enable(True)
        n0 = _count(G, "act_conv")
        outs[env] = G.forward(st)
        assert _count(G, "act_conv") - n0 == (0 if env else 1)
        G.timing_enable(False)
    for i in range(40):
        assert relinf(outs["2"][i], outs[None][i]) < 2 * TOL32, i


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LDS_NETS))
def test_an_image_or_a_map_beyond_the_lds_keeps_the_training_buffer_route(hip_api, name, monkeypatch):
    """act_conv_plan's 160 KB budget is what refuses these nets: the row-size switch is open for both (held open / not reached)."""
    kw = LDS_NETS[name]
    monkeypatch.setenv("SMARTIES_HIP_GENERIC", "4096")
    if name == "map-162K":
        assert _row_bytes(kw) <= capi.ACT_CONV_MAX_ROW_BYTES
    G, O = _pair(hip_api, kw)
    G.step(2); O.step(2)
    st = _rows(np.random.default_rng(4), 3, G.dIn)
    G.timing_enable(True)
    out = G.forward(st)
    assert _count(G, "act_conv") == 0
    G.timing_enable(False)
    _check_rows(name, 3, out, O.forward(st))


@pytest.mark.gpu
def test_a_map_beyond_the_lds_is_refused_as_shipped(hip_api, monkeypatch):
    """the same small-row net without any switch: the plan's refusal is all that stands between it and a launch asking for more LDS than a workgroup has"""
    monkeypatch.delenv("SMARTIES_HIP_GENERIC", raising=False)
    G = _pair(hip_api, LDS_NETS["map-162K"], oracle=False)
    G.step(1)
    st = _rows(np.random.default_rng(4), 20, G.dIn)
    G.timing_enable(True)
    out = G.forward(st)
    assert _count(G, "act_conv") == 0 and np.isfinite(out).all()
    G.timing_enable(False)


@pytest.mark.gpu
def test_rows_beyond_the_measured_size_keep_the_training_buffer_route(hip_api, monkeypatch):
    """HL_ACT_CONV_MAX_ROW_BYTES: the RACER_atari.json rows (110 KB) stay on the training forward launches, where they are faster."""
    monkeypatch.delenv("SMARTIES_HIP_GENERIC", raising=False)
    G, O = _pair(hip_api, "atari")
    assert 4 * G.dIn > capi.ACT_CONV_MAX_ROW_BYTES
    G.step(2); O.step(2)
    st = _rows(np.random.default_rng(4), 3, G.dIn)
    G.timing_enable(True)
    out = G.forward(st)
    assert _count(G, "act_conv") == 0
    G.timing_enable(False)
    _check_rows("atari-default", 3, out, O.forward(st))


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_conv_acting_refusals(hip_api):
    G = _pair(hip_api, "odd", oracle=False)
    G.step(2)
    st = _rows(np.random.default_rng(4), 40, G.dIn)
    assert G.forward(st[:0]).shape == (0, G.nOut)                             # n = 0: HL_OK
    good = G.forward(st)
    assert np.isfinite(good).all()
    G.step_begin()
    with pytest.raises(capi.HlError) as e:
        G.forward(st)
    assert e.value.status == 4                                                # HL_ERR_STATE
    G.step_end()
    again = G.forward(st)                                                     # (the step in between moved the weights)
    assert again.shape == good.shape and np.isfinite(again).all()


# ---- 9. surface and resources (no GPU) ---------------------------------------------------------------------------------------------
def test_conv_stack_kernel_builds_without_scratch():
    import __graft_entry__ as ge
    ge.build_hip()
    header = open(os.path.join(ROOT, "include", "smarties_hip_act.h")).read()
    m = re.search(r"#define\s+HL_ACT_CONV_STAGE_BYTES\s+\((\d+)u\s*<<\s*(\d+)\)", header)
    assert m and int(m.group(1)) << int(m.group(2)) == capi.ACT_CONV_STAGE_BYTES == 32 << 20
    m = re.search(r"#define\s+HL_ACT_CONV_MAX_ROW_BYTES\s+\((\d+)u\s*<<\s*(\d+)\)", header)
    assert m and int(m.group(1)) << int(m.group(2)) == capi.ACT_CONV_MAX_ROW_BYTES
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = resource_usage.kernels().get("actconv.hip")
    assert rows, "no resource remarks of actconv.hip beside the objects"
    assert any(k["name"].startswith("act_conv_kernel") for k in rows)
    for k in rows:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
