"""hl_forward's many-row route for dense nets (smarties_amd/csrc/actrows.hip: act_rows_kernel): the whole net for a block of 16 rows per
workgroup on the MFMA, one launch per chunk of HL_ACT_ROWS_CHUNK rows, the training buffers and a minibatch drawn ahead left alone.

GPU suite: every row against the CPU oracle's ol_forward, for the shapes where the kernel's tails, residuals and row blocks can go
wrong; the wide single-row calls; row independence; one launch per chunk; the training path left untouched; the route over the training
buffers (SMARTIES_HIP_GENERIC=2) for comparison; refusals.
CPU suite (the last test): the chunk constant and the kernel's resource remarks."""
import os
import re
import sys

import numpy as np
import pytest

from acting import ROWS_WIDE as WIDE, TOL32, _compare_step, _pair, _rows
from oracle_api import fill_synth, synth_cfg
from parity import COL_ROWS, assert_columns, relinf, twin64
from smarties_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sc(kw, **over):
    d = dict(seed=21, dimS=kw["dimS"], dimA=kw["dimA"], lenMin=5, lenMax=40, pTerm=0.5)
    d.update(over)
    return synth_cfg(**d)


def _launches(G):
    return G.timing_get("act_rows")[1]


NETS = {
    # K not a multiple of 4, narrowing residuals, widths below 16
    "24x16x8": dict(dimS=9, dimA=3, bounded=[0, 0, 0], hidden=(24, 16, 8), nnFunc="Tanh", batchSize=8, maxTotObsNum=2000, randSeed=5),
    # a width that is no multiple of 16, a widening residual with resW < size
    "20x40": dict(dimS=17, dimA=2, bounded=[1, 0], hidden=(20, 40), nnFunc="Tanh", batchSize=8, maxTotObsNum=2000, randSeed=7),
    # stMean[c % dS] on stacked rows
    "app3-2x32": dict(dimS=9, dimA=3, bounded=[0, 0, 0], hidden=(32, 32), nnFunc="Tanh", batchSize=8, maxTotObsNum=2000, randSeed=5, nAppendedObs=3),
    # the headline shape
    "2x256-softsign": dict(dimS=17, dimA=6, hidden=(256, 256), nnFunc="SoftSign", batchSize=32, maxTotObsNum=4000, randSeed=3),
    "discrete5": dict(dimS=9, dimA=1, bounded=[0], hidden=(48, 32), nnFunc="Tanh", batchSize=8, maxTotObsNum=2000, randSeed=9,
                      adv_kind=capi.ADV_DISCRETE, n_options=5),
    "tanh-out-gauss": dict(dimS=9, dimA=3, bounded=[1, 0, 0], hidden=(48, 32), nnFunc="Tanh", batchSize=8, maxTotObsNum=2000, randSeed=11,
                           adv_kind=capi.ADV_GAUSSIAN, nnOutputFunc="Tanh"),
}


# ---- 1. parity with the oracle, row by row -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NETS))
def test_many_rows_match_oracle_row_by_row(hip_api, name):
    kw = NETS[name]
    G, O = _pair(hip_api, kw, _sc(kw), 40, given=name == "tanh-out-gauss")
    G.step(3); O.step(3)
    st = _rows(np.random.default_rng(11), capi.ACT_ROWS_CHUNK + 1, G.dIn)
    ref = O.forward(st)
    ref64 = twin64(O).forward(st)
    for n in (65, 81, 300, capi.ACT_ROWS_CHUNK + 1):      # a block with one live row, ragged blocks, two chunks
        out = G.forward(st[:n])
        assert out.shape == (n, G.nOut)
        err = [relinf(out[i], ref[i]) for i in range(n)]
        worst = int(np.argmax(err))
        print("%s n=%d: worst row %d relinf %.3g" % (name, n, worst, err[worst]))
        assert err[worst] < TOL32, (name, n, worst, out[worst], ref[worst])
        assert_columns(out, ref64[:n], TOL32, (name, n), ref[:n])


# ---- 2. the wide single-row call ---------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WIDE))
def test_wide_nets_take_the_route_for_any_row_count(hip_api, name):
    kw = WIDE[name]
    G, O = _pair(hip_api, kw, _sc(kw, lenMin=5, lenMax=20), 20)
    G.step(3); O.step(3)
    st = _rows(np.random.default_rng(5), 70, G.dIn)
    ref = O.forward(st)
    ref64 = twin64(O).forward(st)
    G.timing_enable(True)
    for n in (1, 3, 70):
        n0 = _launches(G)
        out = G.forward(st[:n])
        assert _launches(G) - n0 == 1, (name, n)
        err = [relinf(out[i], ref[i]) for i in range(n)]
        print("%s n=%d: worst relinf %.3g" % (name, n, max(err)))
        assert max(err) < TOL32, (name, n, int(np.argmax(err)))
        if n >= COL_ROWS:
            assert_columns(out, ref64[:n], TOL32, (name, n), ref[:n])
    G.timing_enable(False)


# ---- 3. row independence -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["24x16x8", "2x256-softsign"])
def test_a_rows_output_does_not_depend_on_its_block_or_on_n(hip_api, name):
    kw = NETS[name]
    G, O = _pair(hip_api, kw, _sc(kw), 40)
    G.step(3)
    rng = np.random.default_rng(13)
    st = _rows(rng, 300, G.dIn)
    out300 = G.forward(st)
    assert np.array_equal(G.forward(st[:65]), out300[:65])
    perm = rng.permutation(300)
    assert np.array_equal(G.forward(st[perm]), out300[perm])


@pytest.mark.gpu
def test_dense_windows_inherit_the_route(hip_api):
    kw = dict(dimS=9, dimA=3, bounded=[0, 0, 0], hidden=(24, 16, 8), nnFunc="Tanh", batchSize=8, maxTotObsNum=1000, randSeed=5, nAppendedObs=3)
    G, O = _pair(hip_api, kw, synth_cfg(seed=3, dimS=9, dimA=3, lenMin=5, lenMax=30, pTerm=0.3), 40)      # (the dense-app3 net of test_hip_act_batch)
    G.step(3)
    rng = np.random.default_rng(3)
    lengths = [1, 2, 5, 8, 3]
    wins = [_rows(rng, lengths[i % 5], 9) for i in range(70)]
    rows = np.stack([np.concatenate([w[max(len(w) - 1 - j, 0)] for j in range(4)]) for w in wins])
    G.timing_enable(True)
    n0 = _launches(G)
    out = G.forward_sequences(wins)
    assert _launches(G) - n0 == 1
    G.timing_enable(False)
    assert np.array_equal(out, G.forward(rows))


# ---- 4. one launch per chunk -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_many_rows_are_one_launch_per_chunk(hip_api):
    kw = NETS["2x256-softsign"]
    G, O = _pair(hip_api, kw, _sc(kw), 40)
    G.step(2); O.step(2)
    st = _rows(np.random.default_rng(6), 2 * capi.ACT_ROWS_CHUNK + 40, G.dIn)
    G.forward(st[:3])
    G.timing_enable(True)
    n0 = _launches(G)
    out65 = G.forward(st[:65])
    n1 = _launches(G)
    assert n1 - n0 == 1
    out = G.forward(st)
    n2 = _launches(G)
    assert n2 - n1 == -(-len(st) // capi.ACT_ROWS_CHUNK) == 3
    out64 = G.forward(st[:64])                                  # the one-kernel route keeps these
    assert _launches(G) == n2
    G.timing_enable(False)
    assert np.array_equal(out[:65], out65)
    assert relinf(out64, out[:64]) < 2 * TOL32
    for i in (0, capi.ACT_ROWS_CHUNK - 1, capi.ACT_ROWS_CHUNK, 2 * capi.ACT_ROWS_CHUNK, len(st) - 1):      # both sides of the chunk borders
        assert relinf(out[i], O.forward(st[i:i + 1])[0]) < TOL32, i
    assert_columns(out, twin64(O).forward(st), TOL32, "three chunks")


# ---- 4b. the size switch: nets beyond HL_ACT_ROWS_SMALL_NET weights take the route only from HL_ACT_ROWS_WIDE_MIN_N rows and two rounds of Mmax on --
SWITCH = {     # name: (configuration, act_rows launches at n = 70, at n = 1025)
    # 9 x 384 + 384 x 384 + 384 x 8 = 153 984 weights, below the 196 608 of the switch; 384 columns: two column groups per wavefront
    "2x384-small": (dict(dimS=9, dimA=3, bounded=[1, 0, 0], hidden=(384, 384), nnFunc="SoftSign", batchSize=8, maxTotObsNum=2000, randSeed=19), 1, 2),
    # 9 x 512 + 512 x 512 + 512 x 8 = 270 848 weights, above it (the measured shape that placed it); two column groups per wavefront
    "2x512-large": (dict(dimS=9, dimA=3, bounded=[1, 0, 0], hidden=(512, 512), nnFunc="SoftSign", batchSize=8, maxTotObsNum=2000, randSeed=19), 0, 2),
    # 9 x 1024 + 1024 x 768 + 768 x 8 = 801 792 weights; 1024 columns: four column groups per wavefront
    "1024x768-large": (dict(dimS=9, dimA=3, bounded=[1, 0, 0], hidden=(1024, 768), nnFunc="Tanh", batchSize=8, maxTotObsNum=2000, randSeed=19), 0, 2),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SWITCH))
def test_size_switch_routes_and_both_routes_match_oracle(hip_api, name):
    kw, at70, at1025 = SWITCH[name]
    G, O = _pair(hip_api, kw, _sc(kw, lenMin=5, lenMax=20), 20)
    G.step(3); O.step(3)
    st = _rows(np.random.default_rng(7), capi.ACT_ROWS_CHUNK + 1, G.dIn)
    ref = O.forward(st)
    ref64 = twin64(O).forward(st)
    G.timing_enable(True)
    for n, want in ((70, at70), (capi.ACT_ROWS_CHUNK + 1, at1025)):
        n0 = _launches(G)
        out = G.forward(st[:n])
        assert _launches(G) - n0 == want, (name, n)
        err = [relinf(out[i], ref[i]) for i in range(n)]
        print("%s n=%d: worst relinf %.3g" % (name, n, max(err)))
        assert max(err) < TOL32, (name, n, int(np.argmax(err)))
        assert_columns(out, ref64[:n], TOL32, (name, n), ref[:n])
    G.timing_enable(False)


@pytest.mark.gpu
def test_a_large_net_waits_for_two_rounds_of_the_training_rows(hip_api):
    """batchSize 600: the launches over the training buffers serve 1025 rows in one round of Mmax = 1200, so the large net stays there."""
    kw = dict(SWITCH["1024x768-large"][0], batchSize=600, maxTotObsNum=4000)
    G = capi.Learner(hip_api, capi.make_config(**kw))
    G.init_weights(); fill_synth(G, _sc(kw, lenMin=20, lenMax=40), 40); G.initialize()
    st = _rows(np.random.default_rng(7), 2401, G.dIn)
    G.timing_enable(True)
    n0 = _launches(G)
    few = G.forward(st[:1025])
    assert _launches(G) == n0
    many = G.forward(st)                      # 2401 rows >= 2 x 1200: three chunks of the many-row route
    assert _launches(G) - n0 == 3
    G.timing_enable(False)
    for i in range(1025):
        assert relinf(many[i], few[i]) < 2 * TOL32, i


# ---- 5. training is untouched ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["24x16x8", "2x256-softsign"])
def test_many_row_acting_leaves_training_untouched(hip_api, name):
    """After a step the next minibatch is already drawn: acting in between must neither consume nor disturb it (same sample indices
    as the oracle in the following step), eager steps and the replayed-graph form."""
    kw = NETS[name]
    G, O = _pair(hip_api, kw, _sc(kw), 40)
    st = _rows(np.random.default_rng(2), 70, G.dIn)
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


# ---- 6. the route over the training buffers stays reachable ------------------------------------------------------------------------
@pytest.mark.gpu
def test_generic_bit_2_keeps_the_training_buffer_route(hip_api, monkeypatch):
    kw = NETS["2x256-softsign"]
    st = _rows(np.random.default_rng(8), 70, 17)
    outs = {}
    for env in (None, "2"):
        monkeypatch.delenv("SMARTIES_HIP_GENERIC", raising=False)
        if env:
            monkeypatch.setenv("SMARTIES_HIP_GENERIC", env)
        G = capi.Learner(hip_api, capi.make_config(**kw))
        G.init_weights(); fill_synth(G, _sc(kw), 40); G.initialize()
        G.step(3)
        G.timing_enable(True)
        n0 = _launches(G)
        outs[env] = G.forward(st)
        assert _launches(G) - n0 == (0 if env else 1)
        G.timing_enable(False)
    for i in range(70):
        assert relinf(outs["2"][i], outs[None][i]) < 2 * TOL32, i


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_many_row_acting_refusals(hip_api):
    kw = NETS["24x16x8"]
    G, O = _pair(hip_api, kw, _sc(kw), 40)
    G.step(2)
    st = _rows(np.random.default_rng(4), 70, G.dIn)
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


# ---- 8. surface and resources (no GPU) ---------------------------------------------------------------------------------------------
def test_row_block_kernel_builds_without_scratch():
    import __graft_entry__ as ge
    ge.build_hip()
    header = open(os.path.join(ROOT, "include", "smarties_hip_act.h")).read()
    m = re.search(r"#define\s+HL_ACT_ROWS_CHUNK\s+(\d+)", header)
    assert m and int(m.group(1)) == capi.ACT_ROWS_CHUNK == 1024
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = resource_usage.kernels().get("actrows.hip")
    assert rows, "no resource remarks of actrows.hip beside the objects"
    assert any(k["name"].startswith("act_rows_kernel") for k in rows)
    for k in rows:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
