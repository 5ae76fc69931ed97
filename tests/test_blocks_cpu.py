"""The yardstick of tests/test_hip_blocks.py, pinned on the CPU: the fp32 restatement (O32, oracle/liboracle_port.so) against its
build with the arrays in double (O64, oracle/liboracle_port64.so) on every shape of tests/blocks.py, four steps from the same
weights, each drawing its own minibatches; the claim "one shape per launch route" held to the names step_exec.h times and, for
the recurrent kernels those names do not tell apart, to the names rec.hip prints; and blocks.judge, what the GPU test asserts, fed
snapshots with one block doctored."""
import os
import re

import numpy as np
import pytest

import blocks
from blocks import N_STEPS, PARAM_Q, SHAPES, TAP_Q, TOL32, cpu_reference
from oracle_api import oracle_learner
from parity import blockdev, fixture_config, flat_for, load_fixture, param_blocks, relinf, setup_from_fixture


@pytest.mark.parametrize("name", list(SHAPES) + list(blocks.BOUND_SHAPES))
def test_both_builds_take_the_same_decisions(name):
    """(i) sampled indices, tags, time steps, far-policy flags, the far-policy count and the generator state are equal at every step;
    (ii) beta agrees to 1e-12"""
    for k, st in enumerate(cpu_reference(name)["steps"]):
        a, b = st["s32"], st["s64"]
        for key in list(blocks.INT_TAPS) + ["rng"]:
            assert np.array_equal(a[key], b[key]), (k, key)
        assert a["nFar"] == b["nFar"] and a["CmaxRet"] == b["CmaxRet"], k
        assert abs(a["beta"] - b["beta"]) <= 1e-12 * b["beta"], (k, a["beta"], b["beta"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_fp32_loses_at_most_a_third_of_tol32_in_every_block(name):
    """(iii) e_cpu(b) <= TOL32 / 3 for every block of gradSum, M1, M2, W and every column of the taps, at every step -- but for the
    blocks the shape lists as ill-conditioned (blocks.py says why they are), at most 1 in 20, each of which does exceed it"""
    ref = cpu_reference(name)
    listed = SHAPES[name].get("listed", {})
    nBlocks = sum(len(d) for d in ref["steps"][0]["e_cpu"].values())
    assert set(ref["steps"][0]["e_cpu"]) == set(PARAM_Q) | set(TAP_Q)
    assert 20 * len(listed) <= nBlocks, (len(listed), nBlocks)
    worst = {}
    for k, st in enumerate(ref["steps"]):
        for q, devs in st["e_cpu"].items():
            w, b = blocks.worst({b: v for b, v in devs.items() if (q, b) not in listed})
            print("step %d %-8s worst e_cpu %.2e in %s" % (k + 1, q, w, b))
            for b, v in devs.items():
                assert (q, b) in listed or v == "zero" or v <= TOL32 / 3, (k, q, b, v)
                if (q, b) in listed:
                    worst[(q, b)] = max(worst.get((q, b), 0.0), v)
    assert set(worst) == set(listed), set(listed) - set(worst)      # (every listed block exists)
    for key, v in worst.items():
        print("listed %s: worst e_cpu %.2e (recorded %.1e)" % (key, v, listed[key]))
        assert v > TOL32 / 3, (key, v)      # (a block that no longer needs its listing loses it)


@pytest.mark.parametrize("name", list(blocks.BOUND_SHAPES))
def test_at_the_upper_bounds_the_cpu_bar_cannot_hide_a_failure(name):
    """blocks.BOUND_SHAPES hold every block to max(TOL32, 4 e_cpu): (a) every block that is no bias block of W has e_cpu <= 2 TOL32 at
    every step, so no such block's GPU bar exceeds 8 TOL32; (b) at least half of the blocks and columns have e_cpu <= TOL32 / 3 at every
    step and keep the plain TOL32.  A shape that breaks one gets other inputs, the conditions stay"""
    ref = cpu_reference(name)
    worst = {}
    for k, st in enumerate(ref["steps"]):
        assert set(st["e_cpu"]) == set(PARAM_Q) | set(TAP_Q)
        for q, devs in st["e_cpu"].items():
            for b, v in devs.items():
                if v != "zero":
                    worst[(q, b)] = max(worst.get((q, b), 0.0), v)
                    assert (q == "W" and b.endswith(".B")) or v <= 2 * TOL32, (k, q, b, v)
    nBlocks = sum(len(d) for d in ref["steps"][0]["e_cpu"].values())
    plain = nBlocks - sum(1 for v in worst.values() if v > TOL32 / 3)
    for key, v in sorted(worst.items(), key=lambda kv: -kv[1])[:8]:
        print("%s: worst e_cpu %.2e" % (key, v))
    print("%d of %d blocks and columns keep the plain TOL32" % (plain, nBlocks))
    assert 2 * plain >= nBlocks, (plain, nBlocks)
    assert all(blocks.bar(name, q, b, v) == max(TOL32, 4 * v) for (q, b), v in worst.items())
    assert "listed" not in blocks.BOUND_SHAPES[name] and name not in SHAPES


def _doctored(ref, q, block, rel=1e-4):
    """(O32's snapshot of step 1 with rel x the block's largest reference element added to the block's first element, the doctored
    array); `block` is a parameter block's name or a tap column "c<j>\""""
    st = ref["steps"][0]
    g = dict(st["s32"])
    a = np.array(g[q], copy=True)
    if q in PARAM_Q:
        (start, n), = [(s, n) for b, s, n in ref["blocks"] if b == block]
        i = start if np.ndim(start) == 0 else start[0]
        sl = slice(start, start + n) if np.ndim(start) == 0 else start
        a[i] += rel * np.abs(np.asarray(st["s64"][q])[sl]).max()
    else:
        j = int(block[1:])
        v = a.reshape(a.shape[0], -1)
        v[0, j] += rel * np.abs(np.asarray(st["s64"][q]).reshape(a.shape[0], -1)[:, j]).max()
    g[q] = a
    return g, a


# one `Tanh` LSTM shape with a residual between its layers, one shape behind convolutions; per shape: a recurrent-weight block of one gate
# in gradSum, the residual's weights in M1, a bias block of W that the shape does not list, a small column of outGrad
DOCTORED = {
    "lstm-320x272-app2-tm": [("gradSum", "L1.lstm.Wr.cell"), ("M1", "L3.res.W"), ("W", "L2.lstm.B"), ("outGrad", "c1")],
    "conv-lstm288-b12": [("gradSum", "L3.lstm.Wr.forget"), ("M1", "L4.res.W"), ("W", "L3.lstm.B"), ("outGrad", "c2")],
}


@pytest.mark.parametrize("name", list(DOCTORED))
def test_judge_names_the_one_block_that_is_off_by_a_ten_thousandth(name):
    """blocks.judge is what the GPU test asserts.  O32's own snapshot of step 1 passes it; with 1e-4 of a block's largest reference
    element added to ONE element of ONE block it names exactly that block -- ten bars, on the block's own scale.  The recurrent-weight
    block's largest gradient is 2e-4 (3e-5 behind the convolutions) of the vector's: under relinf(whole vector) < TOL32, the bar of
    the route tests, the doctored gradient passes"""
    ref = cpu_reference(name)
    st = ref["steps"][0]
    before = {q: np.array(st["s32"][q], copy=True) for q, _ in DOCTORED[name]}
    assert blocks.judge(name, 0, dict(st["s32"]), st, ref["blocks"]) == []
    for q, block in DOCTORED[name]:
        assert (q, block) not in SHAPES[name].get("listed", {})
        g, a = _doctored(ref, q, block)
        problems = blocks.judge(name, 0, g, st, ref["blocks"])
        print(problems)
        assert len(problems) == 1 and problems[0].startswith("step 1 %s %s: e_hip" % (q, block)), problems
        if ".Wr." in block:
            print("whole-vector deviation of the doctored %s: %.2e" % (q, relinf(a, st["s64"][q])))
            assert relinf(a, st["s64"][q]) < TOL32      # (the old bar does not see it)
    assert all(np.array_equal(st["s32"][q], a) for q, a in before.items())      # (the shared reference is left as it was)


def rec_route_names():
    """every name rec_route_name (smarties_amd/csrc/rec.hip) can print: its formats, the kernels without template arguments in both
    directions and both gate counts, the templated ones with the arguments tests/test_hip_rec_sample_kernels.py::SHAPES lists"""
    import test_hip_rec_sample_kernels as sample_kernels
    src = open(os.path.join(ROOT, "smarties_amd", "csrc", "rec.hip")).read()
    body = src[src.index("std::string rec_route_name("):]
    body = body[:body.index("\n}\n")]
    fmts = re.findall(r'snprintf\(t,\s*sizeof\(t\),\s*"([^"]+)"', body)
    assert len(fmts) == len(set(fmts)) == 7 and body.count("case REC_") == 6, fmts      # (a new kind or form shows up here first)
    for word in ('"backward"', '"forward"', '"mgu"', '"lstm"', '"true"', '"false"'):
        assert word in body, word
    listed = set(n for v in sample_kernels.SHAPES.values() for n in v[4:6])
    names, seen = set(), set()
    for f in fmts:
        if "<" not in f:      # launch_rec_tm_%s, %s32_%s_wave_kernel
            assert f.count("%s") in (1, 2) and f.count("%") == f.count("%s"), f
            for d in ("forward", "backward"):
                names |= {f % d} if f.count("%s") == 1 else {f % (k, d) for k in ("mgu", "lstm")}
            continue
        rx = re.compile("^" + re.escape(f).replace("%s", r"(\w+)").replace("%d", r"(\d+)") + "$")
        hit = set(n for n in listed if rx.match(n))
        assert hit, f      # (every templated kernel family has a case there)
        if f.startswith("lstm_"):      # (a format per direction)
            assert all(("backward" in n) == ("backward" in f) for n in hit), (f, hit)
        else:
            assert {rx.match(n).group(1) for n in hit} == {"forward", "backward"}, (f, hit)
        names |= hit; seen |= hit
    assert seen == listed, listed - seen      # (and every case there is a name the source can print)
    return names


def test_every_recurrent_kernel_is_some_shapes_rec_route_or_is_excused():
    """rec_forward / rec_backward are the timers' names of fifteen per-sample instantiations, the wave kernels and all of rectm.hip, so
    test_every_counter_fires_in_some_shape_or_is_excused cannot tell them apart: every name rec_route_name can print is the stated (and,
    on the GPU, checked) rec_route of at least one shape, or in blocks.REC_EXCUSED with a reason and a test of the suite that runs it"""
    names = rec_route_names()
    assert len(names) == 2 + 4 + 25, sorted(names)      # rectm.hip's two launchers, four wave kernels, 13 + 12 per-sample instantiations
    stated = {}
    for name in list(SHAPES) + list(blocks.BOUND_SHAPES):
        sh = blocks.shape(name)
        if "rec_route" in sh:
            fwd, bwd = sh["rec_route"]
            assert "forward" in fwd and "backward" in bwd, name
            assert "rec_forward" in blocks.ROUTES[name] and "rec_backward" in blocks.ROUTES[name], name      # (a launch of its own: not the one-launch step)
            stated.setdefault(fwd, name); stated.setdefault(bwd, name)
        if "conv_rec_dx" in sh:
            assert sh["conv_rec_dx"] in ((0, 0), (0, 1), (1, 1)) and sh["kw"].get("conv") and "rec_route" in sh, name
        if "ref" in sh:      # (the same configuration under another environment)
            twin = blocks.shape(sh["ref"])
            assert all(sh[k] == twin[k] for k in ("kw", "sc", "n_eps")) and sh.get("env") != twin.get("env") and "ref" not in twin, name
    assert set(stated) - names == set(), set(stated) - names      # (no stale name)
    assert set(blocks.REC_EXCUSED) <= names and set(blocks.REC_EXCUSED) & set(stated) == set()
    assert names - set(stated) - set(blocks.REC_EXCUSED) == set(), names - set(stated) - set(blocks.REC_EXCUSED)
    for n, (why, by) in blocks.REC_EXCUSED.items():
        path, test = by.split("::")
        assert why and re.search(r"^def %s\(" % re.escape(test), open(os.path.join(ROOT, path)).read(), re.M), (n, by)
    # both forms of the gradient into the feature rows have a shape
    assert {blocks.shape(n)["conv_rec_dx"] for n in SHAPES if "conv_rec_dx" in blocks.shape(n)} >= {(0, 1), (1, 1)}


def test_replay_fields_of_both_builds_agree():
    """what four steps wrote back into the replay: per field over all episodes within TOL32 / 3 of its largest entry"""
    for name in SHAPES:
        ref = cpu_reference(name) if name in ("fused-2x32-b16", "lstm-2x32-wave", "discrete18-2x128-b40", "conv-atari-18opt-b8", "per-rank-2x32-b16") else None
        if ref is None:
            continue
        for f, v in ref["fields64"].items():
            assert relinf(ref["fields32"][f], v) <= TOL32 / 3, (name, f)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def step_exec_counters():
    """every name smarties_amd/csrc/step_exec.h passes to timed(h, ...): the literals, and the snprintf families with every layer index"""
    src = open(os.path.join(ROOT, "smarties_amd", "csrc", "step_exec.h")).read()
    hdr = open(os.path.join(ROOT, "include", "smarties_hip.h")).read()
    nMax = max(int(m) for m in re.findall(r"#define\s+HL_MAX_(?:HIDDEN|CONV)\s+(\d+)", hdr))
    args = re.findall(r"\btimed\(h,\s*([^,]+),", src)
    assert len(args) > 50 and set(a for a in args if not a.startswith('"')) == {"nm"}, sorted(set(args))      # (a literal, or the formatted buffer)
    names = set(a.strip('"') for a in args if a.startswith('"'))
    fmts = set(re.findall(r'snprintf\(nm,\s*sizeof\(nm\),\s*"([^"]+)"', src))
    assert fmts and all(f.count("%d") == 1 and f.count("%") == 1 for f in fmts), fmts
    for f in fmts:
        names |= set(f % j for j in range(nMax))
    return names


def test_route_counters_are_the_names_step_exec_times():
    """blocks.ROUTE_COUNTERS is what a route is read from: a launch timed under a name it lacks would fire unseen in every route"""
    names = step_exec_counters()
    for fam in ("gemm16_fwd", "gemm16_dx", "conv_fwd", "conv_dx"):
        assert fam + "0" in names and fam + "7" in names, fam
    assert len(set(blocks.ROUTE_COUNTERS)) == len(blocks.ROUTE_COUNTERS)
    assert names - set(blocks.ROUTE_COUNTERS) == set()
    assert set(blocks.ROUTE_COUNTERS) - names == set()      # (and no stale name that nothing can fire)


def test_every_counter_fires_in_some_shape_or_is_excused():
    """"one shape per launch route" kept honest: every counter is in the recorded route of at least one shape, or in blocks.EXCUSED with
    an allowed reason and a test of the suite that runs the launch; the counters a shape is there for are in its recorded route"""
    fired = set()
    for name in list(SHAPES) + list(blocks.BOUND_SHAPES):
        assert name in blocks.ROUTES, name      # (every shape has a recorded route)
        assert set(blocks.ROUTES[name]) <= set(blocks.ROUTE_COUNTERS), name
        fired |= set(blocks.ROUTES[name])
    assert set(blocks.EXCUSED) <= set(blocks.ROUTE_COUNTERS)
    assert fired & set(blocks.EXCUSED) == set()
    assert set(blocks.ROUTE_COUNTERS) - fired - set(blocks.EXCUSED) == set()
    for c, (why, by) in blocks.EXCUSED.items():
        assert why in ("exchange", "periodic", "repeat", "unreachable"), c
        if why == "unreachable":      # (the loops that format these names start at layer 1: nothing can run them)
            assert by is None and c in ("gemm16_dx0", "conv_dx0"), c
            continue
        path, test = by.split("::")
        assert re.search(r"^def %s\(" % re.escape(test), open(os.path.join(ROOT, path)).read(), re.M), (c, by)
    for name, (must, must_not) in blocks.REQUIRED.items():
        route = blocks.ROUTES[name]
        assert must and all(c in route for c in must), (name, [c for c in must if c not in route])
        assert not any(c in route for c in must_not), (name, [c for c in must_not if c in route])
    assert set(blocks.ROWS_KIND) <= set(n for n in SHAPES if "conv_fwd0" in blocks.ROUTES[n])


def test_blockdev_sees_a_zeroed_layer_that_relinf_does_not():
    """M2 of the headline net after the first step of tests/golden/ns_shape.bin (the minibatch the reference drew) with the second
    hidden layer's weight block zeroed: under the norm of the whole vector that is below the 2 TOL32 the parity tests allow; per
    block it is a deviation of 1"""
    fx = load_fixture("ns_shape.bin")
    O = oracle_learner(fixture_config(fx))
    setup_from_fixture(O, fx)
    flat = flat_for(O, fx["s1_tag"], fx["s1_t"])
    O.step(1, flat=flat[np.argsort(flat, kind="stable")])
    m2 = O.get_params()[2]
    blk = param_blocks(O)
    O.close()
    assert relinf(m2, fx["s1_M2"]) < 2 * TOL32      # (the bar the suite holds M2 to)
    (bname, start, n), = [b for b in blk if b[0] == "L2.dense.W"]
    assert n == 256 * 256
    bad = m2.copy()
    bad[start:start + n] = 0
    assert relinf(bad, m2) < 2 * TOL32
    d = blockdev(blk, bad, m2)
    assert d[bname] == 1.0
    assert all(v == 0.0 for b, v in d.items() if b != bname)


def test_block_helpers_cover_the_parameter_vector_and_report_zero_blocks():
    """every parameter but the SIMD padding belongs to exactly one block; recurrent layers are split per gate into input and
    recurrent weights; a reference block of zeros is reported as "zero" and tolerates no non-zero entry"""
    for name in ("fused-2x32-b16", "lstm-24x24-bptt5", "mgu-48x32", "rnn-24x16", "conv-small", "encoder-24-16x16-b20"):
        O = oracle_learner(blocks.capi.make_config(**SHAPES[name]["kw"]))
        blk, lay = param_blocks(O), O.layout()
        seen = np.zeros(O.nParams, np.int32)
        for _, start, n in blk:
            seen[slice(start, start + n) if np.ndim(start) == 0 else start] += 1
        assert seen.max() == 1 and seen.sum() == int(lay["nW"].sum() + lay["nB"].sum()), name
        O.close()
    names = [b[0] for b in param_blocks(oracle_learner(blocks.capi.make_config(**SHAPES["lstm-24x24-bptt5"]["kw"])))]
    assert [n for n in names if n.startswith("L1.")] == ["L1.lstm.Wx.cell", "L1.lstm.Wx.in", "L1.lstm.Wx.forget", "L1.lstm.Wx.out",
                                                         "L1.lstm.Wr.cell", "L1.lstm.Wr.in", "L1.lstm.Wr.forget", "L1.lstm.Wr.out", "L1.lstm.B"]
    ref = np.zeros(8); ref[4:] = 1.0
    assert blockdev([("a", 0, 4), ("b", 4, 4)], ref, ref) == {"a": "zero", "b": 0.0}
    assert blocks.coldev(np.zeros((3, 2)), np.zeros((3, 2))) == {"c0": "zero", "c1": "zero"}
    with pytest.raises(AssertionError):
        blockdev([("a", 0, 4)], ref + 1e-30, ref)
    with pytest.raises(AssertionError):
        blocks.coldev(np.full((3, 1), 1e-30), np.zeros((3, 1)))
    assert N_STEPS == 4
