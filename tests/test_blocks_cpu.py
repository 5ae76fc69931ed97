"""The yardstick of tests/test_hip_blocks.py, pinned on the CPU: the fp32 restatement (O32, oracle/liboracle_port.so) against its
build with the arrays in double (O64, oracle/liboracle_port64.so) on every shape of tests/blocks.py, four steps from the same
weights, each drawing its own minibatches; and the claim "one shape per launch route" held to the names step_exec.h times."""
import os
import re

import numpy as np
import pytest

import blocks
from blocks import N_STEPS, PARAM_Q, SHAPES, TAP_Q, TOL32, cpu_reference
from oracle_api import oracle_learner
from parity import blockdev, fixture_config, flat_for, load_fixture, param_blocks, relinf, setup_from_fixture


@pytest.mark.parametrize("name", list(SHAPES))
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
    for name in SHAPES:
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
