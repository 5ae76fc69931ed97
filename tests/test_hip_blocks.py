"""Three-way comparison per launch route of the training step: the HIP library (G), the fp32 restatement (O32) and its build with
the arrays in double (O64), from the same fp32 weights and the same synthetic replay, four single steps, every parameter block
and every tap column on its own scale (tests/blocks.py, tests/parity.py: blockdev, coldev).

e_hip(b) = dev(G, O64) is held to TOL32 per block -- tests/test_blocks_cpu.py proves e_cpu(b) = dev(O32, O64) <= TOL32 / 3 for the
same inputs -- or to 4 e_cpu(b) for the few blocks a shape lists as ill-conditioned.  The first two steps run as the suite's other
tests run them (the captured single-step graph); the last two run with the launch timers on, which makes them eager launches
and counts them: the counters that fire, and how often, are the shape's route, and a shape that takes another one fails; so does
one whose first convolutional layer takes another form of the row-block kernels than blocks.ROWS_KIND states."""
import numpy as np
import pytest

from smarties_amd import capi
import blocks
from blocks import N_STEPS, PARAM_Q, ROUTE_COUNTERS, SHAPES, TAP_Q, TOL32, cpu_reference
from parity import relinf

pytestmark = pytest.mark.gpu
N_TIMED = 2      # the last steps, with the timers on


def run_case(hip_api, name):
    """-> (problems, report): what is wrong (nothing, in a passing test) and the figures worth printing"""
    ref = cpu_reference(name)
    G, = blocks.make_learners([lambda cfg: capi.Learner(hip_api, cfg)], name, params=ref["params0"])
    problems, report = [], []
    assert np.array_equal(G.get_rng_state(), ref["rng0"])
    for k, st in enumerate(ref["steps"]):
        if k == N_STEPS - N_TIMED:
            G.timing_enable(True)
        G.step(1)
        s32, s64, g = st["s32"], st["s64"], blocks.snapshot(G)
        for key in list(blocks.INT_TAPS) + ["rng"]:
            if not (np.array_equal(g[key], s64[key]) and np.array_equal(g[key], s32[key])):
                problems.append("step %d: %s differs" % (k + 1, key))
        if not (g["nFar"] == s64["nFar"] == s32["nFar"] and g["CmaxRet"] == s64["CmaxRet"] == s32["CmaxRet"]):
            problems.append("step %d: nFarPolicySteps / CmaxRet differ" % (k + 1))
        if not abs(g["beta"] - s64["beta"]) <= 1e-12 * s64["beta"]:
            problems.append("step %d: beta %r against %r" % (k + 1, g["beta"], s64["beta"]))
        e_hip = blocks.deviations(ref["blocks"], g, s64)
        for q in list(PARAM_Q) + list(TAP_Q):
            w, b = blocks.worst(e_hip[q])
            report.append("step %d %-8s worst e_hip %.2e in %-22s e_cpu there %s" % (k + 1, q, w, b, st["e_cpu"][q].get(b, "-")))
            for b, v in e_hip[q].items():
                e_cpu = st["e_cpu"][q][b]
                if v == "zero" or e_cpu == "zero":
                    if v != e_cpu:
                        problems.append("step %d %s %s: %s on the device, %s on the CPU" % (k + 1, q, b, v, e_cpu))
                elif not v <= blocks.bar(name, q, b, e_cpu):
                    problems.append("step %d %s %s: e_hip %.3e over its bar %.3e (e_cpu %.3e)" % (k + 1, q, b, v, blocks.bar(name, q, b, e_cpu), e_cpu))
    counts = {c: G.timing_get(c)[1] for c in ROUTE_COUNTERS}
    G.timing_enable(False)
    route = {c: n / N_TIMED for c, n in counts.items() if n}
    report.append("route: %r" % ({c: (int(n) if n == int(n) else n) for c, n in route.items()},))
    if route != SHAPES[name].get("route"):
        problems.append("route %r, expected %r" % (route, SHAPES[name].get("route")))
    # (conv_fwd0 / conv_dw_* count launches of either form of the row-block kernels: which one is the learner's to say)
    kind = G.debug_conv_rows_kind()
    report.append("row-block kernels of the first convolutional layer: %d" % kind)
    if kind != blocks.ROWS_KIND.get(name, -1):
        problems.append("row-block kernel form %d, expected %d" % (kind, blocks.ROWS_KIND.get(name, -1)))
    fields = blocks.episode_fields(G)
    for f, v in ref["fields64"].items():
        d = relinf(fields[f], v)
        report.append("replay %-7s dev %.2e (O32: %.2e)" % (f, d, relinf(ref["fields32"][f], v)))
        if not d <= TOL32:
            problems.append("replay field %s: %.3e" % (f, d))
    G.close()
    return problems, report


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_block_and_column_against_fp64(hip_api, name):
    problems, report = run_case(hip_api, name)
    print("\n".join(report))
    assert not problems, "\n".join(problems)
