"""Three-way comparison per launch route of the training step: the HIP library (G), the fp32 restatement (O32) and its build with
the arrays in double (O64), from the same fp32 weights and the same synthetic replay, four single steps, every parameter block
and every tap column on its own scale (tests/blocks.py, tests/parity.py: blockdev, coldev).

e_hip(b) = dev(G, O64) is held to TOL32 per block -- tests/test_blocks_cpu.py proves e_cpu(b) = dev(O32, O64) <= TOL32 / 3 for the
same inputs -- or to 4 e_cpu(b) for the few blocks a shape lists as ill-conditioned.  The first two steps run as the suite's other
tests run them (the captured single-step graph); the last two run with the launch timers on, which makes them eager launches
and counts them: the counters that fire, and how often, are the shape's route, and a shape that takes another one fails; so does
one whose first convolutional layer takes another form of the row-block kernels than blocks.ROWS_KIND states, or whose recurrent
launches or gradient into the feature rows take another kernel than the shape's `rec_route` / `conv_rec_dx` state (the timers
give every recurrent kernel one name).  What a step is judged by is blocks.judge, which tests/test_blocks_cpu.py feeds doctored snapshots."""
import numpy as np
import pytest

from smarties_amd import capi
import blocks
from blocks import N_STEPS, ROUTE_COUNTERS, SHAPES, TOL32, cpu_reference
from parity import conv_rec_dx_form, relinf

pytestmark = pytest.mark.gpu
N_TIMED = 2      # the last steps, with the timers on


def run_case(hip_api, name, monkeypatch=None):
    """-> (problems, report): what is wrong (nothing, in a passing test) and the figures worth printing"""
    sh = blocks.shape(name)
    ref = cpu_reference(name)
    for var, value in sh.get("env", {}).items():      # (read where the learner is created; the CPU restatement has been stepped by now)
        monkeypatch.setenv(var, value)
    G, = blocks.make_learners([lambda cfg: capi.Learner(hip_api, cfg)], name, params=ref["params0"])
    problems, report = [], []
    assert np.array_equal(G.get_rng_state(), ref["rng0"])
    for k, st in enumerate(ref["steps"]):
        if k == N_STEPS - N_TIMED:
            G.timing_enable(True)
        G.step(1)
        problems += blocks.judge(name, k, blocks.snapshot(G), st, ref["blocks"], report)
    counts = {c: G.timing_get(c)[1] for c in ROUTE_COUNTERS}
    G.timing_enable(False)
    route = {c: n / N_TIMED for c, n in counts.items() if n}
    report.append("route: %r" % ({c: (int(n) if n == int(n) else n) for c, n in route.items()},))
    if route != sh.get("route"):
        problems.append("route %r, expected %r" % (route, sh.get("route")))
    # (conv_fwd0 / conv_dw_* count launches of either form of the row-block kernels: which one is the learner's to say)
    kind = G.debug_conv_rows_kind()
    report.append("row-block kernels of the first convolutional layer: %d" % kind)
    if kind != blocks.ROWS_KIND.get(name, -1):
        problems.append("row-block kernel form %d, expected %d" % (kind, blocks.ROWS_KIND.get(name, -1)))
    # (rec_forward / rec_backward time every recurrent kernel, gemm16_dx<n> both forms of the gradient into the feature rows: the
    #  learner says which, for the shapes that state what they are there for)
    if "rec_route" in sh:
        rec = (G.debug_rec_route(False), G.debug_rec_route(True))
        report.append("rec_route: %r" % (rec,))
        if rec != tuple(sh["rec_route"]):
            problems.append("recurrent kernels %r, expected %r" % (rec, tuple(sh["rec_route"])))
    if "conv_rec_dx" in sh:
        form = conv_rec_dx_form(G)
        report.append("conv_rec_dx: %r" % (form,))
        if form != tuple(sh["conv_rec_dx"]):
            problems.append("gradient into the feature rows: form %r, expected %r" % (form, tuple(sh["conv_rec_dx"])))
    fields = blocks.episode_fields(G)
    for f, v in ref["fields64"].items():
        d = relinf(fields[f], v)
        report.append("replay %-7s dev %.2e (O32: %.2e)" % (f, d, relinf(ref["fields32"][f], v)))
        if not d <= TOL32:
            problems.append("replay field %s: %.3e" % (f, d))
    G.close()
    return problems, report


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_block_and_column_against_fp64(hip_api, name, monkeypatch):
    problems, report = run_case(hip_api, name, monkeypatch)
    print("\n".join(report))
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("name", list(blocks.BOUND_SHAPES))
def test_the_upper_bounds_against_fp64_with_every_bar_taken_from_the_cpu(hip_api, name, monkeypatch):
    """1024 cells and 8192 input floats: the fp32 restatement itself loses more than TOL32 / 3 in many blocks (summation length), so
    every block and column is held to max(TOL32, 4 e_cpu) of its step; tests/test_blocks_cpu.py holds e_cpu of these shapes to the
    conditions that keep that rule from hiding a failure"""
    problems, report = run_case(hip_api, name, monkeypatch)
    print("\n".join(report))
    assert not problems, "\n".join(problems)
