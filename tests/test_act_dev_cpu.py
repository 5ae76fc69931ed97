"""Acting and episode ingestion from device memory (include/smarties_hip_dev.h), the part that needs no GPU: the header and the
exported symbols, the null-handle refusals, the resource remarks of the two new kernels (smarties_amd/csrc/actdev.hip), and the numpy
fp64 restatement of RACER::selectAction's three heads (tests/acting.py: head_np) that tests/test_hip_act_dev.py holds the device head to -- pinned here against
values worked out by hand for one agent per head."""
import ctypes as C
import os
import re
import sys

import numpy as np

from acting import CLIP, _net2v, head_np
from smarties_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("hl_forward_dev", "hl_select_actions_dev", "hl_append_episodes_dev")


# ---- 1. the checker against hand-computed values -----------------------------------------------------------------------------------
# SoftPlus(0.75) = (0.75 + 1.25) / 2 = 1, SoftPlus(0) = 0.5, SoftPlus(-0.75) = 0.25, SoftPlus(1.875) = (1.875 + 2.125) / 2 = 2;
# scaleNet2V(1.03) = 100 x 52.03 - 100 sqrt(2704) = 3, scaleNet2V(-1.03) = -3, scaleNet2V(0) = 0
def test_checker_vracer_head_by_hand():
    out = [1.03, 8.0, -0.5, 0.25, 0.75, 0.0, 1.875]      # V | mean x 3 | stdev pre-images x 3
    act, mu, v, a = head_np(out, [1.0, 2.0, -0.5], 3, bounded=[1, 0, 1])
    # 8 + 1 x 1 = 9 is past the clip of the bounded component 0; -0.5 + 0.5 x 2 = 0.5; 0.25 + 2 x (-0.5) = -0.75 stays inside
    assert np.allclose(act, [CLIP, 0.5, -0.75], rtol=1e-15, atol=0) and act[0] == CLIP
    assert np.allclose(mu, [8.0, -0.5, 0.25, 1.0, 0.5, 2.0], rtol=1e-15, atol=0)
    assert abs(float(v) - 3.0) < 1e-6 and a == 0
    act, mu, v, a = head_np(out, None, 3, bounded=[1, 0, 1])      # the evaluation action: the mean, not clipped (Continuous_policy.h:779)
    assert np.array_equal(act, [8.0, -0.5, 0.25]) and a == 0


def test_checker_gaussian_head_by_hand():
    out = [-1.03, 0.75, 0.75, -0.75, 0.5, 0.75]           # V | coef, L+, L- | mean | stdev pre-image
    act, mu, v, a = head_np(out, [1.0], 1, gaussian=True)
    assert act[0] == 1.5 and np.array_equal(mu, [0.5, 1.0])
    # a > mean: quad = 1 / L+ = 1; ratio = sqrt(1 / 2) / 2 + sqrt(0.25 / 1.25) / 2; A = 1 x (exp(-1/2) - ratio)
    A = 0.6065306597126334 - (0.35355339059327373 + 0.22360679774997896)
    assert abs(float(v) + 3.0) < 1e-6
    assert a == np.float32(np.float32(_net2v(-1.03) + A) - np.float32(_net2v(-1.03)))
    assert abs(float(a) - 0.0293704713693807) < 3e-7      # (one float ulp of the operands, |V| = 3)
    act, mu, v, a0 = head_np(out, None, 1, gaussian=True)      # the mean: quad = 0, A = 1 - ratio
    assert act[0] == 0.5 and abs(float(a0) - (1 - 0.5771601883432527)) < 3e-7


def test_checker_discrete_head_by_hand():
    out = [0.0, 1.0, 2.0, 4.0, 0.75, 0.0, -0.75]          # V | A x 3 | logits x 3: SoftPlus 1, 0.5, 0.25 -> p = 4/7, 2/7, 1/7
    act, mu, v, a = head_np(out, 0.7, 1, n_options=3)     # running sums 0.571, 0.857: option 1 is the first beyond 0.7
    assert np.allclose(mu, [4 / 7, 2 / 7, 1 / 7], rtol=1e-15, atol=0)
    assert act[0] == 1.1 and v == 0 and abs(float(a) - 2 / 7) < 1e-7      # A[1] - sum p A = 2 - 12/7
    act, mu, v, a = head_np(out, 0.0, 1, n_options=3)
    assert act[0] == 0.1
    act, mu, v, a = head_np(out, 0.999, 1, n_options=3)
    assert act[0] == 2.1 and abs(float(a) - (4 - 12 / 7)) < 3e-7
    act, mu, v, a = head_np(out, None, 1, n_options=3)    # the arg-max option
    assert act[0] == 0.1 and abs(float(a) - (1 - 12 / 7)) < 1e-7


# ---- 2. the surface ----------------------------------------------------------------------------------------------------------------
def test_dev_header_declares_the_entry_points_and_the_main_header_none():
    dev = open(os.path.join(ROOT, "include", "smarties_hip_dev.h")).read()
    main = open(os.path.join(ROOT, "include", "smarties_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"HL_API\s+int\s+%s\s*\(" % name, dev), name
        assert name not in main, name      # (tests/test_cabi_symbols.py wants an oracle twin of everything declared there)


def test_library_exports_the_entry_points_and_refuses_a_null_handle():
    import __graft_entry__ as ge
    ge.build_hip()
    api = capi.load_hip()
    for name in ENTRY_POINTS:
        assert api.has(name[3:]), name
    null = C.c_void_p()
    assert api.fn("forward_dev")(null, 1, None, None, None) == 1                                  # HL_ERR_BAD_ARG
    assert api.fn("select_actions_dev")(null, 1, None, None, None, None, None, None, None) == 1
    assert api.fn("append_episodes_dev")(null, 0, None, None, None, None, 1, None, None, None, None, None, None, None) == 1


def test_timing_profile_and_design_bullet_agree():
    """every median of profiles/act_dev_timing.json stands, to a tenth of a microsecond, in DESIGN.md's bullet -- which says so where the
    device route is not faster than its host twin"""
    import json
    prof = json.load(open(os.path.join(ROOT, "profiles", "act_dev_timing.json")))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    at = design.index("**Acting and ingestion from device memory**")
    bullet = design[at:design.index("### 4.5", at)]
    assert "profiles/act_dev_timing.json" in bullet and "tools/act_dev_timing.py" in bullet
    assert prof["rounds"] >= 5 and set(prof["forward_us"]) == {"1024", "16384"} and prof["episodes"] == 64 and prof["episode_steps"] == 200
    for n, d in prof["forward_us"].items():
        assert set(d) == {"host", "host_from_tensor", "dev_enqueue", "dev_complete", "select_complete"}
        for k, v in d.items():
            assert v["min"] <= v["median"] <= v["max"]
            assert "%.1f" % v["median"] in bullet, (n, k)
        if d["dev_complete"]["median"] >= d["host"]["median"]:
            assert "NOT faster" in bullet, n
    for k, v in prof["ingest_us"].items():
        assert "%.1f" % v["median"] in bullet, k


def test_dev_kernels_build_without_scratch():
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = resource_usage.kernels().get("actdev.hip")
    assert rows, "no resource remarks of actdev.hip beside the objects"
    names = {k["name"] for k in rows}
    assert {"act_head_kernel", "ingest_dev_kernel"} <= names, names
    for k in rows:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
