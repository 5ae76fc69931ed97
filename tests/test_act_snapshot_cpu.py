"""Acting on a policy snapshot (include/smarties_hip_dev.h: hl_policy_snapshot, hl_policy_snapshot_info, hl_act_dev_source), the part that
needs no GPU: the header declares the three calls and the two source constants, the main header none of them, the built library exports
them, each refuses a null handle, and the copy kernel is built without scratch."""
import ctypes as C
import os
import re
import sys

from smarties_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("hl_policy_snapshot", "hl_policy_snapshot_info", "hl_act_dev_source")


def test_dev_header_declares_the_snapshot_calls_and_the_main_header_none():
    dev = open(os.path.join(ROOT, "include", "smarties_hip_dev.h")).read()
    main = open(os.path.join(ROOT, "include", "smarties_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"HL_API\s+int\s+%s\s*\(" % name, dev), name
        assert name not in main, name      # (tests/test_cabi_symbols.py wants an oracle twin of everything declared there)
    assert re.search(r"enum\s*\{\s*HL_ACT_LIVE\s*=\s*0\s*,\s*HL_ACT_SNAPSHOT\s*=\s*1\s*\}", dev)
    assert (capi.ACT_LIVE, capi.ACT_SNAPSHOT) == (0, 1)


def test_library_exports_the_snapshot_calls_and_refuses_a_null_handle():
    import __graft_entry__ as ge
    ge.build_hip()
    api = capi.load_hip()
    for name in ENTRY_POINTS:
        assert api.has(name[3:]), name
    null = C.c_void_p()
    n, g = C.c_int64(), C.c_int64()
    assert api.fn("policy_snapshot")(null) == 1                                  # HL_ERR_BAD_ARG
    assert api.fn("policy_snapshot_info")(null, C.byref(n), C.byref(g)) == 1
    assert api.fn("act_dev_source")(null, capi.ACT_SNAPSHOT) == 1
    assert api.fn("act_dev_source")(null, capi.ACT_LIVE) == 1


def test_timing_profile_and_design_bullet_agree():
    """every median of profiles/act_snapshot_timing.json stands in DESIGN.md's bullet (latencies to a tenth of a microsecond, steps to a
    hundredth) -- which says so in the words "NOT faster" where the snapshot source does not complete below the live one on an idle learner"""
    import json
    prof = json.load(open(os.path.join(ROOT, "profiles", "act_snapshot_timing.json")))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    at = design.index("**Acting on a policy snapshot while gradient steps run**")
    assert at > design.index("**Acting and ingestion from device memory**")
    bullet = design[at:design.index("### 4.5", at)]
    assert "profiles/act_snapshot_timing.json" in bullet and "tools/act_snapshot_timing.py" in bullet
    assert prof["rounds"] >= 5 and prof["steps"] == 2000 and set(prof["nets"]) == {"cfg-NS", "atari"}
    assert prof["nets"]["cfg-NS"]["agents"] == 64 and prof["nets"]["atari"]["agents"] == 256

    def ordered(v):
        return v["min"] <= v["median"] <= v["max"]

    for name, d in prof["nets"].items():
        assert d["device_failure_code"] is False, name
        for src in ("live", "snapshot"):
            assert ordered(d["idle_us"][src]) and "%.1f" % d["idle_us"][src]["median"] in bullet, (name, src)
            for k in ("act", "drain"):
                v = d["backlog_us"][src][k]
                assert ordered(v) and "%.1f" % v["median"] in bullet, (name, src, k)
        if d["idle_us"]["snapshot"]["median"] >= d["idle_us"]["live"]["median"]:
            assert "NOT faster" in bullet, name
        assert set(d["interference_us_per_step"]) == {"alone", "64", "1024"}
        for k, v in d["interference_us_per_step"].items():
            assert ordered(v) and "%.2f" % v["median"] in bullet, (name, k)
        assert "%.1f" % d["policy_snapshot_us"] in bullet, name
        # the claim the feature makes: behind the backlog the snapshot source does not wait for the steps
        assert d["backlog_us"]["snapshot"]["act"]["median"] < d["backlog_us"]["snapshot"]["drain"]["median"] / 2 <= d["backlog_us"]["live"]["act"]["median"]
    limits = design[design.index("## 8. Limits"):]
    assert "HL_ACT_LIVE" in limits and "hl_policy_snapshot" in limits


def test_snapshot_kernel_builds_without_scratch():
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = {k["name"]: k for k in resource_usage.kernels().get("actdev.hip")}
    assert "policy_snapshot_kernel" in rows, sorted(rows)
    for k in rows.values():      # the kernels the file held before keep their figures' zeros too
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
