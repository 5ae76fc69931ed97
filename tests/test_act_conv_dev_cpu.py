"""Acting from device memory for feed-forward nets behind convolutions (hl_forward_sequences_dev, hl_select_actions_sequences_dev of
include/smarties_hip_dev.h), the part that needs no GPU: the resource remarks of the two kernels of smarties_amd/csrc/actconv.hip, the
header's text, and the agreement of the measured profile with DESIGN.md's bullet."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_both_conv_stack_kernels_build_without_scratch_or_spills():
    """act_conv_kernel (rows in pinned staging) and act_conv_dev_kernel (windows in device memory): no scratch, no vector register
    spilled to memory, no scalar register parked in vector lanes"""
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = resource_usage.kernels().get("actconv.hip")
    assert rows, "no resource remarks of actconv.hip beside the objects"
    assert sorted(k["name"] for k in rows) == ["act_conv_dev_kernel", "act_conv_kernel"], rows
    for k in rows:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k


def test_dev_header_names_conv_nets_as_served():
    dev = open(os.path.join(ROOT, "include", "smarties_hip_dev.h")).read()
    at = dev.index("hl_forward_sequences for windows in device memory")
    text = dev[at:dev.index("HL_API int hl_forward_sequences_dev", at)]
    served = re.search(r"Served, feed-forward nets behind convolutions:(.*?)(?:\n \*\n| \* Served,| \* Status:)", text, re.S)
    assert served, "no 'Served' paragraph for nets behind convolutions"
    assert "act_conv_dev_kernel" in served.group(1) and "bit for bit" in served.group(1)
    # the row calls keep refusing them and say where to go
    rows = dev[dev.index("hl_forward for rows in device memory"):dev.index("HL_API int hl_forward_dev")]
    assert "convolutions in front (hl_forward_sequences_dev" in rows


def test_timing_profile_and_design_bullet_agree():
    """every median of profiles/act_conv_dev_timing.json stands, to a tenth of a microsecond, in DESIGN.md's bullet -- which says so in
    the words "NOT faster" wherever the device route does not complete below what a GPU simulator pays for the host call"""
    prof = json.load(open(os.path.join(ROOT, "profiles", "act_conv_dev_timing.json")))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    at = design.index("**Acting from device memory behind convolutions**")
    assert at > design.index("**Recurrent acting from device memory**")
    bullet = design[at:design.index("### 4.5", at)]
    assert "profiles/act_conv_dev_timing.json" in bullet and "tools/act_conv_dev_timing.py" in bullet
    assert prof["rounds"] >= 5 and prof["shape"].startswith("RACER_atari.json")
    assert set(prof["forward_us"]) == {"64", "256", "1024"}
    for n, d in prof["forward_us"].items():
        assert set(d) == {"host", "host_from_tensor", "dev_enqueue", "dev_complete", "select_complete"}
        for k, v in d.items():
            assert v["min"] <= v["median"] <= v["max"]
            assert "%.1f" % v["median"] in bullet, (n, k)
        if d["dev_complete"]["median"] >= d["host_from_tensor"]["median"]:
            assert "NOT faster" in bullet, n
    for n, d in prof["kernel_us"].items():      # the device time of a call's launches
        assert set(d) == {"act_conv_dev", "act_rows_dev"}
        for k, v in d.items():
            assert "%.1f" % v["median"] in bullet, (n, k)
