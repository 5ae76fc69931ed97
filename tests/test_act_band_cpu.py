"""Acting from device memory beyond the resident plans (smarties_amd/csrc/actband.hip, act_plan.h), the part that needs no GPU: the plans of
the banded conv-stack kernel and the panelled row-block kernel under the address and undefined-behaviour sanitizers
(tests/cpp/act_plan_check.cpp, a stand-alone program run as a child process), the resource remarks of the new kernels, the header's text, and
the agreement of the measured profile with DESIGN.md's bullet."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_band_and_panel_plans_under_sanitizers(tmp_path):
    """act_plan.h reads the argument records of kernels.h, whose launcher declarations need the HIP headers: they are only parsed here"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/cpp/act_plan_check.cpp")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "act_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "act_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "act_plan_check: ok" in r.stdout, r.stdout


def test_banded_and_panelled_kernels_build_without_scratch_or_spills():
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    ks = resource_usage.kernels()
    rows = ks.get("actband.hip")
    assert rows, "no resource remarks of actband.hip beside the objects"
    names = sorted(k["name"] for k in rows)
    assert "act_conv_band_dev_kernel" in names and any(n.startswith("act_rows_panel_kernel") for n in names), names
    assert all(n == "act_conv_band_dev_kernel" or n.startswith("act_rows_panel_kernel") for n in names), names
    for k in rows:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
    # the files the kernels' shared code was moved out of still hold their kernels alone, as clean as before
    assert sorted(k["name"] for k in ks["actconv.hip"]) == ["act_conv_dev_kernel", "act_conv_kernel"]
    assert all(k["name"].startswith("act_rows_kernel") for k in ks["actrows.hip"]) and ks["actrows.hip"]
    for k in ks["actconv.hip"] + ks["actrows.hip"]:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k


def test_dev_header_names_the_banded_and_panelled_kernels_as_served():
    from smarties_amd import capi
    dev = open(os.path.join(ROOT, "include", "smarties_hip_dev.h")).read()
    m = re.search(r"#define\s+HL_ACT_DEV_MAX_ROW\s+(\d+)", dev)
    assert m and int(m.group(1)) == capi.ACT_DEV_MAX_ROW == 8192
    at = dev.index("hl_forward_sequences for windows in device memory")
    text = dev[at:dev.index("HL_API int hl_forward_sequences_dev", at)]
    served = text[text.index("Served,"):text.index(" * Status:")]
    for word in ("act_conv_band_dev_kernel", "act_rows_panel_kernel", "HL_ACT_DEV_MAX_ROW", "Nature-DQN"):
        assert word in served, word
    status = text[text.index(" * Status:"):]
    assert "the Nature-DQN stack among them" not in status and "HL_ACT_DEV_MAX_ROW" in status
    rows = dev[dev.index("hl_forward for rows in device memory"):dev.index("HL_API int hl_forward_dev")]
    assert "act_rows_panel_kernel" in rows and "HL_ACT_DEV_MAX_ROW" in rows


def test_band_timing_profile_and_design_bullet_agree():
    """every median of profiles/act_band_timing.json stands, to a tenth of a microsecond, in DESIGN.md's bullet -- which says so in the
    words "NOT faster" wherever the device route does not complete below what a GPU simulator pays for the host call"""
    prof = json.load(open(os.path.join(ROOT, "profiles", "act_band_timing.json")))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    at = design.index("**Acting from device memory for the Nature-DQN stack and large images**")
    assert at > design.index("**Acting from device memory behind convolutions**")
    bullet = design[at:design.index("### 4.5", at)]
    assert "profiles/act_band_timing.json" in bullet and "tools/act_band_timing.py" in bullet
    assert prof["rounds"] >= 5 and prof["shape"].startswith("Nature-DQN stack") and prof["banding_shape"].startswith("RACER_atari.json")
    assert set(prof["forward_us"]) == set(prof["kernel_us"]) == set(prof["banding_us"]) == {"64", "256", "1024"}
    for n, d in prof["forward_us"].items():
        assert set(d) == {"host_from_tensor", "dev_enqueue", "dev_complete"}
        if d["dev_complete"]["median"] >= d["host_from_tensor"]["median"]:
            assert "NOT faster" in bullet, n
    for key, cols in (("forward_us", None), ("kernel_us", {"act_conv_band_dev", "act_rows_panel_dev"}), ("banding_us", {"act_conv_dev", "act_conv_band_dev"})):
        for n, d in prof[key].items():
            assert cols is None or set(d) == cols
            for k, v in d.items():
                assert v["min"] <= v["median"] <= v["max"]
                assert "%.1f" % v["median"] in bullet, (key, n, k)
