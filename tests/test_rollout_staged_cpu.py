"""The rollout's staging ring (include/smarties_hip_rollout.h: hl_rollout_staging, hl_rollout_stage_info), the part that needs no GPU: the
header and the exported symbols, the refusals in front of the device, the ring's arithmetic under the sanitizers against a brute-force
restatement, the Python restatement the GPU tests take their expected counts from, the new kernel's resources, and DESIGN.md's bullet
against the committed profile."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

import rollout_staged as S
from smarties_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("hl_rollout_staging", "hl_rollout_stage_info")


def _api():
    import __graft_entry__ as ge
    ge.build_hip()
    return capi.load_hip()


def test_header_declares_the_staging_calls_and_the_library_exports_them():
    txt = open(os.path.join(ROOT, "include", "smarties_hip_rollout.h")).read()
    main = open(os.path.join(ROOT, "include", "smarties_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"HL_API\s+int\s+%s\s*\(" % name, txt), name
        assert name not in main, name
    assert re.search(r"HL_API\s+int\s+hl_rollout_staging\s*\(\s*hl_rollout\s*\*\s*r\s*,\s*int64_t\s+rows\s*\)", txt)
    fields = re.search(r"typedef struct hl_rollout_stage_counts \{(.*?)\}", txt, re.S).group(1)
    assert re.findall(r"int64_t\s+(\w+);", fields) == [k for k, _ in capi.RolloutStageCounts._fields_]
    assert all(t is C.c_int64 for _, t in capi.RolloutStageCounts._fields_)
    # the known limits stay stated
    assert "uploads the episode table" in txt and "hl_set_episode_log" in txt
    assert "rollout_ring.h" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    api = _api()
    for name in ENTRY_POINTS:
        assert api.has(name[3:]), name
    null = C.c_void_p()
    assert api.fn("rollout_staging")(null, 64) == 1                                     # HL_ERR_BAD_ARG: a null handle, no device needed
    assert api.fn("rollout_stage_info")(null, C.byref(capi.RolloutStageCounts())) == 1


def test_ring_arithmetic_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/cpp/rollout_ring_check.cpp")
    exe = str(tmp_path / "rollout_ring_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "cpp", "rollout_ring_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "rollout_ring_check: ok" in r.stdout, r.stdout


def test_restated_ring_gives_the_counts_the_gpu_tests_expect():
    """the Python restatement (tests/rollout_staged.py), written from the header's text: the order test's 70 episodes of 2 states on 96
    rows; the toy simulator's 60 calls on 28 rows wrap, as tests/test_hip_rollout_staged.py asserts of the library"""
    want = S.expected_stage_counts(96, [[], [2] * 70])
    assert want == dict(capacity=96, batches=3, episodes=70, rows=140, wraps=1)
    ring = S.Ring(96)
    ring.call([2] * 70)
    assert [p[0] for p in ring.placed[:24]] == list(range(0, 48, 2)) and ring.placed[24][0] == 48 and ring.placed[48][0] == 0
    sched = S.toy_schedule(S.LENGTHS, S.MAX_STEPS, S.CALLS)
    assert all(2 <= n <= S.MAX_STEPS for call in sched for n in call) and max(len(c) for c in sched) >= 2
    toy = S.expected_stage_counts(28, sched)
    assert toy["episodes"] == sum(len(c) for c in sched) > 10 and toy["wraps"] >= 1
    # the backlog test: 6 episodes of 2 states on 2 maxSteps = 8 rows are three batches, the third at row 0
    assert S.expected_stage_counts(8, [[2] * 6]) == dict(capacity=8, batches=3, episodes=6, rows=12, wraps=1)
    # a batch never holds more than 64 episodes
    assert S.expected_stage_counts(4096, [[2] * 130])["batches"] == 3


def test_stage_kernel_builds_without_scratch():
    _api()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = [k for k in resource_usage.kernels().get("rollout.hip") if "rollout_stage_kernel" in k["name"]]
    assert len(rows) == 2, rows      # the 16-byte and the 4-byte form of the state rows
    for k in rows:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k


def test_snapshot_timing_profile_and_design_bullet_agree():
    """every median of profiles/rollout_snapshot_timing.json stands in DESIGN.md's bullet to a tenth of a microsecond (steps: a
    hundredth), and the bullet names every point at which the staged call is slower than the live one (or says that there is none)"""
    prof = json.load(open(os.path.join(ROOT, "profiles", "rollout_snapshot_timing.json")))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    at = design.index("**The rollout buffer under the snapshot source: staged episode hand-off**")
    bullet = design[at:design.index("### 4.5", at)]
    assert "profiles/rollout_snapshot_timing.json" in bullet and "tools/rollout_snapshot_timing.py" in bullet
    assert prof["calls"] == 200 and prof["warmup"] == 50 and prof["steps"] == 2000 and set(prof["nets"]) == {"lstm-2x32", "dense-2x256"}
    slower = []
    for name, d in prof["nets"].items():
        assert set(d) == {"64", "1024"}, name
        for n, v in d.items():
            for src in ("live", "snapshot"):
                for k in ("host_us", "device_us"):
                    q = v["idle"][src][k]
                    assert q["p25"] <= q["median"] <= q["p75"]
                    assert "%.1f" % q["median"] in bullet, (name, n, src, k)
                assert "%.1f" % v["backlog_us"][src]["median"] in bullet, (name, n, src)
            for form in ("alone", "beside_staged_calls"):
                assert "%.2f" % v["step_us"][form]["median"] in bullet, (name, n, form)
            for k in ("rollout_stage_kernel", "ingest_dev_kernel"):
                assert v["launch_us_per_call"][k] > 0 and "%.1f" % v["launch_us_per_call"][k] in bullet, (name, n, k)
            assert v["info"]["snapshot"]["no_room"] == 0 and v["stage"]["episodes"] == v["info"]["snapshot"]["episodes"]
            for col in ("host_us", "device_us"):
                if v["idle"]["snapshot"][col]["median"] > v["idle"]["live"][col]["median"]:
                    slower.append("%s n=%s %s" % (name, n, col))
            if v["backlog_us"]["snapshot"]["median"] > v["backlog_us"]["live"]["median"]:
                slower.append("%s n=%s backlog_us" % (name, n))
    assert sorted(slower) == sorted(prof["staged_slower_than_live"])
    for point in slower:
        assert point in bullet, point
    assert ("slower at none of the twelve points" in bullet) == (not slower)
