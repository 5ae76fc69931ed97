"""Recurrent acting from device memory (hl_forward_sequences_dev, hl_select_actions_sequences_dev of include/smarties_hip_dev.h), the part
that needs no GPU: the header and the exported symbols, the null-handle refusals, the resource remarks of the twelve act_seq_kernel
instantiations (smarties_amd/csrc/actseq.hip) and of act_stack_dev_kernel (actdev.hip), and the agreement of the measured profile with
DESIGN.md's bullet."""
import ctypes as C
import json
import os
import re
import sys

from smarties_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("hl_forward_sequences_dev", "hl_select_actions_sequences_dev")


def test_dev_header_declares_the_window_entry_points_and_the_main_header_neither():
    dev = open(os.path.join(ROOT, "include", "smarties_hip_dev.h")).read()
    main = open(os.path.join(ROOT, "include", "smarties_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"HL_API\s+int\s+%s\s*\(" % name, dev), name
        assert name not in main, name      # (tests/test_cabi_symbols.py wants an oracle twin of everything declared there)
    # the window rule and the one-row case are part of the contract
    assert "max(1, min(len, nnBPTTseq + 1 + nAppendedObs))" in dev and "max(len, 1) - ns" in dev
    assert "dNSteps[i] < 1 reads one row" in dev


def test_library_exports_the_window_entry_points_and_refuses_a_null_handle():
    import __graft_entry__ as ge
    ge.build_hip()
    api = capi.load_hip()
    for name in ENTRY_POINTS:
        assert api.has(name[3:]), name
    null = C.c_void_p()
    assert api.fn("forward_sequences_dev")(null, 1, None, None, 1, None, None, None) == 1                                  # HL_ERR_BAD_ARG
    assert api.fn("select_actions_sequences_dev")(null, 1, None, None, 1, None, None, None, None, None, None, None) == 1


def test_window_kernels_build_without_scratch():
    """twelve instantiations of act_seq_kernel -- LDSW x GATES as before, each with the windows in pinned staging and in device memory --
    and the row-stacking kernel: no scratch, no register spilled to memory.  (The scalar registers the six host instantiations park in
    vector lanes are the parent commit's; a device instantiation parks no more of them than its host twin.)"""
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    res = resource_usage.kernels()
    seq = {k["name"]: k for k in res.get("actseq.hip", []) if k["name"].startswith("act_seq_kernel")}
    want = {"act_seq_kernel<%s, %d, %s>" % (l, g, d) for l in ("true", "false") for g in (4, 2, 1) for d in ("true", "false")}
    assert set(seq) == want, sorted(seq)
    for k in seq.values():
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    for l in ("true", "false"):
        for g in (4, 2, 1):
            host, dev = seq["act_seq_kernel<%s, %d, false>" % (l, g)], seq["act_seq_kernel<%s, %d, true>" % (l, g)]
            assert dev["sgpr_spill"] <= host["sgpr_spill"] and dev["lds"] == host["lds"], (host, dev)
    stack = [k for k in res.get("actdev.hip", []) if k["name"] == "act_stack_dev_kernel"]
    assert len(stack) == 1
    assert stack[0]["scratch"] == 0 and stack[0]["vgpr_spill"] == 0 and stack[0]["sgpr_spill"] == 0, stack[0]


def test_timing_profile_and_design_bullet_agree():
    """every median of profiles/act_seq_dev_timing.json stands, to a tenth of a microsecond, in DESIGN.md's bullet -- which says so in
    the words "NOT faster" wherever the device route does not complete below the host call"""
    prof = json.load(open(os.path.join(ROOT, "profiles", "act_seq_dev_timing.json")))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    at = design.index("**Recurrent acting from device memory**")
    assert at > design.index("**Acting and ingestion from device memory**")
    bullet = design[at:design.index("### 4.5", at)]
    assert "profiles/act_seq_dev_timing.json" in bullet and "tools/act_seq_dev_timing.py" in bullet
    assert prof["rounds"] >= 5 and prof["shape"] == "LSTM 2x32, dimS 4, 17-step windows"
    assert set(prof["forward_us"]) == {"64", "1024", "4096"}
    for n, d in prof["forward_us"].items():
        assert set(d) == {"host", "host_from_tensor", "dev_enqueue", "dev_complete", "select_complete"}
        for k, v in d.items():
            assert v["min"] <= v["median"] <= v["max"]
            assert "%.1f" % v["median"] in bullet, (n, k)
        if d["dev_complete"]["median"] >= d["host"]["median"]:
            assert "NOT faster" in bullet, n
    for n, d in prof["kernel_us"].items():      # the device time of a call's launches
        for k in ("act_seq", "act_seq_dev"):
            assert "%.1f" % d[k]["median"] in bullet, (n, k)
