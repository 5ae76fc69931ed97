"""The rollout buffer (include/smarties_hip_rollout.h), the part that needs no GPU: the header and the exported symbols, the refusals in
front of the device, the noise mapping's restatement against the generator's published known answers, and the new kernels' resources."""
import ctypes as C
import os
import re
import sys

import numpy as np

import rollout as R
from smarties_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("hl_rollout_create", "hl_rollout_destroy", "hl_rollout_step", "hl_rollout_info", "hl_rollout_read", "hl_rollout_noise")


def _api():
    import __graft_entry__ as ge
    ge.build_hip()
    return capi.load_hip()


def test_rollout_header_declares_the_calls_and_the_main_header_none():
    txt = open(os.path.join(ROOT, "include", "smarties_hip_rollout.h")).read()
    main = open(os.path.join(ROOT, "include", "smarties_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"HL_API\s+int\s+%s\s*\(" % name, txt), name
        assert name not in main, name      # (tests/test_cabi_symbols.py wants an oracle twin of everything declared there)
    fields = re.search(r"typedef struct hl_rollout_counts \{(.*?)\}", txt, re.S).group(1)
    assert re.findall(r"int64_t\s+(\w+);", fields) == [k for k, _ in capi.RolloutCounts._fields_]
    assert re.search(r"enum\s*\{\s*HL_ROLLOUT_EVALUATE\s*=\s*1\s*,\s*HL_ROLLOUT_NO_STORE\s*=\s*2\s*\}", txt)
    assert (capi.ROLLOUT_EVALUATE, capi.ROLLOUT_NO_STORE) == (1, 2)
    assert "rollout.hip" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_library_exports_the_six_symbols_and_refuses_bad_arguments_without_a_device():
    api = _api()
    for name in ENTRY_POINTS:
        assert api.has(name[3:]), name
    h, null = C.c_void_p(), C.c_void_p()
    fake = C.c_void_p(8)      # never dereferenced: the sizes are refused first
    assert api.fn("rollout_create")(null, 4, 8, 0, 0, C.byref(h)) == 1      # HL_ERR_BAD_ARG: a null handle
    for n_env, max_steps in ((0, 8), (-3, 8), (capi.ROLLOUT_MAX_ENV + 1, 8), (4, 1), (4, 0)):
        assert api.fn("rollout_create")(fake, n_env, max_steps, 0, 0, C.byref(h)) == 1, (n_env, max_steps)
    assert api.fn("rollout_create")(fake, 4, 8, 0, 0, None) == 1
    assert not h
    assert api.fn("rollout_step")(null, null, null, null, null, 0, null, null) == 1
    assert api.fn("rollout_info")(null, C.byref(capi.RolloutCounts())) == 1
    assert api.fn("rollout_read")(null, 0, None, None, None, None, None, None, None) == 1
    assert api.fn("rollout_destroy")(null) == 0
    out = C.c_double()
    assert api.fn("rollout_noise")(1, 0, 0, 0, 0, 0, None) == 1
    assert api.fn("rollout_noise")(1, -1, 0, 0, 0, 0, C.byref(out)) == 1


def test_philox_core_reproduces_the_published_known_answers():
    """Random123's kat_vectors for philox4x32-10: the all-zero and the all-ones counter and key; the array form and the plain-integer
    form, written apart, give the same words (the round constants decide)"""
    f = 0xFFFFFFFF
    assert R.philox_int((0, 0, 0, 0), (0, 0)) == R.KAT_ZERO
    assert R.philox_int((f, f, f, f), (f, f)) == R.KAT_ONES
    assert tuple(int(x) for x in R.philox_np(0, 0, 0, 0, 0, 0)) == R.KAT_ZERO
    assert tuple(int(x) for x in R.philox_np(f, f, f, f, f, f)) == R.KAT_ONES
    rng = np.random.default_rng(4)
    for _ in range(50):
        c = [int(x) for x in rng.integers(0, 2**32, 4)]
        k = [int(x) for x in rng.integers(0, 2**32, 2)]
        assert tuple(int(x) for x in R.philox_np(*c, *k)) == R.philox_int(c, k)


def test_restated_noise_is_clipped_and_replaces_the_normal_tail():
    """10^5 draws: all within +-3; the share of replaced draws is the normal's mass beyond 3 sigma, 0.27 %"""
    i = np.arange(100000)
    rep = []
    z = R.noise_np(20240229, i % 1000, i // 1000, 3, 1, replaced=rep)
    assert z.shape == (100000,) and np.all(np.abs(z) <= 3.0)
    share = rep[0].mean()
    assert 0.002 <= share <= 0.0035, share
    assert abs(z.mean()) < 0.02 and 0.97 < z.std() < 1.0      # (the clipped normal's deviation is 0.9866)
    u = R.noise_np(20240229, i % 1000, i // 1000, 3, 0, discrete=True)
    assert np.all((u >= 0) & (u < 1)) and abs(u.mean() - 0.5) < 0.01


def test_host_evaluation_of_the_library_equals_the_restatement():
    """hl_rollout_noise runs the text the device compiles: the uniforms equal the restatement's exactly, the normal deviates to the last
    places of the host's log, cos and sqrt; draws that fall beyond +-3 among them"""
    api = _api()
    seed = 0x0123456789ABCDEF
    env, ep, t, comp = np.meshgrid([0, 3, 39, 65535], [0, 1, 7, 2**31], [0, 5, 1000], [0, 1, 2, 63], indexing="ij")
    rep = []
    want = R.noise_np(seed, env, ep, t, comp, replaced=rep).ravel()
    want_u = R.noise_np(seed, env, ep, t, comp, discrete=True).ravel()
    got = np.array([capi.rollout_noise(api, seed, *q) for q in zip(env.ravel(), ep.ravel(), t.ravel(), comp.ravel())])
    got_u = np.array([capi.rollout_noise(api, seed, *q, discrete=True) for q in zip(env.ravel(), ep.ravel(), t.ravel(), comp.ravel())])
    assert np.array_equal(got_u, want_u)
    assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()
    # a replaced draw: searched in the restatement, asked of the library
    i = np.arange(4000)
    rep = []
    z = R.noise_np(seed, i, 0, 0, 0, replaced=rep)
    hit = np.flatnonzero(rep[0])
    assert hit.size > 0
    for e in hit[:3]:
        assert abs(capi.rollout_noise(api, seed, int(e), 0, 0, 0) - z[e]) <= 1e-12


def test_timing_profile_and_design_bullet_agree():
    """every host and device median of profiles/rollout_timing.json stands in DESIGN.md's bullet to a tenth of a microsecond, and the
    bullet names every point at which the new call is slower than the hand-written loop (or says that there is none)"""
    import json
    prof = json.load(open(os.path.join(ROOT, "profiles", "rollout_timing.json")))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    at = design.index("**A rollout buffer for vectorised simulators: one call per simulator step**")
    bullet = design[at:design.index("### 4.5", at)]
    assert "profiles/rollout_timing.json" in bullet and "tools/rollout_timing.py" in bullet
    assert prof["calls"] == 200 and prof["warmup"] == 50 and set(prof["nets"]) == {"lstm-2x32", "dense-2x256"}
    slower = []
    for name, d in prof["nets"].items():
        assert set(d) == {"64", "1024", "4096"}, name
        for n, v in d.items():
            for col in ("rollout", "hand_loop"):
                for k in ("host_us", "device_us"):
                    assert "%.1f" % v[col][k] in bullet, (name, n, col, k)
            slower += ["%s n=%s %s" % (name, n, k) for k in ("host_us", "device_us") if v["rollout"][k] > v["hand_loop"][k]]
            assert v["no_room"] == 0 and v["launch_us_per_call"]["rollout_book_kernel"] > 0
    assert slower == prof["rollout_slower_than_hand_loop"]
    assert ("slower at none of the six points" in bullet) == (not slower)


def test_rollout_kernels_build_without_scratch():
    _api()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = {k["name"]: k for k in resource_usage.kernels().get("rollout.hip")}
    for want in ("rollout_book_kernel", "rollout_noise_kernel", "rollout_store_kernel"):
        assert any(want in name for name in rows), sorted(rows)
    for k in rows.values():
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
