"""Panel exchange of the fused forward / head / dX kernel (fused.hip): every workgroup of a panel sends its 16 x 8 share of the
output layer along with its y3 / f'(x2) tile, and the barrier takes its target from an early read of the (monotonic) arrive
counter.  Smallest shapes at which each path of that exchange runs, against the CPU oracle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_api import synth_cfg, fill_synth
from parity import relinf
from smarties_amd import capi
from test_hip_parity import _pair, _compare_step, hip_learner, TOL32

pytestmark = pytest.mark.gpu

# short episodes that all end truncated: the minibatch carries next-state rows (their O[0] is V(s'))
SHORT = dict(lenMin=2, lenMax=6, pTerm=0.0)


@pytest.mark.parametrize("cfg_kw", [
    dict(dimS=3, dimA=1, hidden=(16, 16), batchSize=5),                       # HT = 1: no peers, one partial panel
    dict(dimS=5, dimA=2, bounded=[1, 0], hidden=(32, 32), batchSize=20),      # HT = 2: a full panel plus a partial one with next-state rows
    dict(dimS=17, dimA=7, hidden=(64, 64), batchSize=40),                     # nDense = 8: every column of the partial tile in use
    dict(dimS=17, dimA=6, hidden=(256, 256), batchSize=48),                   # the bench width; three panels on three XCDs
], ids=["16x16-b5", "32x32-b20", "64x64-dA7-b40", "256x256-b48"])
def test_smallest_shapes_match_oracle(hip_api, cfg_kw):
    cfg_kw = dict(cfg_kw, maxTotObsNum=2000, randSeed=7)
    G, O = _pair(hip_api, cfg_kw, synth_cfg(seed=71, dimS=cfg_kw["dimS"], dimA=cfg_kw["dimA"], **SHORT), 150)
    for _ in range(2):
        G.step(1); O.step(1)
        _compare_step(G, O)
    G.step(8); O.step(8)
    assert np.array_equal(G.readback(capi.TAP_FLAT), O.readback(capi.TAP_FLAT))
    assert relinf(G.get_params()[0], O.get_params()[0]) < 2 * TOL32


def test_both_exchange_modes_give_the_same_bits():
    """Plain stores / loads through the XCD's L2 (mode 0) and agent-scope ones (mode 1, SMARTIES_HIP_PANEL_SAFE=1) carry the same
    numbers: parameters and beta after 12 steps are bit-identical.  Fresh processes: the mode is fixed at hl_create from the environment."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = (
        "import sys, hashlib, ctypes as C; sys.path[:0] = [%r, %r]\n"
        "from smarties_amd import capi, load_hip; from oracle_api import synth_cfg, fill_synth\n"
        "api = load_hip(); sc = synth_cfg(seed=72, dimS=17, dimA=7, lenMin=2, lenMax=6, pTerm=0.0)\n"
        "L = capi.Learner(api, capi.make_config(dimS=17, dimA=7, hidden=(64, 64), batchSize=40, maxTotObsNum=2000))\n"
        "L.init_weights(); fill_synth(L, sc, 150); L.initialize(); L.step(1); L.step(11); L.sync()\n"
        "m = api.lib.hl_debug_panel_mode; m.restype = C.c_int; m.argtypes = [C.c_void_p]\n"
        "print('MODE', m(L.h), 'HASH', hashlib.sha1(b''.join(a.tobytes() for a in L.get_params())).hexdigest(), L.scalars().beta)\n"
    ) % (os.path.dirname(here), here)
    outs = []
    for safe in ("0", "1"):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SMARTIES_HIP_PANEL_SAFE=safe), capture_output=True, text=True, timeout=120)
        line = [l for l in out.stdout.splitlines() if l.startswith("MODE")]
        assert line, out.stdout + out.stderr[-2000:]
        outs.append(line[-1].split())
    assert outs[0][1] == "0" and outs[1][1] == "1"
    assert outs[0][3:] == outs[1][3:], outs


def test_same_seed_same_bits(hip_api):
    """Two learners, same seed, 300 replayed steps: the partial outputs are summed in one fixed association whatever the order in
    which the workgroups of a panel arrive."""
    cfg_kw = dict(dimS=17, dimA=7, hidden=(64, 64), batchSize=40, maxTotObsNum=2000, randSeed=5)
    sc = synth_cfg(seed=73, dimS=17, dimA=7, **SHORT)
    out = []
    for _ in range(2):
        L = hip_learner(hip_api, capi.make_config(**cfg_kw))
        L.init_weights(); fill_synth(L, sc, 150); L.initialize()
        L.step(300)
        w, m1, m2 = L.get_params(); s = L.scalars()
        assert np.isfinite(w).all() and s.nGradSteps == 300
        out.append((w, m1, m2, s.beta, L.get_rng_state()))
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


def test_arrive_counters_wrap(hip_api):
    """The arrive counters are monotonic 32-bit numbers; the barrier's target is derived from a read of the counter before the
    workgroup's own arrival.  Started two launches below 2^32, the steps cross the wrap: they still follow the oracle and no
    wait times out (scalars() raises on the device's error flag)."""
    setc = hip_api.lib.hl_debug_set_panel_counters; setc.restype = C.c_int; setc.argtypes = [C.c_void_p, C.c_uint32]
    cfg_kw = dict(dimS=5, dimA=2, bounded=[1, 0], hidden=(32, 32), batchSize=20, maxTotObsNum=2000, randSeed=9)
    G, O = _pair(hip_api, cfg_kw, synth_cfg(seed=74, dimS=5, dimA=2, **SHORT), 150)
    HT = 2
    assert setc(G.h, 1) != 0                      # not a multiple of HT: no state the kernel can meet
    assert setc(G.h, 2 ** 32 - 2 * HT) == 0
    for _ in range(5):
        G.step(1); O.step(1)
        _compare_step(G, O)
        G.scalars()
