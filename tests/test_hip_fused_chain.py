"""Chained first and second layer of the fused forward / head / dX kernel (fused.hip, 512 threads, widths of 64 and more): the
wavefronts that contract x2 = h1 W1 compute the h1 tiles of their own K range with the operands of the first product exchanged,
so that its accumulators are the A operand of the second -- no h1 panel in LDS, no barrier between the two products.  Smallest
shapes at which each tile count per wavefront runs, and the width that keeps the panel form, against the CPU oracle; all on
short truncated episodes, so that next-state rows occur."""
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

SHORT = dict(lenMin=2, lenMax=6, pTerm=0.0)

SHAPES = [
    dict(dimS=3, dimA=1, hidden=(64, 64), batchSize=20),                        # one tile per wavefront, one k-step, a partial panel
    dict(dimS=32, dimA=7, hidden=(64, 64), batchSize=40),                       # eight k-steps, every output column in use
    dict(dimS=17, dimA=2, bounded=[1, 0], hidden=(128, 128), batchSize=40),     # two tiles per wavefront, padded dSp
    dict(dimS=17, dimA=6, hidden=(256, 256), batchSize=48),                     # the bench width, three panels
    dict(dimS=5, dimA=2, hidden=(32, 32), batchSize=20),                        # the width that keeps the panel form
]
IDS = ["64x64-dS3-b20", "64x64-dS32-dA7-b40", "128x128-b40", "256x256-b48", "32x32-b20"]


def _follows_oracle(hip_api, cfg_kw, seed):
    cfg_kw = dict(cfg_kw, maxTotObsNum=2000, randSeed=7)
    G, O = _pair(hip_api, cfg_kw, synth_cfg(seed=seed, dimS=cfg_kw["dimS"], dimA=cfg_kw["dimA"], **SHORT), 150)
    for _ in range(2):
        G.step(1); O.step(1)
        _compare_step(G, O)
    G.step(8); O.step(8)
    assert np.array_equal(G.readback(capi.TAP_FLAT), O.readback(capi.TAP_FLAT))
    err = relinf(G.get_params()[0], O.get_params()[0])
    print("weights after 10 steps: relinf %.3g (bound %.3g)" % (err, 2 * TOL32))
    assert err < 2 * TOL32


@pytest.mark.parametrize("cfg_kw", SHAPES, ids=IDS)
def test_shapes_match_oracle(hip_api, cfg_kw):
    _follows_oracle(hip_api, cfg_kw, 81)


@pytest.mark.parametrize("func", ["Tanh", "Relu"])      # Tanh: its own instantiation; Relu: the generic one (run-time dispatch)
def test_other_activations_at_64(hip_api, func):
    _follows_oracle(hip_api, dict(dimS=32, dimA=7, hidden=(64, 64), batchSize=40, nnFunc=func), 82)


CFG128 = dict(dimS=17, dimA=2, bounded=[1, 0], hidden=(128, 128), batchSize=40, maxTotObsNum=2000)


def test_same_seed_same_bits(hip_api):
    """Two learners, same seed, 300 replayed steps at 128 x 128: weights, both Adam moments, beta and the generator state."""
    sc = synth_cfg(seed=83, dimS=17, dimA=2, **SHORT)
    out = []
    for _ in range(2):
        L = hip_learner(hip_api, capi.make_config(randSeed=5, **CFG128))
        L.init_weights(); fill_synth(L, sc, 150); L.initialize()
        L.step(300)
        w, m1, m2 = L.get_params(); s = L.scalars()
        assert np.isfinite(w).all() and s.nGradSteps == 300
        out.append((w, m1, m2, s.beta, L.get_rng_state()))
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


def test_both_exchange_modes_give_the_same_bits():
    """SMARTIES_HIP_PANEL_SAFE=0 and =1 at 128 x 128, fresh processes (the mode is fixed at hl_create): bit-identical parameters."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = (
        "import sys, hashlib, ctypes as C; sys.path[:0] = [%r, %r]\n"
        "from smarties_amd import capi, load_hip; from oracle_api import synth_cfg, fill_synth\n"
        "api = load_hip(); sc = synth_cfg(seed=84, dimS=17, dimA=2, lenMin=2, lenMax=6, pTerm=0.0)\n"
        "L = capi.Learner(api, capi.make_config(**%r))\n"
        "L.init_weights(); fill_synth(L, sc, 150); L.initialize(); L.step(1); L.step(11); L.sync()\n"
        "m = api.lib.hl_debug_panel_mode; m.restype = C.c_int; m.argtypes = [C.c_void_p]\n"
        "print('MODE', m(L.h), 'HASH', hashlib.sha1(b''.join(a.tobytes() for a in L.get_params())).hexdigest(), L.scalars().beta)\n"
    ) % (os.path.dirname(here), here, CFG128)
    outs = []
    for safe in ("0", "1"):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SMARTIES_HIP_PANEL_SAFE=safe), capture_output=True, text=True, timeout=120)
        line = [l for l in out.stdout.splitlines() if l.startswith("MODE")]
        assert line, out.stdout + out.stderr[-2000:]
        outs.append(line[-1].split())
    assert outs[0][1] == "0" and outs[1][1] == "1"
    assert outs[0][3:] == outs[1][3:], outs
