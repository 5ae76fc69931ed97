"""hl_create_dpg (include/smarties_hip_dpg.h), the part that needs no GPU: the exported symbols, the statuses answered in front of the
device query, and the arithmetic's own margin -- the restatement of tests/test_hip_dpg.py with fp32 networks stays within a third of
the GPU test's bound of its fp64 run at the same shapes, so that bound is one the fp32 kernels can meet."""
import os
import subprocess
import sys

import numpy as np
import pytest

from blocks import TOL32
from test_hip_dpg import SHAPES, blocks_of, dev, dpg_step, episodes, random_nets, rows_of      # (the restatement lives beside the GPU test)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (config changes, status without a device: 2 = HL_ERR_NO_DEVICE (admitted), 8 = HL_ERR_UNSUPPORTED)
CASES = {
    "dense": (dict(), 2), "cap": (dict(dimA=16), 2), "deep": (dict(hidden=(128,) * 8), 2),
    "retrace": (dict(returnsEstimator="retrace"), 8), "recurrent": (dict(nn_type=1), 8), "encoder_rnn": (dict(encoder=(16,), encoder_rnn=1), 8),
    "encoder": (dict(encoder=(16,)), 8), "appended": (dict(nAppendedObs=1), 8), "ranks": (dict(n_ranks=2), 8), "cap+1": (dict(dimA=17), 8),
    "conv": (dict(dimS=64, conv=[(8, 8, 1, 4, 3, 1)]), 8), "dimS": (dict(dimS=513), 8), "batch": (dict(batchSize=1040), 8),
    "width": (dict(hidden=(528,)), 8), "lds": (dict(hidden=(512, 512, 512)), 8),
}
SYMBOLS = ("create_dpg", "dpg_critic_num_params", "dpg_get_critic", "dpg_set_critic", "dpg_get_target", "dpg_set_target", "dpg_readback")

_CODE = """
import sys; sys.path.insert(0, %r)
import ctypes as C
from smarties_amd import capi
api = capi.load_hip()
print("SYMBOL|%%d" %% all(api.has(s) for s in %r))
for name, (kw, _) in %r.items():
    kw = dict(dict(dimS=6, dimA=3, hidden=(32,), batchSize=8, maxTotObsNum=2000, returnsEstimator="none"), **kw)
    cfg = capi.make_config(bounded=[0] * kw["dimA"], **kw)
    dpg = capi.DpgConfig(C.sizeof(capi.DpgConfig), 0, 0.01)
    h = C.c_void_p()
    rc = api.fn("create_dpg")(C.byref(cfg), C.byref(dpg), C.byref(h))
    print("CASE|%%s|%%d|%%s" %% (name, rc, "handle" if h else ""))
"""


@pytest.fixture(scope="module")
def child():
    import __graft_entry__ as ge
    ge.build_hip()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", _CODE % (ROOT, SYMBOLS, CASES)], capture_output=True, text=True, env=env)
    return out.stdout.splitlines(), out.stdout + out.stderr


@pytest.mark.parametrize("name", sorted(CASES))
def test_status_without_a_device_and_no_handle_left(child, name):
    assert "SYMBOL|1" in child[0], child[1]
    got = [l.split("|") for l in child[0] if l.startswith("CASE|%s|" % name)]
    assert got == [["CASE", name, str(CASES[name][1]), ""]], (got, child[1])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_fp32_networks_stay_within_a_third_of_the_bound(name):
    shape = SHAPES[name]; dS, dA, hidden, B, _ = shape
    eps, samples = episodes(dS, dA, B)
    rows = rows_of(eps, samples, np.zeros(dS, np.float32), np.ones(dS, np.float32), (0.0, 1.0))
    nets = random_nets(shape)
    r64, r32 = (dpg_step(nets, shape, rows, 0.8, 4.0, 0.25, dt) for dt in (np.float64, np.float32))
    assert r64["far"] == r32["far"] and any(r64["far"]) and not all(r64["far"])
    cols = lambda k: max(dev(r32[k][:, c], r64[k][:, c]) for c in range(r64[k].shape[1]))
    blk = lambda k, lay: max(dev(r32[k][i:i + n], r64[k][i:i + n]) for i, n in blocks_of(r64[lay]))
    worst = {"qT": dev(r32["qT"], r64["qT"]), "qN": dev(r32["qN"], r64["qN"]), "q": dev(r32["q"], r64["q"]), "dQda": cols("dQda"), "pvec": cols("pvec"),
             "Ga": cols("Ga"), "Gc": dev(r32["Gc"], r64["Gc"]), "ga": blk("ga", "la"), "gc": blk("gc", "lc"),
             "wb": max(dev([w[i] for w in r32["wb"]], [w[i] for w in r64["wb"]]) for i in range(5))}
    assert all(v <= TOL32 / 3 for v in worst.values()), worst
