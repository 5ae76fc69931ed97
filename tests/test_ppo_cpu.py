"""hl_create_ppo (include/smarties_hip_ppo.h), the part that needs no GPU: the exported symbols, the statuses answered in front of the
device query, the serial penalty / DKL_target chain on a hand-computed example, and the arithmetic's own margin -- the restatement of
tests/test_hip_ppo.py with fp32 networks stays within a third of the GPU test's bound of its fp64 run."""
import os
import subprocess
import sys

import numpy as np
import pytest

from blocks import TOL32
from test_hip_dpg import dev
from test_hip_ppo import SHAPES, all_blocks, chain, conditions, episodes, ppo_step, random_nets      # (the restatement lives beside the GPU test)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (config changes, status without a device: 2 = HL_ERR_NO_DEVICE (admitted), 8 = HL_ERR_UNSUPPORTED)
CASES = {"dense": (dict(), 2), "cap": (dict(dimA=16), 2), "options": (dict(values=(8, 64)), 2), "recurrent": (dict(nn_type=1), 8),
         "encoder": (dict(encoder=(16,)), 8), "appended": (dict(nAppendedObs=1), 8), "ranks": (dict(n_ranks=2), 8), "cap+1": (dict(dimA=17), 8),
         "conv": (dict(dimS=64, conv=[(8, 8, 1, 4, 3, 1)]), 8), "dimS": (dict(dimS=513), 8), "batch": (dict(batchSize=1040), 8),
         "clip": (dict(clipImpWeight=1.0), 8), "epochs": (dict(nEpochs=0), 8), "options+1": (dict(values=(9, 57)), 8)}
SYMBOLS = ("create_ppo", "ppo_values", "ppo_critic_num_params", "ppo_get_critic", "ppo_set_critic", "ppo_get_state", "ppo_set_state", "ppo_readback")

_CODE = """
import sys; sys.path.insert(0, %r)
import ctypes as C
import numpy as np
from smarties_amd import capi
api = capi.load_hip()
print("SYMBOL|%%d" %% all(api.has(s) for s in %r))
for name, (kw, _) in %r.items():
    kw = dict(dict(dimS=6, dimA=3, hidden=(32,), batchSize=8, maxTotObsNum=64, clipImpWeight=0.2, returnsEstimator="GAE", nEpochs=1, values=None), **kw)
    nE, values = kw.pop("nEpochs"), kw.pop("values")
    ppo = capi.PpoConfig(C.sizeof(capi.PpoConfig), nE, 0.01, 0)
    if values:
        kw.update(dimA=len(values), adv_kind=capi.ADV_DISCRETE, n_options=int(np.prod(values))); ppo.n_vars = len(values)
        for i, v in enumerate(values): ppo.values[i] = v
    cfg = capi.make_config(bounded=[0] * kw["dimA"], **kw)
    h = C.c_void_p()
    rc = api.fn("create_ppo")(C.byref(cfg), C.byref(ppo), C.byref(h))
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


def test_the_serial_chain_on_five_rows():
    """penalCoef 0.7, DKL_target 0.01; rows (DKL, RHO, isOff) in ascending order, worked by hand:
    1. DKL 0.001 < 0.01 / 1.5: delta = -0.35; near, target 0.01 < RHO 1.0: target = 0.01 x 1.0001
    2. DKL 0.02 > 1.5 x 0.010001: delta = -0.35 + 0.7 = 0.35; far, target < RHO 1.5: unchanged
    3. DKL 0.01 between: delta unchanged; far, RHO 0.005 < target: target x 0.9995
    4. DKL 0.5 above: delta = 1.05; near (RHO 0.9 > target): target x 1.0001
    5. DKL 0.0 below: delta = 0.7; near: target x 1.0001
    penalCoef = 0.7 + 1e-4 x 0.7 / 5"""
    pen, tgt = chain(((0.001, 1.0, False), (0.02, 1.5, True), (0.01, 0.005, True), (0.5, 0.9, False), (0.0, 1.0, False)), 0.7, 0.01)
    assert abs(pen - (0.7 + 1e-4 * 0.7 / 5)) < 1e-15 and abs(tgt - 0.01 * 1.0001 * 0.9995 * 1.0001 * 1.0001) < 1e-17
    assert chain(((1.0, 1.0, False),) * 3, 1e-9, 0.5)[0] == float(np.finfo(np.float32).eps)      # the floor at nnEPS


@pytest.mark.parametrize("name", ["c16", "d80"])
def test_fp32_networks_stay_within_a_third_of_the_bound(name):
    shape = SHAPES[name]; nets = random_nets(shape); eps = episodes(shape, nets[0]); rng = np.random.RandomState(2)
    rows = [dict(s=e["S"][t], a=e["A"][t], mu=e["MU"][t], ret=float(np.sign(e["R"][t + 1]) * (0.5 + rng.rand())), vold=float(e["V"][t])) for e in eps for t in range(4)]
    r64, r32 = (ppo_step(nets, shape, rows, 0.7, 0.005, 3.16e-4, dt) for dt in (np.float64, np.float32))
    conditions(r64, 0.005)
    assert r64["off"] == r32["off"] and r64["zero"] == r32["zero"]
    cols = lambda k: max(dev(r32[k][:, c], r64[k][:, c]) for c in range(r64[k].shape[1]))
    blk = lambda k, lay: max(dev(r32[k][i:i + n], r64[k][i:i + n]) for i, n in all_blocks(r64[lay]))
    worst = {"P": cols("P"), "V": dev(r32["V"], r64["V"]), "rho": dev(r32["rho"], r64["rho"]), "dkl": dev(r32["dkl"], r64["dkl"]), "gain": dev(r32["gain"], r64["gain"]),
             "G": cols("G"), "Gc": dev(r32["Gc"], r64["Gc"]), "ga": blk("ga", "la"), "gc": blk("gc", "lc"), "pen": dev([r32["pen"]], [r64["pen"]]), "tgt": dev([r32["tgt"]], [r64["tgt"]]),
             "wb": max(dev([w[i] for w in r32["wb"]], [w[i] for w in r64["wb"]]) for i in range(4))}
    assert all(v <= TOL32 / 3 for v in worst.values()), worst
