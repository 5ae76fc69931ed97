"""hl_create_dqn (include/smarties_hip_dqn.h), the part that needs no GPU: the inputs of tests/test_hip_dqn.py are fair -- its restatement
with the network in fp32 stays within a third of the bound of the fp64 one at every shape --, the exported symbols, and the refusals
answered in front of the device query."""
import os
import subprocess
import sys

import numpy as np
import pytest

from blocks import TOL32
import test_hip_dqn as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("values,hidden,est,delay,B", T.CASES)
def test_fp32_network_within_a_third_of_the_bound(values, hidden, est, delay, B):
    nOpt = int(np.prod(values)); rng = np.random.RandomState(5); lay, nP = T.layout(T.DS, hidden, nOpt)
    blobs = []
    for _ in range(2):      # weights as hl_init_weights scales them: hidden +-sqrt(6 / (in + out)), residuals 1 / 0, output a tenth of that
        W = np.zeros(nP, np.float32); prev = T.DS; l = 1
        for j, h in enumerate(hidden + (nOpt,)):
            n = -(-h // 8) * 8 * prev; s = np.sqrt(6.0 / (prev + h)) * (0.1 if j == len(hidden) else 1)
            W[lay["indW"][l]:lay["indW"][l] + n] = rng.uniform(-s, s, n); l += 1
            if 0 < j < len(hidden):
                W[lay["indW"][l]:lay["indW"][l] + h] = 1; l += 1
            prev = h
        blobs.append(W)
    eps = T.replay(values, B); N, samples = T.episodes(B)
    X, X1 = [np.stack([eps[e]["S"][t + d] for e, t in samples]) for d in (0, 1)]
    lab = [T.label(eps[e]["A"][t], values) for e, t in samples]; MU = np.stack([eps[e]["MU"][t] for e, t in samples])
    tgt = dict(ret=np.array([eps[e]["R"][t] for e, t in samples])) if est != "none" else dict(
        r=np.array([eps[e]["R"][t] for e, t in samples]), term=[t + 2 == N and eps[e]["term"] for e, t in samples])
    args = (blobs[0], blobs[1] if delay > 0 else None, lay, nP, hidden, nOpt, X, X1, lab, MU, tgt, 0.999, 5.0, 0.25)
    ref, ref32 = T.restate(*args), T.restate(*args, dt=np.float32)
    assert ref["nfar"] == 1 and T.worst(ref32, ref, lay, hidden, nOpt) <= TOL32 / 3


# name -> (config changes, options per variable, status without a device: 2 = HL_ERR_NO_DEVICE (admitted), 8 = HL_ERR_UNSUPPORTED)
REFUSALS = {"dense": (dict(), (3, 6), 2), "cap": (dict(), (512,), 2), "cap+1": (dict(), (513,), 8), "recurrent": (dict(nn_type=1), (4,), 8),
            "ranks": (dict(n_ranks=2), (4,), 8), "conv": (dict(dimS=64, conv=[(8, 8, 1, 4, 3, 1)]), (4,), 8), "batch": (dict(batchSize=1040), (4,), 8)}

_CODE = """
import sys; sys.path.insert(0, %r)
import ctypes as C, numpy as np
from smarties_amd import capi
api = capi.load_hip()
print("SYMBOL|%%d" %% all(api.has(s) for s in ("create_dqn", "dqn_get_target", "dqn_set_target")))
for name, (kw, values, _) in %r.items():
    kw = dict(dict(dimS=6, hidden=(32,), batchSize=8, maxTotObsNum=2000), **kw)
    cfg = capi.make_config(dimA=len(values), adv_kind=capi.ADV_DISCRETE, n_options=int(np.prod(values)), **kw)
    dqn = capi.DqnConfig(C.sizeof(capi.DqnConfig), 0, 0.01); v = np.asarray(values, np.int32); h = C.c_void_p()
    rc = api.fn("create_dqn")(C.byref(cfg), C.byref(dqn), v.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(h))
    print("CASE|%%s|%%d|%%s" %% (name, rc, "handle" if h else ""))
"""


@pytest.fixture(scope="module")
def child():
    import __graft_entry__ as ge
    ge.build_hip()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", _CODE % (ROOT, REFUSALS)], capture_output=True, text=True, env=env)
    return out.stdout.splitlines(), out.stdout + out.stderr


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_status_without_a_device_and_no_handle_left(child, name):
    assert "SYMBOL|1" in child[0], child[1]
    got = [l.split("|") for l in child[0] if l.startswith("CASE|%s|" % name)]
    assert got == [["CASE", name, str(REFUSALS[name][2]), ""]], (got, child[1])
