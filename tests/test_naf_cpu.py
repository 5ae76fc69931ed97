"""hl_create_naf (include/smarties_hip_naf.h), the part that needs no GPU: the exported symbols, the refusals answered in front of the
device query, and hl_create itself left as it was."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (config changes, status without a device: 2 = HL_ERR_NO_DEVICE (admitted), 8 = HL_ERR_UNSUPPORTED)
CASES = {
    "dense": (dict(), 2), "cap": (dict(dimA=17), 2),
    "recurrent": (dict(nn_type=1), 8), "ranks": (dict(n_ranks=2), 8), "cap+1": (dict(dimA=18), 8),
    "conv": (dict(dimS=64, conv=[(8, 8, 1, 4, 3, 1)]), 8),
}

_CODE = """
import sys; sys.path.insert(0, %r)
import ctypes as C
from smarties_amd import capi
api = capi.load_hip()
print("SYMBOL|%%d" %% all(api.has(s) for s in ("create_naf", "naf_get_target", "naf_set_target")))
for name, (kw, _) in %r.items():
    kw = dict(dict(dimS=6, dimA=3, hidden=(32,), batchSize=8, maxTotObsNum=2000), **kw)
    cfg = capi.make_config(bounded=[0] * kw["dimA"], **kw)
    naf = capi.NafConfig(C.sizeof(capi.NafConfig), 0, 0.01)
    h = C.c_void_p()
    rc = api.fn("create_naf")(C.byref(cfg), C.byref(naf), C.byref(h))
    print("CASE|%%s|%%d|%%s" %% (name, rc, "handle" if h else ""))
cfg = capi.make_config(dimS=6, dimA=3, bounded=[0] * 3, hidden=(32,), batchSize=8, maxTotObsNum=2000)
h = C.c_void_p()
print("CREATE|%%d" %% api.fn("create")(C.byref(cfg), C.byref(h)))
"""


@pytest.fixture(scope="module")
def child():
    import __graft_entry__ as ge
    ge.build_hip()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", _CODE % (ROOT, CASES)], capture_output=True, text=True, env=env)
    return out.stdout.splitlines(), out.stdout + out.stderr


@pytest.mark.parametrize("name", sorted(CASES))
def test_status_without_a_device_and_no_handle_left(child, name):
    assert "SYMBOL|1" in child[0] and "CREATE|2" in child[0], child[1]      # the symbols are exported; hl_create answers as before
    got = [l.split("|") for l in child[0] if l.startswith("CASE|%s|" % name)]
    assert got == [["CASE", name, str(CASES[name][1]), ""]], (got, child[1])
