"""hl_create_discrete (include/smarties_hip_discrete.h), the part that needs no GPU: the exported symbol, what it admits and refuses in
front of the device query, hl_create's own refusals left as they were, and the new head's resources."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (adv_kind is discrete, dimA, n_options, values handed over, status without a device)
CASES = {
    "3x4": (1, 2, 12, (3, 4), 2), "2x2x2x2x4": (1, 5, 64, (2, 2, 2, 2, 4), 2), "9x9": (1, 2, 81, (9, 9), 2), "130": (1, 1, 130, (130,), 2),
    "8x8x8": (1, 3, 512, (8, 8, 8), 2),                                   # admitted: HL_ERR_NO_DEVICE
    "513": (1, 1, 513, (513,), 8), "23x23": (1, 2, 529, (23, 23), 8),    # a size: HL_ERR_UNSUPPORTED
    "product-differs": (1, 2, 13, (3, 4), 1), "variable-of-one": (1, 2, 4, (4, 1), 1), "n_vars-not-dimA": (1, 3, 12, (3, 4), 1),
    "not-discrete": (0, 2, 12, (3, 4), 1),                               # HL_ERR_BAD_ARG
    "hl_create-two-variables": (1, 2, 12, None, 1), "hl_create-65": (1, 1, 65, None, 1),      # hl_create itself: as before
}

_CODE = """
import sys; sys.path.insert(0, %r)
import ctypes as C
import numpy as np
from smarties_amd import capi
api = capi.load_hip()
print("SYMBOL|%%d" %% api.has("create_discrete"))
for name, (disc, dimA, nopt, values, _) in %r.items():
    cfg = capi.make_config(dimS=6, dimA=dimA, bounded=[0] * dimA, hidden=(32,), batchSize=8, maxTotObsNum=2000,
                           adv_kind=capi.ADV_DISCRETE if disc else capi.ADV_ZERO, n_options=nopt)
    h = C.c_void_p()
    if values is None:
        rc = api.fn("create")(C.byref(cfg), C.byref(h))
    else:
        v = np.asarray(values, np.int32)
        rc = api.fn("create_discrete")(C.byref(cfg), len(v), v.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(h))
    print("CASE|%%s|%%d|%%s" %% (name, rc, "handle" if h else ""))
"""


@pytest.fixture(scope="module")
def child():
    """One child process without a device for all cases."""
    import __graft_entry__ as ge
    ge.build_hip()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", _CODE % (ROOT, CASES)], capture_output=True, text=True, env=env)
    return out.stdout.splitlines(), out.stdout + out.stderr


@pytest.mark.parametrize("name", sorted(CASES))
def test_status_without_a_device_and_no_handle_left(child, name):
    assert "SYMBOL|1" in child[0], child[1]      # hl_create_discrete is exported
    got = [l.split("|") for l in child[0] if l.startswith("CASE|%s|" % name)]
    assert got == [["CASE", name, str(CASES[name][4]), ""]], (got, child[1])



def test_wide_head_kernels_spill_no_vector_register_and_hold_no_scratch_instruction():
    """The compiler's remarks kept beside the objects and the ISA (tools/resource_usage.py).  A frame slot the compiler reserves and never
    touches -- tests/test_kernel_resources.py: DEAD_SLOT -- is told from a spill by the ISA"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    ks = [k for k in resource_usage.kernels()["headw.hip"] if k["name"].startswith("head_wide_kernel<")]
    isa = resource_usage.scratch_instructions("headw.hip")
    assert len(ks) == 3 and all(k["vgpr_spill"] == 0 and k["scratch"] <= 64 and isa[k["name"]] == 0 for k in ks), (ks, isa)
