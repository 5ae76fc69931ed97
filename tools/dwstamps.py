"""When does the last workgroup of each kind of the weight-gradient launch (dw_table_kernel, gemm16.hip) finish?  The bench
configuration, library built with HL_EXTRA_FLAGS=-DHL_DWSTAMPS (python tools/dwstamps.py [--lib PATH] [batch])."""
import os, sys, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import bench, numpy as np
from smarties_amd import capi
argv = sys.argv[1:]
if argv and argv[0] == "--lib":
    capi.HIP_LIB = os.path.abspath(argv[1]); argv = argv[2:]
api = capi.load_hip()
g = api.lib.hl_debug_stamps; g.restype = C.c_int; g.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
CFG = dict(bench.CFG)
if argv: CFG['batchSize'] = int(argv[0])
L = capi.Learner(api, capi.make_config(**CFG)); L.init_weights()
for e in range(5000): L.append_episode(**bench.synthetic_episode(np, e))
L.initialize()
acc = []
for it in range(40):
    L.step(8)
    out = (C.c_longlong * 32)(); assert g(L.h, out) == 0
    acc.append(np.array(list(out), dtype=np.int64))
a = np.array(acc[5:])
assert (a[:, 28] != 0).all(), "no stamps: the library was not built with -DHL_DWSTAMPS"
# maxima over the call's launches but the last (which carries a longer bookkeeping rider and is not stamped) and the entry stamp of
# the last launch stamped: the differences belong to that launch, a step inside a call
for nm, i in (("weight-gradient tiles", 24), ("bookkeeping rider", 25), ("sampler rider (search, gather)", 26), ("gather helpers", 27)):
    d = (a[:, i] - a[:, 28]) * 10
    print("last workgroup of %-32s ends %6.0f ns after the first tile workgroup's entry (min %d, max %d)" % (nm, np.median(d), d.min(), d.max()))
