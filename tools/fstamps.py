import os, sys, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import bench, numpy as np
from smarties_amd import capi, load_hip
api = load_hip()
g = api.lib.hl_debug_stamps; g.restype = C.c_int; g.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
CFG = dict(bench.CFG)
if len(sys.argv) > 1: CFG['batchSize'] = int(sys.argv[1])     # (with -DHL_FSTAMP_PANEL=p: a workgroup in the crowd)
L = capi.Learner(api, capi.make_config(**CFG)); L.init_weights()
for e in range(5000): L.append_episode(**bench.synthetic_episode(np, e))
L.initialize()
acc = []
for it in range(40):
    L.step(8)
    out = (C.c_longlong * 32)(); assert g(L.h, out) == 0
    acc.append(np.array(list(out), dtype=np.int64))
a = np.array(acc[5:])
d = np.diff(a[:, 0:14], axis=1) * 10   # ns
m = np.median(a, axis=0)
# slot 16 is written by the chained form only (fused.hip: the wavefront that chains tile 1); there slots 1..3 are thread 0's, which
# takes no part in the products: stamp 2 is where it reaches the x2 barrier (behind the fp64 head terms, where they sit there)
chained = m[16] != 0
names = ['loads+stage', 'h1', 'x2 mma+red', 'epi+st issue', 'precompute', 'waitcnt', 'barrier', 'partials issue', 'partials sum', 'head', 'dx2', 'dx mma+red', 'final store']
if chained: names[1], names[2] = 'wave 0 to barrier', 'wave 0 at barrier'
med = np.median(d, axis=0)
for nm, v in zip(names, med): print('%-16s %7.0f ns' % (nm, v))
print('total', med.sum())
if chained:
    print('chain detail (the wavefront of tile 1): staging barrier->h1 loop end %d ns, bias+activation+own tile %d ns, x2 MFMAs+partial stored %d ns, x2 barrier left %d ns later'
          % ((m[14] - m[1]) * 10, (m[15] - m[14]) * 10, (m[16] - m[15]) * 10, (m[3] - m[16]) * 10))
    if m[17] != 0: print('head terms under the panel barrier: %d ns (from the arrival, W1 row tile staged in between)' % ((m[17] - m[6]) * 10))
else:
    print('h1 detail: start->loop end %d ns, epilogue %d ns, sync+reads %d ns' % ((m[14]-m[1])*10, (m[15]-m[14])*10, (m[2]-m[15])*10))
# when the last workgroup of each kind finished, relative to the entry of the stamped workgroup (same launch)
e = a[:, 31]
for nm, i in (("stamped workgroup (panel 0, tile 1)", 13), ("last ordinary panel workgroup", 20), ("last next-state-row panel workgroup", 21), ("sampler rider (draws, sort)", 22), ("far-policy / beta rider", 23)):
    print("%-40s ends %6.0f ns after the entry stamp" % (nm, np.median(a[:, i] - e) * 10))
