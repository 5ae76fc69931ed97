"""Bits of the replayed step for a list of fused-kernel shapes: N replayed steps from a fixed seed, then one line per shape with a
hash of the weights, both Adam moments, beta and the generator state.  Two builds of the library compute the same thing when
their outputs are equal line for line:

    python tools/step_bits.py [--lib PATH/libsmarties_hip.so] [--steps N] > a.txt     (diff a.txt b.txt)
"""
import argparse, hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
from smarties_amd import capi
from oracle_api import fill_synth, synth_cfg

ap = argparse.ArgumentParser()
ap.add_argument("--lib", help="library to load instead of smarties_amd/libsmarties_hip.so")
ap.add_argument("--steps", type=int, default=300)
args = ap.parse_args()
if args.lib:
    capi.HIP_LIB = os.path.abspath(args.lib)
api = capi.load_hip()

SHORT = dict(lenMin=2, lenMax=6, pTerm=0.0)
SHAPES = [      # the five of tests/test_hip_fused_chain.py, the bench shape, then the k-step counts 1, 1, 2, 5, 8 at two widths
    dict(dimS=3, dimA=1, hidden=(64, 64), batchSize=20),
    dict(dimS=32, dimA=7, hidden=(64, 64), batchSize=40),
    dict(dimS=17, dimA=2, bounded=[1, 0], hidden=(128, 128), batchSize=40),
    dict(dimS=17, dimA=6, hidden=(256, 256), batchSize=48),
    dict(dimS=5, dimA=2, hidden=(32, 32), batchSize=20),
    dict(dimS=17, dimA=6, hidden=(256, 256), batchSize=256),
] + [dict(dimS=s, dimA=2, hidden=(h, h), batchSize=40) for h in (64, 128) for s in (1, 4, 5, 20, 29)]

for kw in SHAPES:
    sc = synth_cfg(seed=83, dimS=kw["dimS"], dimA=kw["dimA"], **SHORT)
    L = capi.Learner(api, capi.make_config(randSeed=5, maxTotObsNum=4000, **kw))
    L.init_weights(); fill_synth(L, sc, 400); L.initialize()
    L.step(args.steps); L.sync()
    w, m1, m2 = L.get_params(); s = L.scalars()
    assert np.isfinite(w).all() and s.nGradSteps == args.steps
    h = hashlib.sha1()
    for a in (w, m1, m2, np.float64(s.beta), np.asarray(L.get_rng_state())):
        h.update(np.ascontiguousarray(a).tobytes())
    print("dS %2d dA %d H %3d B %3d  steps %d  %s  beta %.17g" % (kw["dimS"], kw["dimA"], kw["hidden"][0], kw["batchSize"], args.steps, h.hexdigest(), s.beta), flush=True)
    L.close()
