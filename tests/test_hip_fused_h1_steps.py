"""First-layer product of the fused forward / head / dX kernel (fused.hip) as straight-line code per k-step count: the count
dSp / 4 = 1..8 is a run-time value that selects one of eight bodies, each reading all its operands before its first MFMA.  Every
count runs against the CPU oracle in each form of the kernel: four chaining wavefronts (64 x 64), eight (128 x 128) and the panel
form (32 x 32); batches of 20 (a partial panel) and 40 (more than one panel); short truncated episodes, so that next-state rows
occur.  Then the weight-gradient launch's problem table (gemm16.hip) on one dense net that has every kind of problem in it."""
import numpy as np
import pytest

from oracle_api import synth_cfg
from parity import relinf
from smarties_amd import capi
from test_hip_parity import _pair, _compare_step, TOL32

pytestmark = pytest.mark.gpu

SHORT = dict(lenMin=2, lenMax=6, pTerm=0.0)

# (hidden width, state width): k-step counts 1..8 with four chaining wavefronts; 5 and 8 with eight; 2 and 8 in the panel form
SHAPES = [(64, s) for s in (3, 5, 9, 13, 17, 21, 25, 32)] + [(128, 17), (128, 32), (32, 5), (32, 32)]


@pytest.mark.parametrize("batch", [20, 40])
@pytest.mark.parametrize("H,dS", SHAPES, ids=["%dx%d-dS%d" % (h, h, s) for h, s in SHAPES])
def test_every_k_step_count_follows_the_oracle(hip_api, H, dS, batch):
    cfg_kw = dict(dimS=dS, dimA=2, hidden=(H, H), batchSize=batch, maxTotObsNum=2000, randSeed=7)
    G, O = _pair(hip_api, cfg_kw, synth_cfg(seed=91, dimS=dS, dimA=2, **SHORT), 150)
    for _ in range(2):
        G.step(1); O.step(1)
        _compare_step(G, O)
    G.step(8); O.step(8)
    assert np.array_equal(G.readback(capi.TAP_FLAT), O.readback(capi.TAP_FLAT))
    err = relinf(G.get_params()[0], O.get_params()[0])
    print("weights after 10 steps: relinf %.3g (bound %.3g)" % (err, 2 * TOL32))
    assert err < 2 * TOL32


def test_weight_gradient_table_on_a_net_with_every_problem_kind(hip_api):
    """Both layers' weights, the residual parameters' column sums, the output layer and the sigma bias: the summed gradient of one
    step against the oracle, at the tolerance every step comparison of the suite uses for it (TOL32, relative to the largest entry)."""
    cfg_kw = dict(dimS=5, dimA=2, hidden=(32, 32), batchSize=20, maxTotObsNum=2000, randSeed=7)
    G, O = _pair(hip_api, cfg_kw, synth_cfg(seed=92, dimS=5, dimA=2, **SHORT), 150)
    G.step(1); O.step(1)
    g, o = G.readback(capi.TAP_GRADSUM), O.readback(capi.TAP_GRADSUM)
    assert g.shape == o.shape and np.abs(o).max() > 0
    err = relinf(g, o)
    print("summed gradient after one step: relinf %.3g (bound %.3g)" % (err, TOL32))
    assert err < TOL32
