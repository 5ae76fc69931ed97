"""On the GPU: convolutional layers of general geometry (convg.hip: zero padding, a stride per axis, strides that are no power of two,
more than 64 channels) against the CPU oracle, through the body of test_hip_parity.py's test_conv_and_appended_observations_match_oracle
and its bounds.  The nets and what each can break: tests/test_convg_cpu.py (NETS) and the table in DESIGN.md section 8."""
import numpy as np
import pytest

from oracle_api import synth_cfg
from parity import relinf
from smarties_amd import capi
from test_convg_cpu import NETS
from test_hip_parity import TOL32, _compare_step, _pair

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(NETS))
def test_general_geometry_convolutions_match_oracle(hip_api, name):
    cfg_kw, sc_kw, n_eps = NETS[name]
    G, O = _pair(hip_api, cfg_kw, synth_cfg(**sc_kw), n_eps)
    for _ in range(5):
        G.step(1); O.step(1)
        _compare_step(G, O)
        w, m1, m2 = G.get_params(); wo, m1o, m2o = O.get_params()
        assert relinf(w, wo) < TOL32 and relinf(m1, m1o) < 2 * TOL32 and relinf(m2, m2o) < 2 * TOL32
        assert G.scalars().nFarPolicySteps == O.scalars().nFarPolicySteps
    G.step(21); O.step(21)                      # replayed graphs
    _compare_step(G, O)
    assert relinf(G.get_params()[0], O.get_params()[0]) < 2 * TOL32
    assert np.array_equal(G.get_rng_state(), O.get_rng_state())
    st = np.random.default_rng(0).normal(size=(3, G.dIn)).astype(np.float32)      # rollout inference on stacked raw states
    assert relinf(G.forward(st), O.forward(st)) < TOL32
