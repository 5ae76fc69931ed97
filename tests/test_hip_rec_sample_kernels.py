"""The workgroup-per-sample recurrent kernels (smarties_amd/csrc/rec.hip: rec_*, lstm_*_lds, mgu_*, rnn_*), instantiation by instantiation.

Each case is the smallest net that selects one instantiation.  hl_debug_rec_route (rec.hip: rec_route_name) states which kernel the
training launches take; the case asserts it, then holds three steps, the parameters and hl_forward_sequence to the CPU oracle.  The
segment forms (YoutRows / DresRows), the convolutional front and the many-agent acting forms are covered by test_hip_act_win.py,
test_hip_act_batch.py and test_hip_a22.py."""
import numpy as np
import pytest

from oracle_api import synth_cfg
from parity import relinf
from smarties_amd import capi
from test_hip_r4 import _pair, _compare_step, TOL32

pytestmark = pytest.mark.gpu

# name: (nn_type, hidden, dimS, extra configuration, forward kernel, backward kernel)
SHAPES = {
    "rnn-20": (capi.NN_RNN, (20,), 6, {}, "rnn_forward_kernel<true>", "rnn_backward_kernel<true>"),
    # 168 rows of 161 floats = 108 192 B of weights: over the 100 KB cut
    "rnn-160-l2": (capi.NN_RNN, (160,), 8, {}, "rnn_forward_kernel<false>", "rnn_backward_kernel<false>"),
    "mgu-8": (capi.NN_MGU, (8,), 5, {}, "mgu_forward_kernel<true, 1>", "mgu_backward_kernel<true, 1>"),
    "mgu-12-8": (capi.NN_MGU, (12, 8), 5, {}, "mgu_forward_kernel<true, 2>", "mgu_backward_kernel<true, 2>"),
    "mgu-8-8-8": (capi.NN_MGU, (8, 8, 8), 5, {}, "mgu_forward_kernel<true, 0>", "mgu_backward_kernel<true, 0>"),
    # appended observations: the first layer's input is not the step's own state
    "mgu-8-app1": (capi.NN_MGU, (8,), 5, dict(nAppendedObs=1), "mgu_forward_kernel<true, 0>", "mgu_backward_kernel<true, 0>"),
    # 8 inputs: no multiple of 16, so not time-step-major; 247 KB of weights
    "mgu-100-100-l2": (capi.NN_MGU, (100, 100), 8, {}, "mgu_forward_kernel<false, 0>", "mgu_backward_kernel<false, 0>"),
    "lstm-8": (capi.NN_LSTM, (8,), 5, {}, "lstm_forward_lds_kernel<1, 0>", "lstm_backward_lds_kernel<1>"),
    "lstm-12-8": (capi.NN_LSTM, (12, 8), 5, {}, "lstm_forward_lds_kernel<2, 0>", "lstm_backward_lds_kernel<2>"),
    "lstm-8-8-8": (capi.NN_LSTM, (8, 8, 8), 5, {}, "lstm_forward_lds_kernel<3, 0>", "lstm_backward_lds_kernel<3>"),
    "lstm-8-8-8-8": (capi.NN_LSTM, (8, 8, 8, 8), 5, {}, "lstm_forward_lds_kernel<0, 0>", "lstm_backward_lds_kernel<0>"),
    # 33 inputs: too wide for the wave kernels of two 32-cell layers
    "lstm-32-32-in33": (capi.NN_LSTM, (32, 32), 33, {}, "lstm_forward_lds_kernel<2, 32>", "lstm_backward_lds_kernel<2>"),
    # 20 steps of 256 states do not fit REC_STATES: the states are fetched step by step
    "lstm-8-no-preload": (capi.NN_LSTM, (8,), 256, dict(nnBPTTseq=18), "lstm_forward_lds_kernel<1, 0>", "lstm_backward_lds_kernel<1>"),
    "lstm-8-app1": (capi.NN_LSTM, (8,), 5, dict(nAppendedObs=1), "rec_forward_kernel<true>", "rec_backward_kernel<true>"),
    # 72 cells: beyond the 64 of the lds kernels; 259 KB of weights
    "lstm-72-72-l2": (capi.NN_LSTM, (72, 72), 8, {}, "rec_forward_kernel<false>", "rec_backward_kernel<false>"),
}


def shape_cfg(name):
    """(configuration, synthetic-replay settings) of a case"""
    nn_type, hidden, dS, extra, _, _ = SHAPES[name]
    kw = dict(dimS=dS, dimA=1, hidden=hidden, nnFunc="Tanh", batchSize=3, maxTotObsNum=8000, randSeed=17, nn_type=nn_type, nnBPTTseq=2,
              adv_kind=capi.ADV_GAUSSIAN)
    kw.update(extra)
    return kw, synth_cfg(seed=23, dimS=dS, dimA=1, lenMin=2, lenMax=max(8, kw["nnBPTTseq"] + 6), pTerm=0.5)


def act_windows(kw, seed=31):
    """windows of 1, 2 and nnBPTTseq + 1 states"""
    rng = np.random.default_rng(seed)
    return [(rng.normal(size=(n, kw["dimS"])) * 1.5 + 0.2).astype(np.float32) for n in (1, 2, kw["nnBPTTseq"] + 1)]


@pytest.mark.parametrize("name", list(SHAPES))
def test_instantiation_is_reached_and_matches_oracle(hip_api, name):
    kw, sc = shape_cfg(name)
    G, O = _pair(hip_api, kw, sc, 30)
    assert G.debug_rec_route(False) == SHAPES[name][4]
    assert G.debug_rec_route(True) == SHAPES[name][5]
    for _ in range(3):
        G.step(1); O.step(1)
        _compare_step(G, O)
    assert relinf(G.get_params()[0], O.get_params()[0]) < 2 * TOL32
    for w in act_windows(kw):
        assert relinf(G.forward_sequence(w), O.forward_sequence(w)) < TOL32, w.shape[0]
    G.close(); O.close()
