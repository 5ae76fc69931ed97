"""Recurrent layers behind convolutions beyond the per-sample kernels' limits: LSTM / MGU layers of up to 1024 cells (multiples of
16; plain RNN layers behind convolutions keep the per-sample kernels and their 256 cells: tests/test_rnn_wide_cpu.py holds that refusal) on a feature row -- state variables beside the image + the last map -- of up to 8192 floats.  Such a net takes the time-step-major
launches (rectm.hip) where a layer exceeds 256 cells or the feature row 1024 floats: the conv stack runs over the B x (nnBPTTseq + 2)
window rows, the prepare launch copies its feature rows into the first layer's operand rows, tm_win_product_kernel and the chain follow;
the gradient into the feature rows is the table's GEMM_X problem up to 1024 inputs and tm_conv_dx_kernel beyond (or wherever
SMARTIES_HIP_GENERIC bit 2048 asks for it) -- the same problem under the same counter, hl_debug_conv_rec_dx says which form forms it.  Acting: the windows' rows through the conv stack, then the product and the acting
chain with the agents as samples, in chunks of min(local batch, HL_ACT_SEQ_CHUNK).

Against the CPU restatement on minibatches the library draws itself; tolerances are those of tests/test_hip_parity.py and
tests/test_hip_a22.py (TOL32 per tap, 2 TOL32 on the weights, integer taps equal)."""
import ctypes as C

import numpy as np
import pytest

from smarties_amd import capi
from oracle_api import synth_cfg, fill_synth
from blocks import CONV2, CONV2_EXTRA, CONV_1331, conv_rec_kw      # (the geometries and the configuration: tests/blocks.py steps them per block)
from parity import COL_ROWS, assert_columns, relinf
from parity import conv_rec_dx_call as _dx_call, conv_rec_dx_form as _dx_form
from test_hip_parity import hip_learner, _pair, _compare_step, TOL32

pytestmark = pytest.mark.gpu

NN = {"lstm": capi.NN_LSTM, "mgu": capi.NN_MGU, "rnn": capi.NN_RNN}
BPTT, BATCH = 4, 12


def _config(kind, hidden, conv, dS, nApp):
    return conv_rec_kw(NN[kind], hidden, conv, dS, nApp, batch=BATCH, bptt=BPTT)


def _counts(G, names):
    return {n: G.timing_get(n)[1] for n in names}


def _steps_and_acting_match_the_restatement(hip_api, kind, hidden, conv, dS, nApp, wide_dx):
    """Episodes of 3 - 12 steps: windows shorter than the BPTT length, steps t < nAppendedObs and truncated next states are sampled.  Four
    eager steps tap by tap, nine more, then weights and generator state; acting on one window of every length and on 3 and 65 ragged
    agents (65 at a local batch of 12: six chunks); a window one state too long is refused."""
    G, O = _pair(hip_api, _config(kind, hidden, conv, dS, nApp), synth_cfg(seed=5, dimS=dS, dimA=1, lenMin=3, lenMax=12, pTerm=0.3), 50)
    G.timing_enable(True)
    for _ in range(4):
        G.step(1); O.step(1)
        _compare_step(G, O)
    # the route: per step one prepare launch (the join), one product, one launch of the gradient into the feature rows, in the expected form
    labels = ["window_rows", "rec_prepare", "rec_in_product", "rec_forward", "rec_backward", "gemm16_dx%d" % len(hidden)]      # (the counter carries the number of layers behind the conv stack)
    got = _counts(G, labels)
    assert all(got[n] == 4 for n in labels), got
    assert _dx_form(G) == (1 if wide_dx else 0, 1)
    G.timing_enable(False)
    G.step(9); O.step(9)
    _compare_step(G, O)
    assert relinf(G.get_params()[0], O.get_params()[0]) < 2 * TOL32
    assert np.array_equal(G.get_rng_state(), O.get_rng_state())
    rng = np.random.default_rng(7)
    for n in sorted({1, 2, BPTT + 1, BPTT + 1 + nApp}):
        S = rng.normal(size=(n, dS)).astype(np.float32)
        assert relinf(G.forward_sequence(S), O.forward_sequence(S)) < TOL32, n
    lens = [1, 2, 3, BPTT + 1, BPTT + 1 + nApp]
    for agents in (3, 65):
        wins = [rng.normal(size=(lens[(i * 3 + agents) % len(lens)], dS)).astype(np.float32) for i in range(agents)]
        out = G.forward_sequences(wins)
        ref = np.stack([O.forward_sequence(w) for w in wins])
        assert out.shape == ref.shape
        for i in range(agents):
            assert relinf(out[i], ref[i]) < TOL32, (agents, i, len(wins[i]))
    with pytest.raises(capi.HlError):
        G.forward_sequence(rng.normal(size=(BPTT + 2 + nApp, dS)).astype(np.float32))
    with pytest.raises(capi.HlError):
        G.forward_sequences([rng.normal(size=(1, dS)).astype(np.float32), rng.normal(size=(BPTT + 2 + nApp, dS)).astype(np.float32)])
    G.close(); O.close()


@pytest.mark.parametrize("kind,hidden,extra", [("lstm", (272,), 0), ("mgu", (272, 48), 0), ("lstm", (272, 32), 6)],
                         ids=["lstm-272", "mgu-272x48", "lstm-272x32-extras"])
def test_wide_recurrent_layers_behind_convolutions_match_oracle(hip_api, kind, hidden, extra):
    """272 cells: one tile past 256, and 4 x 272 gate columns end in a ragged 64-column tile of the product.  576 (582 with the six state
    variables) inputs: the gradient into the feature rows is the GEMM_X problem."""
    if extra:
        _steps_and_acting_match_the_restatement(hip_api, kind, hidden, CONV2_EXTRA, 258, 2, False)
    else:
        _steps_and_acting_match_the_restatement(hip_api, kind, hidden, CONV2, 256, 3, False)


@pytest.mark.parametrize("kind,hidden", [("lstm", (32,)), ("mgu", (48, 16))], ids=["lstm-32", "mgu-48x16"])
def test_a_wide_feature_row_takes_the_route_with_narrow_cells(hip_api, kind, hidden):
    """A feature row of 1331 floats in front of layers the per-sample kernels would hold: the product's scalar tail (1331 is odd), a last
    slice of 19 columns, and tm_conv_dx_kernel for the gradient into the rows (21 input tiles, the last one of 51 columns)."""
    _steps_and_acting_match_the_restatement(hip_api, kind, hidden, CONV_1331, 338, 0, True)


def _dx_blocks(L):
    """(gate deltas, residual deltas, Dres of the last convolution's rows) as the last step left them (hl_debug_conv_rec_dx)"""
    f = _dx_call(L)
    out = []
    for which in (0, 1, 2):
        dims = (C.c_int32 * 2)()
        L._ck(f(L.h, which, None, 0, dims))
        a = np.zeros((dims[0], dims[1]), np.float32)
        L._ck(f(L.h, which, a.ctypes.data_as(C.c_void_p), a.size, dims))
        out.append(a)
    return out


def test_both_forms_of_the_gradient_into_the_feature_rows_against_fp64(hip_api, monkeypatch):
    """576 features under 272 LSTM cells: both forms serve.  One learner takes the GEMM_X / EPI_DX problem, its twin (SMARTIES_HIP_GENERIC
    bit 2048) tm_conv_dx_kernel; same weights, same replay, same minibatch.  Each one's Dres of the last convolution's 72 window rows is
    held, COLUMN BY COLUMN on the column's own scale, to the same product in double of its own operands (the gate deltas and residual
    deltas it read, the weights): a bound on the worst row would hide a wrong column.  Rows of steps a sample does not have are zero.
    (parity.twin64, the restatement in double, answers the acting calls only: it has no tap for a hidden layer's input gradient, so the
    product in double is formed here, in numpy, from the operands hl_debug_conv_rec_dx reads back; it depends on neither kernel.)"""
    kw = _config("lstm", (272,), CONV2, 256, 3)
    sc = synth_cfg(seed=5, dimS=256, dimA=1, lenMin=3, lenMax=12, pTerm=0.3)
    got = {}
    for bit in (0, 2048):
        monkeypatch.setenv("SMARTIES_HIP_GENERIC", str(bit))
        L = hip_learner(hip_api, capi.make_config(**kw))
        L.init_weights(); fill_synth(L, sc, 50); L.initialize(); L.set_tap(True)
        L.timing_enable(True)
        L.step(1)
        assert L.timing_get("gemm16_dx1")[1] == 1 and _dx_form(L) == (1 if bit else 0, 1)
        D, Rd, Dres = _dx_blocks(L)
        lay, t = L.layout(), L.readback(capi.TAP_TSTEP)
        got[bit] = (D, Rd, Dres, lay, t)
        L.close()
    monkeypatch.delenv("SMARTIES_HIP_GENERIC")
    # the weights both learners read during the step: a third one, initialised alike and not stepped
    L = hip_learner(hip_api, capi.make_config(**kw)); L.init_weights()
    w = L.get_params()[0].astype(np.float64); L.close()
    D0, Rd0, _, lay, t = got[0]
    assert np.array_equal(D0, got[2048][0]) and np.array_equal(Rd0, got[2048][1])      # everything in front of the launch is the same code
    nIn, nC = 576, 272
    iW, iWr = int(lay["indW"][3]), int(lay["indW"][4])      # layers: input, two convolutions, the LSTM layer, its parametric residual, output
    assert int(lay["nW"][3]) == 4 * nC * (nIn + nC) and int(lay["nW"][4]) == nC
    Win = w[iW:iW + nIn * 4 * nC].reshape(nIn, 4 * nC)
    ref = D0.astype(np.float64) @ Win.T
    ref[:, :nC] += Rd0[:, :nC].astype(np.float64) * w[iWr:iWr + nC]
    assert ref.shape[0] == BATCH * (BPTT + 2) >= COL_ROWS
    K = BPTT + 2
    for b in range(BATCH):      # rows behind the sample's last step, the next state's row among them
        T = min(BPTT, int(t[b]))
        assert not D0[b * K + T + 1:(b + 1) * K].any()
    for bit in (0, 2048):
        Dres = got[bit][2][:, :nIn]
        assert_columns(Dres, ref, TOL32, "Dres, SMARTIES_HIP_GENERIC bit %d" % bit)
        for b in range(BATCH):
            T = min(BPTT, int(t[b]))
            assert not Dres[b * K + T + 1:(b + 1) * K].any(), (bit, b)


def test_two_runs_end_bit_identical(hip_api):
    """1 + 5 + 9 steps of 272 LSTM cells behind two convolutions, twice: every element of the product and of the gradient into the
    feature rows is one chain of MFMAs, the backward diagonals join their producers in a fixed order."""
    sc = synth_cfg(seed=5, dimS=256, dimA=1, lenMin=3, lenMax=12, pTerm=0.3)

    def run():
        L = hip_learner(hip_api, capi.make_config(**_config("lstm", (272,), CONV2, 256, 3)))
        L.init_weights(); fill_synth(L, sc, 50); L.initialize()
        for n in (1, 5, 9):
            L.step(n)
        L.sync()
        out = (L.get_params()[0].copy(), L.get_rng_state().copy(), L.scalars().beta)
        L.close()
        return out
    a, b = run(), run()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_the_device_window_calls_keep_refusing_these_nets(hip_api):
    """hl_forward_sequences_dev serves recurrent nets without convolutions in front: refused with the text it had, as hl_forward is."""
    import torch
    L = hip_learner(hip_api, capi.make_config(**_config("lstm", (272,), CONV2, 256, 3)))
    L.init_weights()
    st = torch.zeros((2, 256), dtype=torch.float32, device="cuda")
    with pytest.raises(capi.HlError) as e:
        L.forward_sequences_dev(st, torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), 2, dtype=torch.int32, device="cuda"), 1)
    assert e.value.status == 8 and "hl_forward_sequences" in str(e.value)
    with pytest.raises(capi.HlError):
        L.forward(np.zeros((1, L.dIn), np.float32))
    L.close()


def test_without_the_time_step_major_launches_these_nets_are_refused_with_a_message(hip_api, monkeypatch):
    """SMARTIES_HIP_GENERIC bit 4 switches the time-step-major launches off: nothing else serves these nets, as for wide inputs."""
    monkeypatch.setenv("SMARTIES_HIP_GENERIC", "4")
    for kind, hidden, conv, dS, nApp in (("lstm", (272,), CONV2, 256, 3), ("lstm", (32,), CONV_1331, 338, 0)):
        with pytest.raises(capi.HlError) as e:
            hip_learner(hip_api, capi.make_config(**_config(kind, hidden, conv, dS, nApp)))
        assert e.value.status == 8 and "bit 4" in str(e.value)
    L = hip_learner(hip_api, capi.make_config(**_config("lstm", (32,), CONV2, 256, 3)))      # within the per-sample kernels' limits: served as before
    assert _dx_form(L) == (0, 0)
    L.close()


def test_refusals_name_the_bound_where_a_device_exists(hip_api):
    """The refused neighbours of tests/test_conv_rec_wide_cpu.py on the GPU: HL_ERR_UNSUPPORTED with a handle whose message names the bound."""
    from test_conv_rec_wide_cpu import CASES
    for name, (kw, want, word) in CASES.items():
        if not word:
            continue
        kw = dict(kw, dimA=1, adv_kind=capi.ADV_DISCRETE, n_options=5, nnFunc="Tanh", batchSize=12, maxTotObsNum=2000, nnBPTTseq=4)
        kw["nn_type"] = NN[kw["nn_type"].lower()]
        with pytest.raises(capi.HlError) as e:
            hip_learner(hip_api, capi.make_config(**kw))
        assert e.value.status == want and word in str(e.value), (name, str(e.value))


@pytest.mark.parametrize("name", ["conv_mgu_wide.bin", "conv_lstm_wide.bin"])
def test_steps_follow_the_reference_on_a_wide_feature_row(hip_api, name):
    """tests/golden/make_conv_rec_wide.sh: MGU 48 + 16 and LSTM 32 on a feature row of 228 state variables + 800 map floats, recorded from
    the compiled reference; test_conv_steps_follow_reference_fixture's body.  1028 inputs: tm_conv_dx_kernel forms the gradient into the rows."""
    from test_hip_parity import test_conv_steps_follow_reference_fixture as body
    body(hip_api, name)
