"""Recurrent nets on wide inputs (a state beyond 256 components, or a stacked input beyond 1024, up to 8192; rectm.hip: tm_win_product_kernel
and the tm_win_*_fwd kernels), the parts that need no GPU: the checker itself against two fixtures recorded from the compiled reference
(tests/golden/make_wide_in.sh), the argument checks of hl_create, the compiler's resource figures of the new kernels."""
import os
import sys

import pytest

import test_oracle_golden
from test_rnn_wide_cpu import _create_status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_follows_reference_fixture_lstm_on_1100_states(monkeypatch):
    """Six RACER steps on two LSTM layers of 16 cells over a state of 1100 components: pins the checker the GPU tests compare with."""
    monkeypatch.setitem(test_oracle_golden.FUNC_OF, "lstm_wide_in.bin", "Tanh")
    test_oracle_golden.test_steps_match_reference("lstm_wide_in.bin")


def test_oracle_follows_reference_fixture_mgu_on_1200_stacked_inputs(monkeypatch, tmp_path):
    """Six V-RACER steps on an MGU layer of 16 cells over 300 states with three appended observations, minibatches from the restricted
    sampler (the body lstm_appended.bin goes through)."""
    monkeypatch.setitem(test_oracle_golden.CONV_FUNC, "mgu_wide_in.bin", "Tanh")
    test_oracle_golden.test_conv_layout_init_and_initialize_match_reference("mgu_wide_in.bin")
    test_oracle_golden.test_conv_steps_match_reference("mgu_wide_in.bin", tmp_path)


ACCEPTED = [
    ("lstm-16x16-dS1100", dict(nn_type="NN_LSTM", hidden=(16, 16), dimS=1100)),
    ("mgu-16-dS300x4", dict(nn_type="NN_MGU", hidden=(16,), dimS=300, nAppendedObs=3)),
    ("rnn-272-dS1030", dict(nn_type="NN_RNN", hidden=(272,), dimS=1030)),
    ("lstm-32x16-dS257", dict(nn_type="NN_LSTM", hidden=(32, 16), dimS=257)),
    ("lstm-16-dS8192", dict(nn_type="NN_LSTM", hidden=(16,), dimS=8192)),
]
REFUSED = [
    ("20-cells-dS300", dict(nn_type="NN_LSTM", hidden=(20,), dimS=300)),                    # a layer that is no multiple of 16 cells
    ("16-dS8193", dict(nn_type="NN_LSTM", hidden=(16,), dimS=8193)),                        # a stacked input above 8192
    ("16-dS2048x5", dict(nn_type="NN_LSTM", hidden=(16,), dimS=2048, nAppendedObs=4)),      # ... from appended observations
    ("lstm-32-dS300-behind-encoder", dict(nn_type="NN_LSTM", hidden=(32,), dimS=300, encoder=[32])),
]


@pytest.mark.parametrize("kw", [kw for _, kw in ACCEPTED], ids=[n for n, _ in ACCEPTED])
def test_hl_create_accepts_wide_inputs(kw):
    """(2 = HL_ERR_NO_DEVICE: the size checks passed and the device was asked for)"""
    assert _create_status(kw) == 2


@pytest.mark.parametrize("kw", [kw for _, kw in REFUSED], ids=[n for n, _ in REFUSED])
def test_hl_create_still_refuses(kw):
    assert _create_status(kw) == 8


def test_wide_input_kernels_carry_no_scratch():
    """The compiler's own remarks (kept beside the objects by build_hip): the product kernel and the three forward kernels whose first layer
    takes its input product from it exist, spill nothing and use no scratch."""
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    ks = [k for src in resource_usage.kernels().values() for k in src if k["name"].startswith("tm_win_")]
    assert sorted(k["name"] for k in ks) == ["tm_win_lstm_fwd_kernel", "tm_win_mgu_fwd_kernel", "tm_win_product_kernel", "tm_win_rnn_fwd_kernel"]
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
