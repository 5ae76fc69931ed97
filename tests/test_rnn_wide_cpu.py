"""Plain RNN layers (nnType "RNN") wider than 256 cells, the parts that need no GPU: the checker itself against a fixture recorded from
the compiled reference, the argument checks of hl_create, the compiler's resource figures of the time-step-major RNN kernels."""
import os
import subprocess
import sys

import pytest

import test_oracle_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_follows_reference_fixture_above_256_cells(monkeypatch):
    """The CPU oracle follows the reference through six RACER steps on 320 x 96 RNN cells: pins the checker the GPU tests compare with.
    The recording covers ONE layer above 256 cells (its whole first gradient has to fit a committed file); stacks with two such layers are
    compared with the oracle only (tests/test_hip_rnn_wide.py)."""
    monkeypatch.setitem(test_oracle_golden.FUNC_OF, "rnn_wide.bin", "Tanh")
    test_oracle_golden.test_steps_match_reference("rnn_wide.bin")


ACCEPTED = [dict(hidden=(512,)), dict(hidden=(320, 272)), dict(hidden=(1024, 1024))]
REFUSED = [
    dict(hidden=(260,)),                                                # above 256 cells and no multiple of 16
    dict(hidden=(1040,)),                                               # above 1024 cells
    dict(hidden=(512,), encoder=[32]),                                  # behind encoder layers
    dict(hidden=(512,), dimS=576, conv=[(12, 12, 4, 8, 3, 1)]),         # behind a convolution
    dict(hidden=(32,), nn_type="NN_MGU", encoder_rnn=1, encoder=[272]), # an RNN encoder segment above 256 cells
]


def _create_status(kw):
    """Status of hl_create in a process that sees no device: the size checks run before the device is opened, so a shape the library
    serves ends with HL_ERR_NO_DEVICE (2) and one it refuses with HL_ERR_UNSUPPORTED (8)."""
    kw = dict(kw)
    nnt = kw.pop("nn_type", "NN_RNN")
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from smarties_amd import capi\n"
            "import ctypes as C\n"
            "api = capi.load_hip(); h = C.c_void_p(); cfg = capi.make_config(nn_type=capi.%s, **%r)\n"
            "rc = api.fn('create')(C.byref(cfg), C.byref(h)); print('RC', rc)\n" % (ROOT, nnt, kw))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert "RC " in out.stdout, out.stdout + out.stderr
    return int(out.stdout.split("RC ")[1].split()[0])


@pytest.mark.parametrize("kw", ACCEPTED, ids=lambda kw: "x".join(map(str, kw["hidden"])))
def test_hl_create_accepts_rnn_layers_up_to_1024_cells(kw):
    assert _create_status(kw) == 2


@pytest.mark.parametrize("kw", REFUSED, ids=["260", "1040", "512-behind-encoder", "512-behind-conv", "mgu-rnn-encoder-272"])
def test_hl_create_still_refuses(kw):
    assert _create_status(kw) == 8


def test_rnn_tm_kernels_carry_no_scratch():
    """The compiler's own remarks (kept beside the objects by build_hip): the time-step-major RNN kernels exist, spill nothing and use no scratch."""
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    ks = [k for src in resource_usage.kernels().values() for k in src if k["name"].startswith("rnn_tm_")]
    assert sorted(k["name"] for k in ks) == ["rnn_tm_bwd_kernel", "rnn_tm_fwd_kernel"]
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
