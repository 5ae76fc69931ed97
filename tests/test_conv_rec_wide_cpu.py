"""CPU suite: which recurrent nets behind convolutions hl_create admits, asked on a machine without a device.  Every size check of these
nets stands in front of the device query, so an admissible configuration ends in HL_ERR_NO_DEVICE (as tests/test_cabi_symbols.py expects of
one) and a refused one in the bare HL_ERR_UNSUPPORTED, no handle left (with a device the refusal leaves a handle whose message names the
bound: tests/test_hip_conv_rec_wide.py).

Admitted beyond the per-sample kernels' limits (256 cells, a feature row of 1024 floats): LSTM / MGU layers that are multiples of
16 cells, 16 to 1024, on a feature row -- state variables beside the image + the last map -- of up to 8192 floats, without encoder layers."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONV2 = [(8, 8, 16, 32, 4, 1), (5, 5, 32, 64, 3, 1)]      # 4 x 256 stacked frames as 16 channels of 8 x 8 -> a feature row of 576
CASES = {
    # name: (make_config keywords, expected status, a word of the message a refusal carries where a device exists, or None)
    "conv-lstm-272": (dict(dimS=256, nAppendedObs=3, conv=CONV2, hidden=(272,), nn_type="LSTM"), 2, None),
    "conv-mgu-272x48": (dict(dimS=256, nAppendedObs=3, conv=CONV2, hidden=(272, 48), nn_type="MGU"), 2, None),
    "row-1331-lstm-32": (dict(dimS=338, conv=[(13, 13, 2, 11, 3, 1)], hidden=(32,), nn_type="LSTM"), 2, None),
    "row-8192-lstm-16": (dict(dimS=1024, conv=[(32, 32, 1, 8, 1, 1)], hidden=(16,), nn_type="LSTM"), 2, None),      # the upper bound itself
    "conv-lstm-1024": (dict(dimS=256, nAppendedObs=3, conv=CONV2, hidden=(1024,), nn_type="LSTM"), 2, None),
    # still refused
    "cells-264": (dict(dimS=256, nAppendedObs=3, conv=CONV2, hidden=(264,), nn_type="LSTM"), 8, "multiple of 16"),
    "cells-1040": (dict(dimS=256, nAppendedObs=3, conv=CONV2, hidden=(1040,), nn_type="LSTM"), 8, "1024"),
    "cells-272x40": (dict(dimS=256, nAppendedObs=3, conv=CONV2, hidden=(272, 40), nn_type="MGU"), 8, "multiple of 16"),
    "row-8200": (dict(dimS=1032, conv=[(32, 32, 1, 8, 1, 1)], hidden=(16,), nn_type="LSTM"), 8, "8192"),
    "row-1331-lstm-20": (dict(dimS=338, conv=[(13, 13, 2, 11, 3, 1)], hidden=(20,), nn_type="LSTM"), 8, "multiple of 16"),
    "rnn-272": (dict(dimS=256, nAppendedObs=3, conv=CONV2, hidden=(272,), nn_type="RNN"), 8, None),      # plain RNN layers behind convolutions: 256 cells, as before
    "encoder-in-front": (dict(dimS=256, nAppendedObs=3, conv=CONV2, hidden=(272,), encoder=[24], encoder_rnn=1, nn_type="MGU"), 8, None),
}

_CODE = """
import sys; sys.path.insert(0, %r)
import ctypes as C
from smarties_amd import capi
api = capi.load_hip()
NN = dict(LSTM=capi.NN_LSTM, MGU=capi.NN_MGU, RNN=capi.NN_RNN)
for name, (kw, _, _) in %r.items():
    kw = dict(kw, dimA=1, adv_kind=capi.ADV_DISCRETE, n_options=5, nnFunc="Tanh", batchSize=12, maxTotObsNum=2000, nnBPTTseq=4)
    kw["nn_type"] = NN[kw["nn_type"]]
    h = C.c_void_p()
    rc = api.fn("create")(C.byref(capi.make_config(**kw)), C.byref(h))
    print("CASE|%%s|%%d|%%s" %% (name, rc, "handle" if h else ""))
"""


def test_hl_create_admits_wide_recurrent_layers_behind_convolutions():
    """One child process without a device for all cases: the status, and no handle left behind by any of them."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", _CODE % (ROOT, CASES)], capture_output=True, text=True, env=env)
    got = {}
    for line in out.stdout.splitlines():
        if line.startswith("CASE|"):
            _, name, rc, msg = line.split("|", 3)
            got[name] = (int(rc), msg)
    assert sorted(got) == sorted(CASES), out.stdout + out.stderr
    for name, (_, want, word) in CASES.items():
        rc, msg = got[name]
        assert rc == want and msg == "", (name, rc, msg)


def test_the_input_gradient_kernel_carries_no_scratch():
    """The compiler's own remarks (kept beside the objects by build_hip): tm_conv_dx_kernel exists, spills nothing and uses no scratch."""
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    ks = [k for src in resource_usage.kernels().values() for k in src if k["name"] == "tm_conv_dx_kernel"]
    assert len(ks) == 1 and ks[0]["scratch"] == 0 and ks[0]["vgpr_spill"] == 0, ks


FIXTURES = ["conv_mgu_wide.bin", "conv_lstm_wide.bin"]      # tests/golden/make_conv_rec_wide.sh: a feature row of 1028 floats, narrow cells


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_follows_the_reference_on_a_wide_feature_row(name, tmp_path, monkeypatch):
    """The yardstick of tests/test_hip_conv_rec_wide.py: the CPU restatement through the bodies of tests/test_oracle_golden.py's
    conv-fixture tests on the two recordings of the compiled reference -- layout, initialisation and six steps."""
    import test_oracle_golden
    monkeypatch.setitem(test_oracle_golden.CONV_FUNC, name, "Tanh")
    test_oracle_golden.test_conv_layout_init_and_initialize_match_reference(name)
    test_oracle_golden.test_conv_steps_match_reference(name, tmp_path)
