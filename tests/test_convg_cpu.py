"""CPU suite: which convolution geometries hl_create admits, asked on a machine without a device (the size checks stand in front of the
device query: an admissible net ends in HL_ERR_NO_DEVICE, a refused one in the bare status with no handle left), and the per-axis
form of a make_config conv entry.  NETS are the nets of tests/test_hip_convg.py, which runs them against the oracle on the GPU."""
import os
import subprocess
import sys

from smarties_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SAME3 = [(9, 7, 3, 5, 3, 1, (1, 1)), (9, 7, 5, 12, 3, 1, (1, 1))]
# name: (make_config keywords, synthetic episodes' keywords, episodes).  Conv entries: (W, H, C, filters, filter, stride[, padding]), pairs are (x, y)
NETS = {
    "same-3x3": (dict(dimS=189, dimA=2, conv=SAME3, hidden=(32,), nnFunc="SoftSign", batchSize=10, maxTotObsNum=800, randSeed=6),
                 dict(seed=8, dimS=189, dimA=2, lenMin=3, lenMax=12, pTerm=0.4), 25),
    "stride3": (dict(dimS=507, dimA=2, conv=[(13, 13, 3, 8, 3, 1), (11, 11, 8, 12, 5, 3, (2, 2))], hidden=(32,), nnFunc="Tanh", batchSize=12,
                     maxTotObsNum=900, randSeed=2),
                dict(seed=4, dimS=507, dimA=2, lenMin=3, lenMax=12, pTerm=0.4), 25),
    "aniso": (dict(dimS=280, dimA=2, conv=[(7, 10, 4, 8, (2, 3), (2, 1), (0, 1)), (3, 10, 8, 16, 3, (1, 2), (1, 0))], hidden=(32,), nnFunc="Tanh",
                   batchSize=12, maxTotObsNum=900, randSeed=3),
              dict(seed=5, dimS=280, dimA=2, lenMin=3, lenMax=12, pTerm=0.4), 25),
    "general-then-classic": (dict(dimS=576, dimA=2, conv=[(12, 12, 4, 8, 3, 1, (1, 1)), (12, 12, 8, 16, 4, 2)], hidden=(32,), nnFunc="Tanh",
                                  batchSize=12, maxTotObsNum=900, randSeed=2),
                             dict(seed=4, dimS=576, dimA=2, lenMin=3, lenMax=12, pTerm=0.4), 25),
    "wide-channels": (dict(dimS=100, dimA=2, conv=[(5, 5, 4, 72, 3, 1, (1, 1)), (5, 5, 72, 80, 3, 1, (1, 1))], hidden=(32,), nnFunc="Tanh",
                           batchSize=10, maxTotObsNum=800, randSeed=7),
                      dict(seed=9, dimS=100, dimA=2, lenMin=3, lenMax=12, pTerm=0.4), 25),
    "frames-extras": (dict(dimS=66, dimA=1, adv_kind=capi.ADV_DISCRETE, n_options=5, nAppendedObs=3, conv=[(8, 8, 4, 6, 3, 2, (1, 1))], hidden=(32,),
                           nnFunc="Tanh", batchSize=24, maxTotObsNum=2000, randSeed=3),
                      dict(seed=5, dimS=66, dimA=1, lenMin=3, lenMax=9, pTerm=0.3), 60),
    "big-batch": (dict(dimS=189, dimA=2, conv=SAME3, hidden=(32,), nnFunc="SoftSign", batchSize=1040, maxTotObsNum=4000, randSeed=6),
                  dict(seed=8, dimS=189, dimA=2, lenMin=20, lenMax=40, pTerm=0.4), 60),
}
BASE = dict(dimS=189, dimA=2, hidden=(32,), batchSize=10, maxTotObsNum=800)
REFUSED = {      # name: (make_config keywords, expected status)
    "stride-9": (dict(BASE, dimS=3 * 20 * 20, conv=[(20, 20, 3, 5, 3, (9, 1), (1, 1))]), 8),
    "padding-3-of-3": (dict(BASE, conv=[(9, 7, 3, 5, 3, 1, (3, 1))]), 8),
    "channels-257": (dict(BASE, conv=[(9, 7, 3, 257, 3, 1, (1, 1))]), 8),
    "lstm-behind-padding": (dict(BASE, conv=SAME3, nn_type=capi.NN_LSTM, nnBPTTseq=4), 8),
    "outY-off-the-formula": (dict(BASE, conv=SAME3), 1),      # (the child adds one to the first layer's outY)
}

_CODE = """
import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)
import ctypes as C
from smarties_amd import capi
from test_convg_cpu import NETS, REFUSED
api = capi.load_hip()
for name, kw in [(n, v[0]) for n, v in NETS.items()] + [(n, v[0]) for n, v in REFUSED.items()] + %r:
    cfg = capi.make_config(**kw)
    if name == "outY-off-the-formula": cfg.conv[0].outY += 1
    h = C.c_void_p()
    rc = api.fn("create")(C.byref(cfg), C.byref(h))
    print("CASE|%%s|%%d|%%s" %% (name, rc, "handle" if h else ""))
"""


def test_hl_create_admits_general_convolution_geometry():
    """One child process without a device for all cases: the status, and no handle left behind by any of them.  Beside NETS, the nets
    tests/blocks.py states for the per-block comparison (column segments, residue classes without a tap, strides up to 8, a padding of
    K - 1, 65 and 256 channels, a 1 x 1 filter): all admitted."""
    import blocks      # (imports this module: not at the top)
    more = [(n, blocks.SHAPES[n]["kw"]) for n in blocks.CONVG_NEW]
    assert len(more) == 5, more
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", _CODE % (ROOT, os.path.join(ROOT, "tests"), more)], capture_output=True, text=True, env=env)
    got = {}
    for line in out.stdout.splitlines():
        if line.startswith("CASE|"):
            _, name, rc, msg = line.split("|", 3)
            got[name] = (int(rc), msg)
    want = dict({n: 2 for n in list(NETS) + [n for n, _ in more]}, **{n: v[1] for n, v in REFUSED.items()})
    assert sorted(got) == sorted(want), out.stdout + out.stderr
    for name, rc in want.items():
        assert got[name] == (rc, ""), (name, got[name])


def test_make_config_takes_a_filter_a_stride_and_a_padding_per_axis():
    c = capi.make_config(dimS=280, dimA=2, conv=[(7, 10, 4, 8, (2, 3), (2, 1), (0, 1)), (3, 10, 8, 16, 3, 1)])
    fields = ("inpFeatures", "inpY", "inpX", "outFeatures", "outY", "outX", "filterx", "filtery", "stridex", "stridey", "paddinx", "paddiny")
    assert [getattr(c.conv[0], f) for f in fields] == [4, 10, 7, 8, 10, 3, 2, 3, 2, 1, 0, 1]
    assert [getattr(c.conv[1], f) for f in fields] == [8, 10, 3, 16, 8, 1, 3, 3, 1, 1, 0, 0]      # the six-number form: one filter, one stride, no padding
