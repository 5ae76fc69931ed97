"""CPU suite: hl_config::reduction_timing (include/smarties_hip.h: HL_RDX_CURRENT / HL_RDX_ONE_BEHIND) -- validated by hl_create with the
other settings, before the device probe; the previous 704-byte layout still accepted; the ctypes mirror laid out as the C header."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

from smarties_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _create_without_device(assignments):
    """hl_create's status in a process that sees no device; `assignments` are Python statements on `cfg` (a capi.make_config())."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from smarties_amd import capi\n"
            "import ctypes as C\n"
            "api = capi.load_hip(); h = C.c_void_p(); cfg = capi.make_config()\n"
            "%s\n"
            "rc = api.fn('create')(C.byref(cfg), C.byref(h)); print('RC', rc)\n" % (ROOT, assignments))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    for line in out.stdout.splitlines():
        if line.startswith("RC "):
            return int(line[3:])
    raise AssertionError(out.stdout + out.stderr)


@pytest.mark.parametrize("value", [2, -1])
def test_unknown_reduction_timing_is_a_bad_argument(value):
    assert _create_without_device("cfg.reduction_timing = %d" % value) == 1      # HL_ERR_BAD_ARG, before the device probe


def test_one_behind_passes_validation():
    assert _create_without_device("cfg.reduction_timing = capi.RDX_ONE_BEHIND") == 2      # HL_ERR_NO_DEVICE: it got as far as the probe


def test_previous_config_layout_is_accepted():
    # an embedding built against the header without reduction_timing passes struct_size 704; the field then reads as HL_RDX_CURRENT
    # (whatever lies behind the 704 bytes is not read: here an invalid value)
    assert _create_without_device("cfg.struct_size = 704; cfg.reduction_timing = 7") == 2


def test_make_config_keyword():
    assert capi.make_config().reduction_timing == capi.RDX_CURRENT
    assert capi.make_config(reduction_timing="one_behind").reduction_timing == capi.RDX_ONE_BEHIND
    assert capi.make_config(reduction_timing=capi.RDX_ONE_BEHIND).reduction_timing == 1


def test_ctypes_config_matches_the_c_layout(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smarties_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d\\n", sizeof(hl_config), offsetof(hl_config, reduction_timing), '
                   'offsetof(hl_config, encoder_rnn), HL_CONFIG_SIZE_V1); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call([cc, "-x", "c", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(exe)])
    size, off, off_prev, v1 = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(capi.HlConfig) == 712
    assert off == capi.HlConfig.reduction_timing.offset
    assert off_prev == capi.HlConfig.encoder_rnn.offset
    assert v1 == 704 == off_prev + 4      # the previous layout ended with encoder_rnn
