"""The host arithmetic of rollout inference (smarties_amd/csrc/act_host.h: the carve of a pinned block, the stacked rows of appended
observations, the tables of a chunk of ragged windows) on the CPU: tests/cpp/act_host_check.cpp, a stand-alone program, built with the
address and undefined-behaviour sanitizers linked in and run as a child process.  Its buffers have exactly the sizes learner_act.h gives
them, so an overrun fails the run; its expectations re-state the contract of include/smarties_hip_act.h float by float."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_act_host_helpers_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/cpp/act_host_check.cpp")
    exe = str(tmp_path / "act_host_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "cpp", "act_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "act_host_check: ok" in r.stdout, r.stdout
