"""CPU suite: bench.py's --dump-outputs plumbing -- the arrays a caller of the timed path receives, collected through the C-ABI (here
from the CPU oracle, which answers the same calls) and written as .npy files in float32 / float64; and the options of a plain run."""
import os
import subprocess
import sys

import numpy as np

import bench
from oracle_api import oracle_learner, fill_synth, synth_cfg
from smarties_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _outputs_after_steps():
    L = oracle_learner(capi.make_config(dimS=17, dimA=6, hidden=(32, 32), batchSize=16, maxTotObsNum=4096, randSeed=42))
    L.init_weights()
    fill_synth(L, synth_cfg(seed=7, dimS=17, dimA=6, lenMin=20, lenMax=40, pTerm=0.3), 80)
    L.initialize()
    L.set_tap(True)
    L.step(5)
    return L, bench.step_outputs(L)


def test_outputs_of_the_timed_path_are_written_as_float_arrays(tmp_path):
    L, out = _outputs_after_steps()
    names = bench.write_arrays(str(tmp_path), out)
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in names)
    total = 0
    for n in names:
        a = np.load(tmp_path / (n + ".npy"))
        assert a.dtype in (np.float32, np.float64), (n, a.dtype)
        assert np.array_equal(a, np.asarray(out[n]).astype(a.dtype)), n
        total += a.nbytes
    assert total <= bench.DUMP_MAX_BYTES
    w = np.load(tmp_path / "weights.npy")
    assert w.dtype == np.float32 and w.size == L.nParams and np.array_equal(w, L.get_params()[0])
    assert np.load(tmp_path / "last_step_outputs.npy").shape == (L.B, L.nOut)
    assert np.load(tmp_path / "replay_sample_episodes.npy").size == bench.DUMP_EPISODES


def test_same_inputs_give_the_same_outputs():
    a, b = _outputs_after_steps()[1], _outputs_after_steps()[1]
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_budget_is_enforced(tmp_path):
    big = {"x": np.zeros(bench.DUMP_MAX_BYTES // 4 + 1, np.float32)}
    try:
        bench.write_arrays(str(tmp_path), big)
    except ValueError:
        return
    raise AssertionError("an output over the budget was written")


def test_command_line_has_the_plain_and_full_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in r.stdout, opt
