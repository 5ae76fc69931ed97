#!/bin/bash
# Records tests/golden/rnn_wide.bin from the COMPILED REFERENCE (oracle/_ref/ref_driver_racer, built by oracle/Makefile):
# RACER on a plain RNN stack of 320 x 96 cells (nnType "RNN": BaseLayer with bRecurrent), the first layer beyond the 256 cells the
# per-sample kernels hold, the second with a parametric residual narrower than the layer below.  Data only (the reference's outputs);
# no reference source is stored.
# lean=1 keeps the first gradient whole, so the recording grows with the parameter count: 145328 floats here, 0.81 MB in all.  (Two
# layers above 256 cells, 320 x 272 = 268352 parameters, give 1.44 MB; those stacks are compared with the oracle in
# tests/test_hip_rnn_wide.py, and the oracle is pinned to the reference by this recording.)
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
make -C "$ROOT/oracle" ref >/dev/null
TMP="$(mktemp -d)"; cd "$TMP"   # the reference writes agent_00_* log files into cwd
"$ROOT/oracle/_ref/ref_driver_racer" fixture "$HERE/rnn_wide.bin" dimS=5 dimA=2 bounded=10 layers=320,96 nnType=RNN nnFunc=Tanh bptt=4 \
   batch=16 nEps=30 lenMin=5 lenMax=40 pTerm=0.5 nSteps=6 gradSteps=1,2,6 retSteps=6 maxObs=2000 minObs=500 lean=1
rm -rf "$TMP"
