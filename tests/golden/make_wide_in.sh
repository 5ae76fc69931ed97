#!/bin/bash
# Records tests/golden/lstm_wide_in.bin and tests/golden/mgu_wide_in.bin from the COMPILED REFERENCE (oracle/_ref/ref_driver_racer and
# oracle/_ref/ref_driver, built by oracle/Makefile): recurrent nets on inputs wider than a forward tile of the library stages --
#   lstm_wide_in.bin   RACER on two LSTM layers of 16 cells over a state of 1100 components (73 776 parameters, 450 600 bytes)
#   mgu_wide_in.bin    V-RACER on one MGU layer of 16 cells over a state of 300 components with 3 appended observations: a stacked input
#                      of 1200 (39 088 parameters, 257 624 bytes), drawn by the restricted sampler (minT = nApp + bptt: the reference itself
#                      reads in front of an episode's start otherwise)
# Data only (the reference's outputs); no reference source is stored.  lean=1 keeps the first gradient whole, so a recording grows with the
# parameter count: the layers are the narrowest the route takes.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
make -C "$ROOT/oracle" ref >/dev/null
TMP="$(mktemp -d)"; cd "$TMP"   # the reference writes agent_00_* log files into cwd
"$ROOT/oracle/_ref/ref_driver_racer" fixture "$HERE/lstm_wide_in.bin" dimS=1100 dimA=2 bounded=10 layers=16,16 nnType=LSTM nnFunc=Tanh bptt=3 \
   batch=8 nEps=30 lenMin=5 lenMax=40 pTerm=0.5 nSteps=6 gradSteps=1,2,6 retSteps=6 maxObs=2000 minObs=500 lean=1
"$ROOT/oracle/_ref/ref_driver" fixture "$HERE/mgu_wide_in.bin" dimS=300 dimA=2 bounded=01 nApp=3 minT=6 layers=16 nnType=MGU nnFunc=Tanh bptt=3 \
   batch=8 nEps=30 lenMin=10 lenMax=40 pTerm=0.5 nSteps=6 gradSteps=1,2,6 retSteps=6 maxObs=2000 minObs=500 lean=1
rm -rf "$TMP"
