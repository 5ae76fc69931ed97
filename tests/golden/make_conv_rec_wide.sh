#!/bin/bash
# Records tests/golden/conv_mgu_wide.bin and tests/golden/conv_lstm_wide.bin from the COMPILED REFERENCE (oracle/_ref/ref_driver_discrete,
# built by oracle/Makefile): recurrent layers behind a convolution on the route of the wide feature rows --
#   conv_mgu_wide.bin    MGU 48 + 16 cells (114 864 parameters, 659 383 bytes)
#   conv_lstm_wide.bin   LSTM 32 cells     (145 392 parameters, 815 983 bytes)
# both discrete RACER with 4 options on 1 + 3 stacked states of 313 components: the first 1024 of the 1252 stacked floats are the
# 8 x 8 x 16 image of the third RACER_atari convolution (the reference builds only the geometries Builder.cpp declares), the other 228
# are state variables beside it, so the first recurrent layer reads a feature row of 228 + 800 = 1028 floats: beyond the 1024 the
# per-sample kernels hold, and the library takes the time-step-major launches with narrow cells (tm_win_product_kernel, tm_conv_dx_kernel).
# Drawn by the restricted sampler (minT = nApp + bptt: the reference itself reads in front of an episode's start otherwise).
# Data only (the reference's outputs); no reference source is stored.  lean=1 keeps the first gradient whole, so a recording grows with
# the parameter count: a layer of 272 cells needs 272 inputs at least (2 x 272 x 544 MGU weights: 2.7 MB recorded), which is why the
# layers beyond 256 cells are held to the CPU restatement alone (tests/test_hip_conv_rec_wide.py) and these two pin the restatement.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
make -C "$ROOT/oracle" ref >/dev/null
TMP="$(mktemp -d)"; cd "$TMP"   # the reference writes agent_00_* log files into cwd
COMMON='dimS=313 dimA=1 nOpt=4 nApp=3 minT=7 conv=8,8,16,32,4,1'
TAIL='nnFunc=Tanh bptt=4 batch=16 nEps=30 lenMin=10 lenMax=40 pTerm=0.5 nSteps=6 gradSteps=1,2,6 retSteps=6 maxObs=2000 minObs=500 lean=1'
"$ROOT/oracle/_ref/ref_driver_discrete" fixture "$HERE/conv_mgu_wide.bin" $COMMON layers=48,16 nnType=MGU $TAIL
"$ROOT/oracle/_ref/ref_driver_discrete" fixture "$HERE/conv_lstm_wide.bin" $COMMON layers=32 nnType=LSTM $TAIL
rm -rf "$TMP"
