"""Shared by tests/test_blocks_cpu.py and tests/test_hip_blocks.py: the shapes (one per launch route of the training step: every
counter of ROUTE_COUNTERS fires in a recorded route or is in EXCUSED, tests/test_blocks_cpu.py), the fp32 / fp64 pair of the CPU
restatement stepped side by side, and the per-block deviations.

O32 is oracle/liboracle_port.so, O64 its build with the arrays in double (oracle/liboracle_port64.so).  Both start from the
same fp32 weights and the same synthetic replay and draw their own minibatches.  e_cpu(block) = dev(O32, O64) is what fp32
arithmetic in the reference's own summation order loses in that block; the CPU test holds it to TOL32 / 3, which is what makes
TOL32 per block a fair bar for e_hip(block) = dev(HIP, O64) in the GPU test.  A block that cannot meet TOL32 / 3 because it is
ill-conditioned is LISTED in its shape's entry with the e_cpu measured on the CPU; its GPU bar is 4 e_cpu, taken at test time.

Why blocks get listed.  Most of them are bias blocks of W in the first steps: hidden biases start at zero, so after k steps a
bias IS the sum of k Adam updates eta numer / (eps + sqrt(M2)), each of size ~eta.  For a bias whose gradient is small -- 0.1 |g| / B
comparable to eps = FLT_EPSILON, where the quotient turns from |g| / eps to 1 -- an absolute error of the gradient sum of 5e-7 of the
block's largest element (ordinary fp32 summation) moves the quotient by up to 0.4 max|g| / B: 1e-5 of the block's largest update and
more.  Weight blocks do not show it (their elements are 1000 eta large), nor do M1 / M2 / gradSum (no quotient).
The recurrent shapes on wide inputs, wide layers and feature rows behind convolutions list a few blocks that are no biases (a gate's
input or recurrent weights in W, M1 or M2, a tap column): there every pre-activation is a sum of 1000 to 2000 terms, and the batch
of 4 to 20 samples is too small to average the rounding of such a sum out of a block's largest element.  That is summation length,
not the conditioning of a quotient; they stay within the cap of 1 block in 20, the CPU test re-measures each one.

The upper bounds of the recurrent routes (1024 cells, 8192 input floats) are BOUND_SHAPES, a table with a rule of its own: there the
fp32 restatement loses more than TOL32 / 3 in many blocks that are no biases, so EVERY block's GPU bar is max(TOL32, 4 e_cpu) of its
step, and tests/test_blocks_cpu.py holds the shapes to conditions that keep that rule from hiding a failure (no block but a bias of W
above 2 TOL32, at least half of the blocks within TOL32 / 3).

A shape states the kernels it is there for: `rec_route`, the (forward, backward) pair hl_debug_rec_route prints, and `conv_rec_dx`,
what hl_debug_conv_rec_dx(which = 4) returns; both are read off recRoute() (rec.hip) and convRecWideDx (step_exec.h), checked on the
GPU, and a shape that reaches another kernel is changed, never the expectation.  `env`: environment variables set while the HIP
learner of the shape is created and stepped (the CPU restatement does not read them).  `ref`: the shape whose CPU reference this
one shares (the same configuration under another `env`).
"""
import functools

import numpy as np

from smarties_amd import capi
from oracle_api import fill_synth, oracle64_learner, oracle_learner, synth_cfg
from parity import blockdev, coldev, episode_arrays_by_tag, param_blocks, worst_dev
import test_hip_rec_sample_kernels as sample_kernels

TOL32 = 1e-5     # north_star: 1e-5 relative fp32 (tests/test_hip_parity.py), here per block
N_STEPS = 4
PARAM_Q = ("gradSum", "M1", "M2", "W")
TAP_Q = {"O": capi.TAP_OUTPUT, "outGrad": capi.TAP_OUTGRAD, "rho": capi.TAP_RHO, "dkl": capi.TAP_DKL, "deltaQ": capi.TAP_DELTAQ}
INT_TAPS = {"flat": capi.TAP_FLAT, "tag": capi.TAP_TAG, "tstep": capi.TAP_TSTEP, "far": capi.TAP_FAR}
EP_FIELDS = {"V": capi.EP_VALUE, "ADV": capi.EP_ADVANTAGE, "impW": capi.EP_IMPW, "dKL": capi.EP_DKL, "deltaQ": capi.EP_DELTAQ}

_LSTM, _MGU, _RNN = capi.NN_LSTM, capi.NN_MGU, capi.NN_RNN


def _rec(kind, hidden, dS, bptt, batch, **over):
    kw = dict(dimS=dS, dimA=2, bounded=[1, 0], hidden=hidden, nnFunc="Tanh", batchSize=batch, maxTotObsNum=8000, randSeed=5,
              nn_type=kind, adv_kind=capi.ADV_GAUSSIAN, nnBPTTseq=bptt)
    kw.update(over)
    return dict(kw=kw, sc=dict(seed=21, dimS=dS, dimA=kw["dimA"], lenMin=2, lenMax=30, pTerm=0.5), n_eps=60)


# recurrent layers behind convolutions, the geometries of tests/test_hip_conv_rec_wide.py
CONV2 = [(8, 8, 16, 32, 4, 1), (5, 5, 32, 64, 3, 1)]           # 1 + 3 stacked frames of 256 as 16 channels of 8 x 8: a feature row of 576
CONV2_EXTRA = [(8, 8, 12, 32, 4, 1), (5, 5, 32, 64, 3, 1)]     # 1 + 2 stacked frames of 258: 768 for the image, 6 state variables beside it
CONV_1331 = [(13, 13, 2, 11, 3, 1)]                            # 338 = 2 x 13 x 13 -> 11 maps of 11 x 11: 1331 floats, odd, no multiple of 32


def conv_rec_kw(kind, hidden, conv, dS, nApp, batch=12, bptt=4):
    """the configuration of that file's cases: discrete with 5 options, Tanh"""
    return dict(dimS=dS, dimA=1, adv_kind=capi.ADV_DISCRETE, n_options=5, nAppendedObs=nApp, conv=conv, hidden=hidden, nnFunc="Tanh",
                batchSize=batch, maxTotObsNum=2000, randSeed=3, nn_type=kind, nnBPTTseq=bptt)


def _conv_rec(kind, hidden, conv, dS, nApp, dx, **more):
    """... on its replay: episodes of 3 to 12 steps, 50 of them; time-step-major, `dx` the form of the gradient into the feature rows"""
    return dict(kw=conv_rec_kw(kind, hidden, conv, dS, nApp), sc=dict(seed=5, dimS=dS, dimA=1, lenMin=3, lenMax=12, pTerm=0.3), n_eps=50,
                rec_route=TM, conv_rec_dx=(dx, 1), **more)


def _sample(name):
    """a case of tests/test_hip_rec_sample_kernels.py (one kernel instantiation each, there at batch 3) at batch 20 on 40 episodes: a
    column's scale is taken over at least parity.COL_ROWS rows.  recRoute() reads neither, the instantiation is the one stated there"""
    kw, sc = sample_kernels.shape_cfg(name)
    return dict(kw=dict(kw, batchSize=20), sc=sc, n_eps=40, rec_route=tuple(sample_kernels.SHAPES[name][4:6]))


TM = ("launch_rec_tm_forward", "launch_rec_tm_backward")      # rectm.hip: recRoute()'s REC_TM

# name -> kw (make_config), sc (synth_cfg, or its arguments), n_eps, route (launches per eager step of every counter of ROUTE_COUNTERS
# that fires), listed ({(quantity, block): e_cpu measured on the CPU}: the ill-conditioned blocks, see the module's docstring),
# rec_route, conv_rec_dx, env, ref (the module's docstring)
SHAPES = {
    # ---- fused step (fused.hip + dw_table_kernel) ----
    "fused-2x32-b16": dict(
        kw=dict(dimS=5, dimA=2, bounded=[1, 0], hidden=(32, 32), batchSize=16, maxTotObsNum=2000, randSeed=42),
        sc=dict(seed=7, dimS=5, dimA=2, lenMin=5, lenMax=40, pTerm=0.5), n_eps=30),
    "fused-2x16-b5": dict(      # one tile per panel, odd batch, every episode truncated and short: many next-state rows
        kw=dict(dimS=3, dimA=1, bounded=[1], hidden=(16, 16), batchSize=5, maxTotObsNum=500, randSeed=3),
        sc=dict(seed=11, dimS=3, dimA=1, lenMin=3, lenMax=6, pTerm=0.0), n_eps=25),
    "fused-2x64-tanh-b40": dict(      # widest state / action spaces of the kernel, two panels and a partial third
        kw=dict(dimS=32, dimA=7, bounded=[1, 0, 1, 0, 1, 0, 1], hidden=(64, 64), nnFunc="Tanh", batchSize=40, maxTotObsNum=3000, randSeed=12),
        sc=dict(seed=13, dimS=32, dimA=7, lenMin=3, lenMax=9, pTerm=0.0), n_eps=120),
    "fused-2x256-b256": dict(      # the headline instantiation
        kw=dict(dimS=17, dimA=6, hidden=(256, 256), batchSize=256, maxTotObsNum=100000, randSeed=1),
        sc=dict(seed=9, dimS=17, dimA=6, lenMin=150, lenMax=250, pTerm=0.2), n_eps=40),
    # ---- wide variant (fusedw.hip) ----
    "fusedw-257x17-b40": dict(
        kw=dict(dimS=257, dimA=17, bounded=[0] * 17, hidden=(256, 256), batchSize=40, maxTotObsNum=60000, clipImpWeight=(17 / 2.0) ** 0.5, randSeed=33),
        sc=dict(seed=29, dimS=257, dimA=17, lenMin=20, lenMax=120, pTerm=0.5, muSpread=0.2), n_eps=40),
    "fusedw-3x128-b40": dict(      # three equal hidden blocks
        kw=dict(dimS=10, dimA=3, bounded=[1, 0, 0], hidden=(128, 128, 128), nnFunc="Tanh", batchSize=40, maxTotObsNum=50000, randSeed=71),
        sc=dict(seed=23, dimS=10, dimA=3, lenMin=5, lenMax=60, pTerm=0.5), n_eps=60),
    "gauss-2x64-b40": dict(      # RACER with the Gaussian advantage: 13 advantage outputs, 26 in all
        kw=dict(dimS=17, dimA=6, bounded=[1, 0, 1, 0, 1, 1], hidden=(64, 64), batchSize=40, maxTotObsNum=20000, randSeed=41, adv_kind=capi.ADV_GAUSSIAN),
        sc=dict(seed=37, dimS=17, dimA=6, lenMin=20, lenMax=80, pTerm=0.4), n_eps=80),
    "discrete18-2x128-b40": dict(      # RACER with 18 options: 37 outputs
        kw=dict(dimS=24, dimA=1, hidden=(128, 128), batchSize=40, maxTotObsNum=20000, randSeed=43, adv_kind=capi.ADV_DISCRETE, n_options=18),
        sc=dict(seed=39, dimS=24, dimA=1, lenMin=20, lenMax=80, pTerm=0.4), n_eps=80),
    # ---- step chain (gemm16.hip: step_chain_kernel) and the separate launches ----
    "chain-24x16x8-tanh-b8": dict(
        kw=dict(dimS=9, dimA=3, bounded=[0, 0, 0], hidden=(24, 16, 8), nnFunc="Tanh", batchSize=8, maxTotObsNum=1000, randSeed=5, nnLambda=1e-4, learnrate=1e-3),
        sc=dict(seed=3, dimS=9, dimA=3, lenMin=3, lenMax=30, pTerm=0.3), n_eps=20),
    "chain-96x40-relu-b48": dict(
        kw=dict(dimS=33, dimA=17, bounded=[0] * 17, hidden=(96, 40), nnFunc="Relu", batchSize=48, maxTotObsNum=5000, randSeed=8),
        sc=dict(seed=4, dimS=33, dimA=17, lenMin=20, lenMax=80, pTerm=0.1, muSpread=0.2), n_eps=60),
    "generic-1x96-b40": dict(      # a single hidden layer: forward, head and weight-gradient launches of their own, no input gradient
        kw=dict(dimS=10, dimA=3, bounded=[1, 0, 0], hidden=(96,), nnFunc="Tanh", batchSize=40, maxTotObsNum=20000, randSeed=19),
        sc=dict(seed=23, dimS=10, dimA=3, lenMin=5, lenMax=60, pTerm=0.5), n_eps=60),
    "fwdchain-64x288-b40": dict(      # a last layer of 288 units: its input gradient takes the long-reduction kernel, so the chain stops at the forward pass
        kw=dict(dimS=10, dimA=3, bounded=[1, 0, 0], hidden=(64, 288), nnFunc="Tanh", batchSize=40, maxTotObsNum=20000, randSeed=19),
        sc=dict(seed=23, dimS=10, dimA=3, lenMin=5, lenMax=60, pTerm=0.5), n_eps=60),
    "generic-288x64-b40": dict(      # 288 inputs to the second layer: its forward takes the long-reduction kernel, every launch on its own
        kw=dict(dimS=10, dimA=3, bounded=[1, 0, 0], hidden=(288, 64), nnFunc="Tanh", batchSize=40, maxTotObsNum=20000, randSeed=19),
        sc=dict(seed=23, dimS=10, dimA=3, lenMin=5, lenMax=60, pTerm=0.5), n_eps=60),
    # ---- local batch above 1024: big_sample_kernel, and bigmm.hip's forward / dX tiles and row-chunked weight gradients ----
    "bigbatch-2x32-b1040": dict(
        kw=dict(dimS=4, dimA=2, bounded=[1, 0], hidden=(32, 32), nnFunc="Tanh", batchSize=1040, maxTotObsNum=400000, randSeed=29),
        sc=dict(seed=31, dimS=4, dimA=2, lenMin=60, lenMax=160, pTerm=0.5), n_eps=40),
    # ---- recurrent ----
    "lstm-2x32-wave": dict(_rec(_LSTM, (32, 32), 6, 16, 40, dimA=1, bounded=[1], gamma=0.99, nnLambda=1e-6, explNoise=0.1)),
    "lstm-24x24-bptt5": _rec(_LSTM, (24, 24), 6, 5, 20, adv_kind=capi.ADV_ZERO),
    "mgu-48x32": _rec(_MGU, (48, 32), 7, 10, 24, adv_kind=capi.ADV_ZERO, bounded=[0, 1]),
    "rnn-24x16": _rec(_RNN, (24, 16), 6, 6, 20),
    "lstm-64x64-tm": _rec(_LSTM, (64, 64), 6, 4, 20),      # narrowest layers the time-step-major launches take: LSTM above 48 cells,
    "mgu-80x80-tm": _rec(_MGU, (80, 80), 6, 4, 20),        # MGU above 64,
    "rnn-272-tm": _rec(_RNN, (272,), 7, 3, 20),            # RNN above the 256 cells of the per-sample kernels
    "lstm-32x16-wide-in": _rec(_LSTM, (32, 16), 257, 3, 20),      # a state above 256 components: the first layer's input product on the MFMA
    "rnn-encoder-mgu": _rec(_MGU, (16, 16), 5, 5, 20, encoder=[24], encoder_rnn=1),      # two segments: an RNN encoder layer under MGU layers
    # ---- preprocessing ----
    "conv-small": dict(      # the geometry of tests/golden/conv_small.bin: 4 stacked frames of 256 as 16 channels of 8 x 8
        kw=dict(dimS=256, dimA=1, bounded=[1], nAppendedObs=3, conv=[(8, 8, 16, 32, 4, 1), (5, 5, 32, 64, 3, 1)], hidden=(64,), batchSize=20,
                maxTotObsNum=2000, randSeed=7),
        sc=dict(seed=7, dimS=256, dimA=1, lenMin=6, lenMax=40, pTerm=0.5), n_eps=30),
    "appended-2x32-b20": dict(      # tests/golden/appended_dense.bin: two appended observations in front of dense layers
        kw=dict(dimS=6, dimA=2, bounded=[1, 0], nAppendedObs=2, hidden=(32, 32), batchSize=20, maxTotObsNum=2000, randSeed=7),
        sc=dict(seed=7, dimS=6, dimA=2, lenMin=4, lenMax=25, pTerm=0.5), n_eps=30),
    "encoder-24-16x16-b20": dict(      # tests/golden/encoder_dense.bin: an encoder layer under the hidden layers
        kw=dict(dimS=5, dimA=2, bounded=[1, 0], encoder=[24], hidden=(16, 16), batchSize=20, maxTotObsNum=2000, randSeed=7),
        sc=dict(seed=7, dimS=5, dimA=2, lenMin=5, lenMax=40, pTerm=0.5), n_eps=30),
    # ---- convolutional routes beside conv-small's: batches are the smallest that still fill a tile edge ----
    "conv-atari-18opt-b8": dict(      # RACER_atari's stack: the first layer's row-block kernels with the geometry at compile time, windows
        # read from the replay; layers 1 to 3 in one launch (convt.hip).  18 options: an ALE action count (and 133 blocks, 5 of them listed)
        kw=dict(dimS=7056, dimA=1, adv_kind=capi.ADV_DISCRETE, n_options=18, nAppendedObs=3,
                conv=[(84, 84, 4, 8, 8, 4), (20, 20, 8, 16, 6, 2), (8, 8, 16, 32, 4, 1), (5, 5, 32, 64, 3, 1)], hidden=(512,), nnFunc="Tanh",
                batchSize=8, maxTotObsNum=600, randSeed=4),
        sc=dict(seed=8, dimS=7056, dimA=1, lenMin=4, lenMax=12, pTerm=0.5), n_eps=14),
    "conv-rows-32x32-b8": dict(      # the smallest first layer the any-geometry row-block kernels take (4 x 8 x 8 patches, 4096 inputs), from the replay
        kw=dict(dimS=1024, dimA=2, bounded=[1, 0], nAppendedObs=3, conv=[(32, 32, 4, 8, 8, 4), (7, 7, 8, 16, 3, 1)], hidden=(32,), nnFunc="Tanh",
                batchSize=8, maxTotObsNum=1500, randSeed=13),
        sc=dict(seed=15, dimS=1024, dimA=2, lenMin=4, lenMax=20, pTerm=0.5), n_eps=30),
    "conv-rows-stacked-extras3-b8": dict(      # the same layer on stacked rows: three state variables beside the image keep it off the replay
        kw=dict(dimS=4099, dimA=2, bounded=[1, 0], nAppendedObs=0, conv=[(32, 32, 4, 8, 8, 4), (7, 7, 8, 16, 3, 1)], hidden=(32,), nnFunc="Tanh",
                batchSize=8, maxTotObsNum=1500, randSeed=13),
        sc=dict(seed=15, dimS=4099, dimA=2, lenMin=4, lenMax=20, pTerm=0.5), n_eps=30),
    "conv-rows-single-b8": dict(      # that layer alone: no other filter-gradient block, so its filter gradient is a launch of its own
        kw=dict(dimS=1024, dimA=2, bounded=[1, 0], nAppendedObs=3, conv=[(32, 32, 4, 8, 8, 4)], hidden=(32,), nnFunc="Tanh",
                batchSize=8, maxTotObsNum=1500, randSeed=13),
        sc=dict(seed=15, dimS=1024, dimA=2, lenMin=4, lenMax=20, pTerm=0.5), n_eps=30),
    "conv-perlayer-strided-b10": dict(      # 12 channels: conv_tail_plan declines, the input gradient is a launch per layer (strided form)
        kw=dict(dimS=576, dimA=2, nAppendedObs=0, conv=[(12, 12, 4, 8, 3, 1), (10, 10, 8, 12, 4, 2)], hidden=(32,), nnFunc="Tanh",
                batchSize=10, maxTotObsNum=1500, randSeed=17),
        sc=dict(seed=19, dimS=576, dimA=2, lenMin=4, lenMax=20, pTerm=0.5), n_eps=30),
    "conv-perlayer-unstrided-b10": dict(      # ... and the unstrided form
        kw=dict(dimS=576, dimA=2, nAppendedObs=0, conv=[(12, 12, 4, 8, 3, 1), (10, 10, 8, 12, 4, 1)], hidden=(32,), nnFunc="Tanh",
                batchSize=10, maxTotObsNum=1500, randSeed=17),
        sc=dict(seed=19, dimS=576, dimA=2, lenMin=4, lenMax=20, pTerm=0.5), n_eps=30),
    "conv-extras6-b24": dict(      # the "6-extras" case of tests/test_hip_a22.py: six state variables beside the image
        kw=dict(dimS=1030, dimA=1, adv_kind=capi.ADV_DISCRETE, n_options=5, conv=[(8, 8, 16, 32, 4, 1), (5, 5, 32, 64, 3, 1)],
                hidden=(48,), nnFunc="Tanh", batchSize=24, maxTotObsNum=2000, randSeed=3),
        sc=dict(seed=5, dimS=1030, dimA=1, lenMin=3, lenMax=9, pTerm=0.3), n_eps=60),
    "conv-lstm32-bptt4": dict(      # convolutions under a recurrent layer: every window row passes through the conv stack
        kw=dict(dimS=256, dimA=1, adv_kind=capi.ADV_DISCRETE, n_options=5, nAppendedObs=3, conv=[(8, 8, 16, 32, 4, 1), (5, 5, 32, 64, 3, 1)],
                hidden=(32,), nnFunc="Tanh", batchSize=12, maxTotObsNum=2000, randSeed=3, nn_type=_LSTM, nnBPTTseq=4),
        sc=dict(seed=5, dimS=256, dimA=1, lenMin=3, lenMax=12, pTerm=0.3), n_eps=50),
    # ---- the prioritised samplers inside a training step ----
    "per-rank-2x32-b16": dict(
        kw=dict(dimS=5, dimA=2, bounded=[1, 0], hidden=(32, 32), batchSize=16, maxTotObsNum=2000, randSeed=42, dataSamplingAlgo="PERrank"),
        sc=dict(seed=7, dimS=5, dimA=2, lenMin=5, lenMax=40, pTerm=0.5), n_eps=30),
    "per-seq-2x32-b16": dict(
        kw=dict(dimS=5, dimA=2, bounded=[1, 0], hidden=(32, 32), batchSize=16, maxTotObsNum=2000, randSeed=42, dataSamplingAlgo="PERseq"),
        sc=dict(seed=7, dimS=5, dimA=2, lenMin=5, lenMax=40, pTerm=0.5), n_eps=30),
    "per-err-lstm24": _rec(_LSTM, (24,), 6, 5, 20, dataSamplingAlgo="PERerr"),
    # ---- a recurrent net's weight gradients over at least 1024 window rows: one launch ----
    "lstm-2x32-bptt16-b64": _rec(_LSTM, (32, 32), 6, 16, 64),      # 64 x 17 = 1088 window rows
    # ---- the time-step-major launches (rectm.hip) beyond their narrowest sizes: the smallest shapes at which each kernel can go wrong ----
    # one tile past 256 cells; 4 x 272 = 1088 gate columns end in a ragged 64-column tile; fewer than 16 samples
    "lstm-272-tm": dict(_rec(_LSTM, (272,), 6, 3, 12), rec_route=TM),
    "mgu-272x48-tm": dict(_rec(_MGU, (272, 48), 6, 3, 12), rec_route=TM),      # both MGU phases; a narrow layer over a wide one
    # appended observations in front of the window; a parametric residual between wide layers
    "lstm-320x272-app2-tm": dict(_rec(_LSTM, (320, 272), 9, 4, 12, nAppendedObs=2), rec_route=TM),
    # three layers: the middle layer's deltas have both producers on one backward diagonal; a derivative that is not tanh's; 20 samples: a
    # partial second block of 16
    "rnn-272x96x80-softsign-tm": dict(_rec(_RNN, (272, 96, 80), 6, 5, 20, nnFunc="SoftSign"), rec_route=TM),
    # ---- ... on wide inputs: the first layer's input product (tm_win_product_kernel) in front of the tm_win_* chains ----
    # tm_win_mgu_fwd_kernel; 5 x 300 input floats, windows that begin before the episode's start; 16-byte loads
    "mgu-64x32-wide-in-app4": dict(_rec(_MGU, (64, 32), 300, 4, 20, nAppendedObs=4), rec_route=TM),
    "rnn-272-wide-in-1027": dict(_rec(_RNN, (272,), 1027, 3, 6), rec_route=TM),      # tm_win_rnn_fwd_kernel; an odd reduction length; 17 cell tiles
    "lstm-16-wide-in-2048": dict(_rec(_LSTM, (16,), 2048, 2, 20), rec_route=TM),     # the product over many K chunks in front of the narrowest layer
    "mgu-1024x1024-tm": dict(_rec(_MGU, (1024, 1024), 5, 2, 4), rec_route=TM),       # the cell bound, still under the ordinary rule
    # ---- ... behind convolutions: the prepare launch joins the feature rows, the product, the gradient into the rows in both forms ----
    # 288 cells: 18 tiles, 1152 gate columns are 18 x 64 (272 cells at this batch put 10 of 93 blocks over TOL32 / 3 on the CPU: over the cap);
    # 576 inputs: the GEMM_X problem
    "conv-lstm288-b12": _conv_rec(_LSTM, (288,), CONV2, 256, 3, 0),
    # the same net with tm_conv_dx_kernel asked for (convRecWideDx: bit 2048): same CPU reference
    "conv-lstm288-b12-dxkernel": _conv_rec(_LSTM, (288,), CONV2, 256, 3, 1, env={"SMARTIES_HIP_GENERIC": "2048"}, ref="conv-lstm288-b12"),
    "conv-mgu272x48-bptt4": _conv_rec(_MGU, (272, 48), CONV2, 256, 3, 0),      # both MGU phases behind convolutions
    # six state variables beside the image through the join (582 inputs); the ragged product tile behind convolutions
    "conv-lstm272x32-extras6": _conv_rec(_LSTM, (272, 32), CONV2_EXTRA, 258, 2, 0),
    # a feature row of 1331 (odd: the product's scalar tail, a last slice of 19 columns); above 1024 inputs tm_conv_dx_kernel, 21 input
    # tiles, the last of 51 columns
    "conv1331-lstm32": _conv_rec(_LSTM, (32,), CONV_1331, 338, 0, 1),
    "conv1331-mgu48x16": _conv_rec(_MGU, (48, 16), CONV_1331, 338, 0, 1),
}
# ---- the workgroup-per-sample kernels (rec.hip), one shape per instantiation ----
SHAPES.update({"sample-" + _n: _sample(_n) for _n in sample_kernels.SHAPES})
# ---- the stand-alone wave kernels of two 32-cell layers: the one-launch step serves these nets unless SMARTIES_HIP_GENERIC bit 4 asks for
# the three-launch form (tests/test_hip_r4.py); recRoute() answers REC_WAVE32 either way ----
_WAVE = dict(dimA=1, bounded=[1], gamma=0.99, nnLambda=1e-6, explNoise=0.1)
SHAPES["lstm-2x32-wave-3launch"] = dict(_rec(_LSTM, (32, 32), 6, 16, 40, **_WAVE), env={"SMARTIES_HIP_GENERIC": "4"}, ref="lstm-2x32-wave",
                                        rec_route=("lstm32_forward_wave_kernel", "lstm32_backward_wave_kernel"))
SHAPES["mgu-2x32-wave-3launch"] = dict(_rec(_MGU, (32, 32), 6, 16, 40, **_WAVE), env={"SMARTIES_HIP_GENERIC": "4"},
                                       rec_route=("mgu32_forward_wave_kernel", "mgu32_backward_wave_kernel"))

# what recRoute() gives the recurrent shapes from before the table stated it: LSTM layers of up to 64 cells on the step's own state take
# the kernels with their own LDS layouts (24 cells: not the 32-cell form), two MGU layers whose weights fit the LDS NL = 2, ...
for _n, _r in {"lstm-24x24-bptt5": ("lstm_forward_lds_kernel<2, 0>", "lstm_backward_lds_kernel<2>"),
               "mgu-48x32": ("mgu_forward_kernel<true, 2>", "mgu_backward_kernel<true, 2>"),
               "rnn-24x16": ("rnn_forward_kernel<true>", "rnn_backward_kernel<true>"),
               # ... and hl_create sends LSTM above 48 cells, MGU above 64, RNN above 256 and every wide input to rectm.hip
               "lstm-64x64-tm": TM, "mgu-80x80-tm": TM, "rnn-272-tm": TM, "lstm-32x16-wide-in": TM}.items():
    SHAPES[_n]["rec_route"] = _r

# The upper bounds: 1024 cells, 8192 input floats.  Judged under the rule of their own the module's docstring states
BOUND_SHAPES = {
    "bound-lstm-1024": dict(_rec(_LSTM, (1024,), 5, 2, 4), rec_route=TM),
    "bound-rnn-1024x1024": dict(_rec(_RNN, (1024, 1024), 5, 2, 16), rec_route=TM),
    "bound-lstm-16-in8192": dict(_rec(_LSTM, (16,), 8192, 2, 4), rec_route=TM),
}


def shape(name):
    return SHAPES[name] if name in SHAPES else BOUND_SHAPES[name]

# every counter hl_timing_get knows for a launch of the training step (smarties_amd/csrc/step_exec.h)
ROUTE_COUNTERS = (["step_tail_kernel", "big_sample_ahead", "per_prepare", "stack_gather", "window_rows", "extras_copy",
                   "fused_fwd_head_dx", "fused_wide", "step_chain", "fwd_chain", "head_kernel", "panel_head",
                   "dw_table_kernel", "gemm16_dw", "big_dw", "dw_wide", "dw_direct", "splitk_reduce", "adam_kernel", "post_kernel", "post_agg_chunks",
                   "rec_prepare", "rec_in_product", "rec_forward", "rec_backward", "rec_step_fused", "rec_forward_lower", "rec_backward_lower", "gemm16_dx_segment",
                   "conv_back", "conv_dw_dense", "conv_dw_all", "conv_dw_rows", "conv_dw", "conv_reduce_adam", "conv_fwd_tail", "conv_prep",
                   "moments_kernel", "xchg_allreduce"]
                  + ["gemm16_fwd%d" % j for j in range(8)] + ["gemm16_dx%d" % j for j in range(8)]
                  + ["conv_fwd%d" % j for j in range(8)] + ["conv_dx%d" % j for j in range(8)])


# the ill-conditioned blocks: worst e_cpu over the N_STEPS steps as measured on the CPU (tests/test_blocks_cpu.py re-measures them)
LISTED = {
    "fused-2x64-tanh-b40": {("W", "L2.dense.B"): 6.4e-06},
    "fused-2x256-b256": {("W", "L1.dense.B"): 1.6e-05, ("W", "L3.res.B"): 1.6e-04},
    "fusedw-257x17-b40": {("W", "L1.dense.B"): 5.8e-06, ("W", "L2.dense.B"): 4.4e-05},
    "fusedw-3x128-b40": {("W", "L1.dense.B"): 2.3e-05, ("W", "L2.dense.B"): 8.7e-06, ("W", "L4.dense.B"): 8.9e-06},
    "discrete18-2x128-b40": {("W", "L2.dense.B"): 1.4e-05},
    "fwdchain-64x288-b40": {("W", "L2.dense.B"): 5.6e-06},
    "bigbatch-2x32-b1040": {("W", "L3.res.B"): 1.2e-05},
    "mgu-48x32": {("W", "L3.res.B"): 3.9e-06},
    "rnn-24x16": {("W", "L1.rnn.B"): 1.1e-05},
    "mgu-80x80-tm": {("W", "L3.res.B"): 5.3e-06},
    "rnn-272-tm": {("W", "L1.rnn.B"): 3.9e-04},
    "conv-small": {("W", "L1.conv.B"): 8.8e-05, ("W", "L2.conv.B"): 6.4e-05},
    "conv-atari-18opt-b8": {("W", "L1.conv.B"): 2.9e-05, ("W", "L2.conv.B"): 4.0e-05, ("W", "L3.conv.B"): 1.7e-05, ("W", "L4.conv.B"): 1.4e-05,
                            ("W", "L6.res.B"): 1.1e-05},
    "conv-rows-32x32-b8": {("W", "L1.conv.B"): 2.4e-04, ("W", "L2.conv.B"): 4.9e-06},
    "conv-rows-stacked-extras3-b8": {("W", "L1.conv.B"): 2.9e-05, ("W", "L2.conv.B"): 2.7e-05},
    "conv-rows-single-b8": {("W", "L1.conv.B"): 9.6e-05},
    "conv-perlayer-strided-b10": {("W", "L1.conv.B"): 3.1e-05, ("W", "L2.conv.B"): 3.8e-05},
    "conv-perlayer-unstrided-b10": {("W", "L1.conv.B"): 1.7e-05, ("W", "L2.conv.B"): 2.0e-04},
    "conv-extras6-b24": {("W", "L1.conv.B"): 1.2e-05, ("W", "L2.conv.B"): 2.7e-05, ("W", "L5.dense.B"): 2.3e-05},
    "conv-lstm32-bptt4": {("W", "L1.conv.B"): 1.8e-05, ("W", "L2.conv.B"): 1.3e-05},
    "rnn-272x96x80-softsign-tm": {("W", "L1.rnn.B"): 1.9e-05, ("W", "L2.rnn.B"): 3.5e-06, ("W", "L3.res.B"): 5.4e-06, ("W", "L4.rnn.B"): 2.0e-05},
    # (the entries below that are no bias blocks of W: sums of 1000 to 2000 terms under a small batch, the module's docstring)
    "mgu-64x32-wide-in-app4": {("W", "L1.mgu.Wx.state"): 3.6e-06},
    "rnn-272-wide-in-1027": {("W", "L1.rnn.B"): 8.5e-05},
    "lstm-16-wide-in-2048": {("M1", "L1.lstm.Wr.forget"): 3.5e-06, ("M2", "L1.lstm.Wx.forget"): 3.6e-06, ("M2", "L1.lstm.Wr.forget"): 4.6e-06},
    "mgu-1024x1024-tm": {("M2", "L2.mgu.Wr.forget"): 3.6e-06, ("W", "L3.res.B"): 3.4e-06, ("O", "c0"): 6.3e-06},
    "conv-lstm288-b12": {("W", "L1.conv.B"): 3.3e-05, ("W", "L2.conv.B"): 4.2e-05, ("W", "L4.res.B"): 6.3e-06, ("W", "L5.out.W"): 4.4e-06},
    "conv-lstm288-b12-dxkernel": {("W", "L1.conv.B"): 3.3e-05, ("W", "L2.conv.B"): 4.2e-05, ("W", "L4.res.B"): 6.3e-06, ("W", "L5.out.W"): 4.4e-06},
    "conv-mgu272x48-bptt4": {("W", "L1.conv.B"): 2.4e-05, ("W", "L2.conv.B"): 8.7e-06, ("W", "L4.res.B"): 7.5e-06},
    "conv-lstm272x32-extras6": {("M2", "L5.lstm.Wr.out"): 4.3e-06, ("W", "L1.conv.B"): 1.7e-05, ("W", "L2.conv.B"): 2.3e-05, ("W", "L6.res.B"): 2.8e-05},
    "conv1331-lstm32": {("M2", "L2.lstm.Wr.out"): 3.9e-06, ("W", "L1.conv.B"): 2.1e-05},
    "conv1331-mgu48x16": {("W", "L1.conv.B"): 2.9e-05},
    # (the per-sample cases: windows of at most 3 steps, so a bias block's gradient is a sum of 20 to 60 deltas of either sign and its
    #  largest element small against them where they cancel -- the gradient sum and the moments of such a block, no quotient involved)
    "sample-rnn-160-l2": {("W", "L1.rnn.B"): 6.0e-05},
    "sample-mgu-8-8-8": {("gradSum", "L5.res.B"): 5.3e-06},
    "sample-mgu-8-app1": {("gradSum", "L2.out.B"): 5.1e-06},
    "sample-lstm-32-32-in33": {("M1", "L5.sigma.B"): 1.6e-05},
    "sample-lstm-8-no-preload": {("gradSum", "L3.sigma.B"): 5.9e-06, ("M1", "L3.sigma.B"): 5.9e-06, ("M2", "L3.sigma.B"): 1.2e-05},
    "sample-lstm-72-72-l2": {("M2", "L2.lstm.B"): 5.9e-06},
}
for _n, _l in LISTED.items():
    shape(_n)["listed"] = _l


# launches per eager step of every counter that fires, as the MI355X takes these shapes (hl_timing_get)
ROUTES = {
    "fused-2x32-b16": {'step_tail_kernel': 1, 'fused_fwd_head_dx': 1, 'dw_table_kernel': 1, 'post_kernel': 1},
    "fused-2x16-b5": {'step_tail_kernel': 1, 'fused_fwd_head_dx': 1, 'dw_table_kernel': 1, 'post_kernel': 1},
    "fused-2x64-tanh-b40": {'step_tail_kernel': 1, 'fused_fwd_head_dx': 1, 'dw_table_kernel': 1, 'post_kernel': 1},
    "fused-2x256-b256": {'step_tail_kernel': 1, 'fused_fwd_head_dx': 1, 'dw_table_kernel': 1, 'post_kernel': 1},
    "fusedw-257x17-b40": {'step_tail_kernel': 1, 'fused_wide': 1, 'dw_table_kernel': 1, 'post_kernel': 1},
    "fusedw-3x128-b40": {'step_tail_kernel': 1, 'fused_wide': 1, 'gemm16_dw': 1, 'post_kernel': 1},
    "gauss-2x64-b40": {'step_tail_kernel': 1, 'fused_wide': 1, 'dw_table_kernel': 1, 'post_kernel': 1},
    "discrete18-2x128-b40": {'step_tail_kernel': 1, 'fused_wide': 1, 'dw_table_kernel': 1, 'post_kernel': 1},
    "chain-24x16x8-tanh-b8": {'step_tail_kernel': 1, 'step_chain': 1, 'gemm16_dw': 1, 'post_kernel': 1},
    "chain-96x40-relu-b48": {'step_tail_kernel': 1, 'step_chain': 1, 'gemm16_dw': 1, 'post_kernel': 1},
    "generic-1x96-b40": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'gemm16_fwd0': 1},
    "bigbatch-2x32-b1040": {'step_tail_kernel': 1, 'big_sample_ahead': 1, 'stack_gather': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'big_dw': 1, 'splitk_reduce': 1, 'post_kernel': 1, 'post_agg_chunks': 1, 'gemm16_fwd0': 1, 'gemm16_fwd1': 1, 'gemm16_dx1': 1},
    "lstm-2x32-wave": {'step_tail_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_step_fused': 1},
    "lstm-24x24-bptt5": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "mgu-48x32": {'step_tail_kernel': 1, 'panel_head': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "rnn-24x16": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "lstm-64x64-tm": {'step_tail_kernel': 1, 'panel_head': 1, 'gemm16_dw': 1, 'big_dw': 1, 'splitk_reduce': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "mgu-80x80-tm": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'big_dw': 1, 'splitk_reduce': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "rnn-272-tm": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'big_dw': 1, 'splitk_reduce': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "lstm-32x16-wide-in": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'big_dw': 1, 'splitk_reduce': 1, 'post_kernel': 1, 'rec_prepare': 1, 'rec_in_product': 1, 'rec_forward': 1, 'rec_backward': 1},
    "conv-small": {'step_tail_kernel': 1, 'stack_gather': 1, 'head_kernel': 1, 'dw_direct': 1, 'post_kernel': 1, 'conv_back': 1, 'conv_dw': 1, 'conv_reduce_adam': 1, 'gemm16_fwd1': 1, 'gemm16_dx1': 1, 'conv_fwd0': 1, 'conv_fwd1': 1},
    "appended-2x32-b20": {'step_tail_kernel': 1, 'stack_gather': 1, 'step_chain': 1, 'gemm16_dw': 1, 'post_kernel': 1},
    "encoder-24-16x16-b20": {'step_tail_kernel': 1, 'step_chain': 1, 'gemm16_dw': 1, 'post_kernel': 1},
    "fwdchain-64x288-b40": {'step_tail_kernel': 1, 'fwd_chain': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'gemm16_dx1': 1},
    "generic-288x64-b40": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'gemm16_fwd0': 1, 'gemm16_fwd1': 1, 'gemm16_dx1': 1},
    "rnn-encoder-mgu": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1, 'rec_forward_lower': 1, 'rec_backward_lower': 1, 'gemm16_dx_segment': 1},
    # (conv_dw_dense, not conv_dw_all: the 3136 x 512 dense layer alone is 196 x 32 weight-gradient tiles of 16 x 16, above the 128 from which
    #  the dense layers' tiles join the filter-gradient launch -- launchBackward: denseMerged -- so the step has no weight-gradient launch of its own)
    "conv-atari-18opt-b8": {'step_tail_kernel': 1, 'head_kernel': 1, 'post_kernel': 1, 'conv_back': 1, 'conv_dw_dense': 1, 'conv_reduce_adam': 1, 'conv_fwd_tail': 1, 'gemm16_fwd1': 1, 'gemm16_dx1': 1, 'conv_fwd0': 1},
    # (conv_dw_all: a 400 x 32 dense layer is 25 x 2 tiles, the net stays below 128: the dense layers keep their launch, gemm16_dw)
    "conv-rows-32x32-b8": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'conv_back': 1, 'conv_dw_all': 1, 'conv_reduce_adam': 1, 'gemm16_fwd1': 1, 'gemm16_dx1': 1, 'conv_fwd0': 1, 'conv_fwd1': 1},
    "conv-rows-stacked-extras3-b8": {'step_tail_kernel': 1, 'stack_gather': 1, 'extras_copy': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'conv_back': 1, 'conv_dw_all': 1, 'conv_reduce_adam': 1, 'gemm16_fwd1': 1, 'gemm16_dx1': 1, 'conv_fwd0': 1, 'conv_fwd1': 1},
    "conv-rows-single-b8": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'conv_dw_rows': 1, 'conv_reduce_adam': 1, 'gemm16_fwd1': 1, 'gemm16_dx1': 1, 'conv_fwd0': 1},
    "conv-perlayer-strided-b10": {'step_tail_kernel': 1, 'stack_gather': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'conv_dw': 1, 'conv_reduce_adam': 1, 'gemm16_fwd1': 1, 'gemm16_dx1': 1, 'conv_fwd0': 1, 'conv_fwd1': 1, 'conv_dx1': 1},
    "conv-perlayer-unstrided-b10": {'step_tail_kernel': 1, 'stack_gather': 1, 'head_kernel': 1, 'dw_direct': 1, 'post_kernel': 1, 'conv_dw': 1, 'conv_reduce_adam': 1, 'gemm16_fwd1': 1, 'gemm16_dx1': 1, 'conv_fwd0': 1, 'conv_fwd1': 1, 'conv_dx1': 1},
    "conv-extras6-b24": {'step_tail_kernel': 1, 'stack_gather': 1, 'extras_copy': 1, 'head_kernel': 1, 'dw_direct': 1, 'post_kernel': 1, 'conv_back': 1, 'conv_dw': 1, 'conv_reduce_adam': 1, 'gemm16_fwd1': 1, 'gemm16_dx1': 1, 'conv_fwd0': 1, 'conv_fwd1': 1},
    "conv-lstm32-bptt4": {'step_tail_kernel': 1, 'stack_gather': 1, 'window_rows': 1, 'panel_head': 1, 'dw_direct': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1, 'conv_back': 1, 'conv_dw': 1, 'conv_reduce_adam': 1, 'gemm16_dx1': 1, 'conv_fwd0': 1, 'conv_fwd1': 1},
    "per-rank-2x32-b16": {'step_tail_kernel': 1, 'per_prepare': 1, 'fused_fwd_head_dx': 1, 'dw_table_kernel': 1, 'post_kernel': 1},
    "per-seq-2x32-b16": {'step_tail_kernel': 1, 'per_prepare': 1, 'fused_fwd_head_dx': 1, 'dw_table_kernel': 1, 'post_kernel': 1},
    "per-err-lstm24": {'step_tail_kernel': 1, 'per_prepare': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "lstm-2x32-bptt16-b64": {'step_tail_kernel': 1, 'dw_wide': 1, 'post_kernel': 1, 'rec_step_fused': 1},
    "lstm-272-tm": {'step_tail_kernel': 1, 'head_kernel': 1, 'dw_direct': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "mgu-272x48-tm": {'step_tail_kernel': 1, 'head_kernel': 1, 'dw_direct': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "lstm-320x272-app2-tm": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'big_dw': 1, 'splitk_reduce': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "rnn-272x96x80-softsign-tm": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'big_dw': 1, 'splitk_reduce': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "mgu-64x32-wide-in-app4": {'step_tail_kernel': 1, 'panel_head': 1, 'gemm16_dw': 1, 'big_dw': 1, 'splitk_reduce': 1, 'post_kernel': 1, 'rec_prepare': 1, 'rec_in_product': 1, 'rec_forward': 1, 'rec_backward': 1},
    "rnn-272-wide-in-1027": {'step_tail_kernel': 1, 'head_kernel': 1, 'dw_direct': 1, 'post_kernel': 1, 'rec_prepare': 1, 'rec_in_product': 1, 'rec_forward': 1, 'rec_backward': 1},
    "lstm-16-wide-in-2048": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'big_dw': 1, 'splitk_reduce': 1, 'post_kernel': 1, 'rec_prepare': 1, 'rec_in_product': 1, 'rec_forward': 1, 'rec_backward': 1},
    "mgu-1024x1024-tm": {'step_tail_kernel': 1, 'head_kernel': 1, 'dw_direct': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "conv-lstm288-b12": {'step_tail_kernel': 1, 'stack_gather': 1, 'window_rows': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'big_dw': 1, 'splitk_reduce': 1, 'post_kernel': 1, 'rec_prepare': 1, 'rec_in_product': 1, 'rec_forward': 1, 'rec_backward': 1, 'conv_back': 1, 'conv_dw': 1, 'conv_reduce_adam': 1, 'gemm16_dx1': 1, 'conv_fwd0': 1, 'conv_fwd1': 1},
    "conv-lstm288-b12-dxkernel": {'step_tail_kernel': 1, 'stack_gather': 1, 'window_rows': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'big_dw': 1, 'splitk_reduce': 1, 'post_kernel': 1, 'rec_prepare': 1, 'rec_in_product': 1, 'rec_forward': 1, 'rec_backward': 1, 'conv_back': 1, 'conv_dw': 1, 'conv_reduce_adam': 1, 'gemm16_dx1': 1, 'conv_fwd0': 1, 'conv_fwd1': 1},
    "conv-mgu272x48-bptt4": {'step_tail_kernel': 1, 'stack_gather': 1, 'window_rows': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'big_dw': 1, 'splitk_reduce': 1, 'post_kernel': 1, 'rec_prepare': 1, 'rec_in_product': 1, 'rec_forward': 1, 'rec_backward': 1, 'conv_back': 1, 'conv_dw': 1, 'conv_reduce_adam': 1, 'gemm16_dx2': 1, 'conv_fwd0': 1, 'conv_fwd1': 1},
    "conv-lstm272x32-extras6": {'step_tail_kernel': 1, 'stack_gather': 1, 'window_rows': 1, 'extras_copy': 1, 'panel_head': 1, 'gemm16_dw': 1, 'big_dw': 1, 'splitk_reduce': 1, 'post_kernel': 1, 'rec_prepare': 1, 'rec_in_product': 1, 'rec_forward': 1, 'rec_backward': 1, 'conv_back': 1, 'conv_dw': 1, 'conv_reduce_adam': 1, 'gemm16_dx2': 1, 'conv_fwd0': 1, 'conv_fwd1': 1},
    "conv1331-lstm32": {'step_tail_kernel': 1, 'stack_gather': 1, 'window_rows': 1, 'panel_head': 1, 'gemm16_dw': 1, 'big_dw': 1, 'splitk_reduce': 1, 'post_kernel': 1, 'rec_prepare': 1, 'rec_in_product': 1, 'rec_forward': 1, 'rec_backward': 1, 'conv_dw': 1, 'conv_reduce_adam': 1, 'gemm16_dx1': 1, 'conv_fwd0': 1},
    "conv1331-mgu48x16": {'step_tail_kernel': 1, 'stack_gather': 1, 'window_rows': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'big_dw': 1, 'splitk_reduce': 1, 'post_kernel': 1, 'rec_prepare': 1, 'rec_in_product': 1, 'rec_forward': 1, 'rec_backward': 1, 'conv_dw': 1, 'conv_reduce_adam': 1, 'gemm16_dx2': 1, 'conv_fwd0': 1},
    "sample-rnn-20": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "sample-rnn-160-l2": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "sample-mgu-8": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "sample-mgu-12-8": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "sample-mgu-8-8-8": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "sample-mgu-8-app1": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "sample-mgu-100-100-l2": {'step_tail_kernel': 1, 'head_kernel': 1, 'dw_direct': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "sample-lstm-8": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "sample-lstm-12-8": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "sample-lstm-8-8-8": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "sample-lstm-8-8-8-8": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "sample-lstm-32-32-in33": {'step_tail_kernel': 1, 'panel_head': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "sample-lstm-8-no-preload": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "sample-lstm-8-app1": {'step_tail_kernel': 1, 'head_kernel': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "sample-lstm-72-72-l2": {'step_tail_kernel': 1, 'head_kernel': 1, 'dw_direct': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "lstm-2x32-wave-3launch": {'step_tail_kernel': 1, 'panel_head': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "mgu-2x32-wave-3launch": {'step_tail_kernel': 1, 'panel_head': 1, 'gemm16_dw': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "bound-lstm-1024": {'step_tail_kernel': 1, 'head_kernel': 1, 'dw_direct': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "bound-rnn-1024x1024": {'step_tail_kernel': 1, 'head_kernel': 1, 'dw_direct': 1, 'post_kernel': 1, 'rec_forward': 1, 'rec_backward': 1},
    "bound-lstm-16-in8192": {'step_tail_kernel': 1, 'head_kernel': 1, 'dw_direct': 1, 'post_kernel': 1, 'rec_prepare': 1, 'rec_in_product': 1, 'rec_forward': 1, 'rec_backward': 1},
}

# the counters a shape is there for: (those that must fire, those that must not).  A shape whose recorded route lacks one is changed
# until it fires, never the expectation (tests/test_blocks_cpu.py)
REQUIRED = {
    "conv-atari-18opt-b8": (["conv_fwd0", "conv_fwd_tail", "conv_back", "conv_dw_dense"], ["stack_gather"]),
    "conv-rows-32x32-b8": (["conv_fwd0", "conv_dw_all"], ["stack_gather"]),
    "conv-rows-stacked-extras3-b8": (["stack_gather", "extras_copy", "conv_dw_all"], []),
    "conv-rows-single-b8": (["conv_fwd0", "conv_dw_rows"], ["stack_gather", "conv_dw"]),
    "conv-perlayer-strided-b10": (["conv_dx1", "conv_dw"], ["conv_back"]),
    "conv-perlayer-unstrided-b10": (["conv_dx1", "conv_dw"], ["conv_back"]),
    "conv-extras6-b24": (["extras_copy"], []),
    "conv-lstm32-bptt4": (["window_rows", "rec_forward", "rec_backward"], []),
    "per-rank-2x32-b16": (["per_prepare"], []),
    "per-seq-2x32-b16": (["per_prepare"], []),
    "per-err-lstm24": (["per_prepare"], []),
    "lstm-2x32-bptt16-b64": (["dw_wide"], []),
    # wide inputs: the prepare launch and the input product in front of the chain
    "mgu-64x32-wide-in-app4": (["rec_prepare", "rec_in_product", "rec_forward", "rec_backward"], []),
    "rnn-272-wide-in-1027": (["rec_prepare", "rec_in_product", "rec_forward", "rec_backward"], []),
    "lstm-16-wide-in-2048": (["rec_prepare", "rec_in_product", "rec_forward", "rec_backward"], []),
    "bound-lstm-16-in8192": (["rec_prepare", "rec_in_product"], []),
    # behind convolutions: those two and the gradient into the feature rows (its counter carries the number of layers behind the conv stack)
    "conv-lstm288-b12": (["window_rows", "rec_prepare", "rec_in_product", "gemm16_dx1"], []),
    "conv-lstm288-b12-dxkernel": (["window_rows", "rec_prepare", "rec_in_product", "gemm16_dx1"], []),
    "conv-mgu272x48-bptt4": (["window_rows", "rec_prepare", "rec_in_product", "gemm16_dx2"], []),
    "conv-lstm272x32-extras6": (["window_rows", "rec_prepare", "rec_in_product", "gemm16_dx2"], []),
    "conv1331-lstm32": (["window_rows", "rec_prepare", "rec_in_product", "gemm16_dx1"], []),
    "conv1331-mgu48x16": (["window_rows", "rec_prepare", "rec_in_product", "gemm16_dx2"], []),
    "lstm-2x32-wave-3launch": (["rec_forward", "rec_backward"], ["rec_step_fused"]),
    "mgu-2x32-wave-3launch": (["rec_forward", "rec_backward"], ["rec_step_fused"]),
}
for _n, _r in ROUTES.items():
    shape(_n)["route"] = _r

# the names rec_route_name (rec.hip) can print that are no shape's rec_route: {name: (why, the test that runs the kernel)}, held to the
# source and to the named tests by tests/test_blocks_cpu.py.  Empty: every kernel recRoute() can choose has a shape
REC_EXCUSED = {}


# the counters of ROUTE_COUNTERS that no shape's route holds: {counter: (why, the test that runs the launch)}.  `why` is one of
#   "exchange"     only a replica exchange reaches the launch (per-block parity of replica steps is tests/test_hip_r6.py's, bit-equal to host sums)
#   "periodic"     a launch of every 1000th step, not of a training step's own launch list
#   "repeat"       the same launch as a covered counter with another layer index as its argument (a deeper stack repeats it)
#   "unreachable"  no configuration hl_create accepts reaches the name (the loops that print it start at layer 1)
# tests/test_blocks_cpu.py holds this table to ROUTES (nothing here fires in a route, everything else does in one) and to the named tests
_R6 = "tests/test_hip_r6.py::test_two_replicas_with_large_local_batches_and_other_layer_types"
_DEEP_DENSE = "tests/test_hip_settings_r3.py::test_random_configurations_match_oracle"       # [wide-320x288x64-oneshot-gemm]: three layers, a launch each
_DEEP_CONV = "tests/test_hip_r5.py::test_every_form_of_the_convolutional_backward_pass_follows_the_reference"      # four layers, per-layer launches (GENERIC & 8)
EXCUSED = {
    "adam_kernel": ("exchange", "tests/test_hip_r6.py::test_rccl_sequence_at_the_baseline_shapes_on_one_rank"),      # (RCCL: dW -> all-reduce -> Adam launch)
    "conv_prep": ("exchange", _R6), "xchg_allreduce": ("exchange", _R6),
    "moments_kernel": ("periodic", "tests/test_hip_parity.py::test_thousand_step_sweep_matches_oracle"),
    "gemm16_dx0": ("unreachable", None), "conv_dx0": ("unreachable", None),
}
# (layers 2 and 3 run in the named tests; no test runs a stack deeper than four convolutions or four separately launched dense layers:
#  counters 4 .. 7 are the same launch_* call with l = 4 .. 7; gemm16_dx2 fires here: the gradient into the feature rows below two recurrent layers)
EXCUSED.update({"gemm16_%s%d" % (k, j): ("repeat", _DEEP_DENSE) for k in ("fwd", "dx") for j in range(2, 8) if (k, j) != ("dx", 2)})
EXCUSED.update({"conv_%s%d" % (k, j): ("repeat", _DEEP_CONV) for k in ("fwd", "dx") for j in range(2, 8)})

# the form of the row-block kernels (conv.hip) the first convolutional layer takes, as hl_debug_conv_rows_kind states it: 1 the RACER_atari
# geometry at compile time, 0 any geometry; every other shape: -1, no row-block kernels (conv_fwd0 and conv_dw_* count launches of either form)
ROWS_KIND = {"conv-atari-18opt-b8": 1, "conv-rows-32x32-b8": 0, "conv-rows-single-b8": 0, "conv-rows-stacked-extras3-b8": 0}


def make_learners(makers, name, params=None):
    """One learner per maker on SHAPES[name]: the same init_weights (so the same generator state behind it), then the same fp32
    weights in all of them -- `params`, or else the first learner's --, the same synthetic replay; tap on."""
    sh = shape(name)
    Ls = [mk(capi.make_config(**sh["kw"])) for mk in makers]
    for L in Ls:
        L.init_weights()
    w, m1, m2 = params if params is not None else Ls[0].get_params()
    for L in Ls:
        assert np.array_equal(L.get_rng_state(), Ls[0].get_rng_state())
        L.set_params(w, m1, m2)
    for L in Ls:
        fill_synth(L, synth_cfg(**sh["sc"]) if isinstance(sh["sc"], dict) else sh["sc"], sh["n_eps"])
        L.initialize()
        L.set_tap(True)
    return Ls


def snapshot(L):
    """What one step left behind in learner L; parameters and the gradient sum in double where L holds them so"""
    s = {k: L.readback(t) for k, t in INT_TAPS.items()}
    s.update({k: L.readback(t) for k, t in TAP_Q.items()})
    s["gradSum"] = L.readback(capi.TAP_GRADSUM)
    s["W"], s["M1"], s["M2"] = L.get_params64() if hasattr(L, "get_params64") else L.get_params()
    sc = L.scalars()
    s.update(beta=sc.beta, CmaxRet=sc.CmaxRet, nFar=sc.nFarPolicySteps, rng=L.get_rng_state())
    return s


def deviations(blocks, s, ref):
    """{quantity: {block or column: deviation of snapshot s from snapshot ref}}"""
    d = {q: blockdev(blocks, s[q], ref[q]) for q in PARAM_Q}
    d.update({q: coldev(s[q], ref[q]) for q in TAP_Q})
    return d


def episode_fields(L):
    """{field: all episodes' values in tag order} (the last entry of IMPW is the constant the library and the port both store)"""
    out = {}
    for k, f in EP_FIELDS.items():
        by = episode_arrays_by_tag(L, f)
        out[k] = np.concatenate([np.asarray(by[t], np.float64) for t in sorted(by)])
    return out


worst = worst_dev


@functools.lru_cache(maxsize=2)
def cpu_reference(name):
    """O32 and O64 stepped N_STEPS times side by side on the shape `name` (or the shape it names as `ref`): per step both snapshots and
    e_cpu, and the replay fields at the end.  Computed once per shape and shared (read-only) by the tests that need it."""
    if "ref" in shape(name):
        return cpu_reference(shape(name)["ref"])
    O32, O64 = make_learners([oracle_learner, oracle64_learner], name)
    blocks = param_blocks(O32)
    params0, rng0 = O32.get_params(), O32.get_rng_state()
    steps = []
    for _ in range(N_STEPS):
        O32.step(1); O64.step(1)
        s32, s64 = snapshot(O32), snapshot(O64)
        steps.append(dict(s32=s32, s64=s64, e_cpu=deviations(blocks, s32, s64)))
    ref = dict(blocks=blocks, params0=params0, rng0=rng0, steps=steps, fields32=episode_fields(O32), fields64=episode_fields(O64))
    O32.close(); O64.close()
    return ref


def bar(name, quantity, block, e_cpu):
    """the GPU bar of one block at one step: TOL32, or 4 e_cpu of that step for a block listed as ill-conditioned (never below TOL32:
    at a step where such a block happens to come out well on the CPU it is held to what every other block is held to); every block of
    a shape of BOUND_SHAPES is judged as a listed one (the module's docstring)"""
    if name in BOUND_SHAPES:
        return max(TOL32, 4 * e_cpu)
    return max(TOL32, 4 * e_cpu) if (quantity, block) in SHAPES[name].get("listed", {}) else TOL32


def judge(name, k, g, st, blocks, report=None):
    """-> problems: what the snapshot g of a learner's step k + 1 on shape `name` has wrong against step st = cpu_reference(name)["steps"][k]
    (blocks = its "blocks").  The integer taps, the generator state, nFarPolicySteps and CmaxRet equal those of both CPU builds, beta
    to 1e-12 of O64's, every parameter block and tap column within its bar of O64 on the block's own scale; a block whose reference is
    identically zero is zero.  The worst block of every quantity goes into `report`."""
    problems = []
    s32, s64 = st["s32"], st["s64"]
    for key in list(INT_TAPS) + ["rng"]:
        if not (np.array_equal(g[key], s64[key]) and np.array_equal(g[key], s32[key])):
            problems.append("step %d: %s differs" % (k + 1, key))
    if not (g["nFar"] == s64["nFar"] == s32["nFar"] and g["CmaxRet"] == s64["CmaxRet"] == s32["CmaxRet"]):
        problems.append("step %d: nFarPolicySteps / CmaxRet differ" % (k + 1))
    if not abs(g["beta"] - s64["beta"]) <= 1e-12 * s64["beta"]:
        problems.append("step %d: beta %r against %r" % (k + 1, g["beta"], s64["beta"]))
    e_hip = deviations(blocks, g, s64)
    for q in list(PARAM_Q) + list(TAP_Q):
        w, b = worst(e_hip[q])
        if report is not None:
            report.append("step %d %-8s worst e_hip %.2e in %-22s e_cpu there %s" % (k + 1, q, w, b, st["e_cpu"][q].get(b, "-")))
        for b, v in e_hip[q].items():
            e_cpu = st["e_cpu"][q][b]
            if v == "zero" or e_cpu == "zero":
                if v != e_cpu:
                    problems.append("step %d %s %s: %s on the device, %s on the CPU" % (k + 1, q, b, v, e_cpu))
            elif not v <= bar(name, q, b, e_cpu):
                problems.append("step %d %s %s: e_hip %.3e over its bar %.3e (e_cpu %.3e)" % (k + 1, q, b, v, bar(name, q, b, e_cpu), e_cpu))
    return problems
