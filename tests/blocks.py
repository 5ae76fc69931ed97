"""Shared by tests/test_blocks_cpu.py and tests/test_hip_blocks.py: the shapes (one per launch route of the training step: every
counter of ROUTE_COUNTERS fires in a recorded route or is in EXCUSED, tests/test_blocks_cpu.py), the fp32 / fp64 pair of the CPU
restatement stepped side by side, and the per-block deviations.

O32 is oracle/liboracle_port.so, O64 its build with the arrays in double (oracle/liboracle_port64.so).  Both start from the
same fp32 weights and the same synthetic replay and draw their own minibatches.  e_cpu(block) = dev(O32, O64) is what fp32
arithmetic in the reference's own summation order loses in that block; the CPU test holds it to TOL32 / 3, which is what makes
TOL32 per block a fair bar for e_hip(block) = dev(HIP, O64) in the GPU test.  A block that cannot meet TOL32 / 3 because it is
ill-conditioned is LISTED in its shape's entry with the e_cpu measured on the CPU; its GPU bar is 4 e_cpu, taken at test time.

Why blocks get listed (all of them are bias blocks of W in the first steps): hidden biases start at zero, so after k steps a
bias IS the sum of k Adam updates eta numer / (eps + sqrt(M2)), each of size ~eta.  For a bias whose gradient is small -- 0.1 |g| / B
comparable to eps = FLT_EPSILON, where the quotient turns from |g| / eps to 1 -- an absolute error of the gradient sum of 5e-7 of the
block's largest element (ordinary fp32 summation) moves the quotient by up to 0.4 max|g| / B: 1e-5 of the block's largest update and
more.  Weight blocks do not show it (their elements are 1000 eta large), nor do M1 / M2 / gradSum (no quotient).
"""
import functools

import numpy as np

from smarties_amd import capi
from oracle_api import fill_synth, oracle64_learner, oracle_learner, synth_cfg
from parity import blockdev, coldev, episode_arrays_by_tag, param_blocks, worst_dev

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


# name -> kw (make_config), sc (synth_cfg), n_eps, route (launches per eager step of every counter of ROUTE_COUNTERS that fires),
# listed ({(quantity, block): e_cpu measured on the CPU}: the ill-conditioned blocks, see the module's docstring)
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
}

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
}
for _n, _l in LISTED.items():
    SHAPES[_n]["listed"] = _l


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
}
for _n, _r in ROUTES.items():
    SHAPES[_n]["route"] = _r


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
#  counters 4 .. 7 are the same launch_* call with l = 4 .. 7)
EXCUSED.update({"gemm16_%s%d" % (k, j): ("repeat", _DEEP_DENSE) for k in ("fwd", "dx") for j in range(2, 8)})
EXCUSED.update({"conv_%s%d" % (k, j): ("repeat", _DEEP_CONV) for k in ("fwd", "dx") for j in range(2, 8)})

# the form of the row-block kernels (conv.hip) the first convolutional layer takes, as hl_debug_conv_rows_kind states it: 1 the RACER_atari
# geometry at compile time, 0 any geometry; every other shape: -1, no row-block kernels (conv_fwd0 and conv_dw_* count launches of either form)
ROWS_KIND = {"conv-atari-18opt-b8": 1, "conv-rows-32x32-b8": 0, "conv-rows-single-b8": 0, "conv-rows-stacked-extras3-b8": 0}


def make_learners(makers, name, params=None):
    """One learner per maker on SHAPES[name]: the same init_weights (so the same generator state behind it), then the same fp32
    weights in all of them -- `params`, or else the first learner's --, the same synthetic replay; tap on."""
    sh = SHAPES[name]
    Ls = [mk(capi.make_config(**sh["kw"])) for mk in makers]
    for L in Ls:
        L.init_weights()
    w, m1, m2 = params if params is not None else Ls[0].get_params()
    for L in Ls:
        assert np.array_equal(L.get_rng_state(), Ls[0].get_rng_state())
        L.set_params(w, m1, m2)
    for L in Ls:
        fill_synth(L, synth_cfg(**sh["sc"]), sh["n_eps"])
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
    """O32 and O64 stepped N_STEPS times side by side on SHAPES[name]: per step both snapshots and e_cpu, and the replay fields at the
    end.  Computed once per shape and shared (read-only) by the tests that need it."""
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
    at a step where such a block happens to come out well on the CPU it is held to what every other block is held to)"""
    return max(TOL32, 4 * e_cpu) if (quantity, block) in SHAPES[name].get("listed", {}) else TOL32
