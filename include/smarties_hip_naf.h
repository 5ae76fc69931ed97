/*
 * include/smarties_hip_naf.h -- the NAF learner (normalized advantage functions; Learners/NAF.cpp of the reference).
 *
 * An addition to the C-ABI of include/smarties_hip.h in a header of its own, as include/smarties_hip_discrete.h is (hl_config keeps its
 * layout and size; the CPU oracle has no twin of these calls).
 *
 * One dense feed-forward network with the outputs
 *   [ V | l[0 .. nL) | m[0 .. dimA) | s[0 .. dimA) ],   nL = dimA (dimA + 1) / 2,   hl_num_outputs = 1 + nL + 2 dimA
 * l fills the lower triangle L row by row (diagonal through SoftPlus), P = L L^T, A(a) = -1/2 (a - mu)^T P (a - mu) with mu = m
 * (HardSigmoid where the component is bounded), Q = V + A; the policy is Continuous_policy on the raw (m, s), s the ParamLayer.  The
 * training step is ReF-ER's second algorithm: rho, D_KL, the far-policy rule, the beta-mixed penalty, the write-backs and the
 * bookkeeping are hl_create's.  A second weight set, the target network, is kept by the optimiser step; with returnsEstimator
 * HL_RET_NONE the target of a step is r_t + gamma V_tgt(s_{t+1}), with any other estimator it is the stored return estimate.
 *
 * Served: nn_type HL_NN_FFNN without convolutions, encoder_rnn or appended observations, states of up to 512 components, local batches
 * up to 1024, one replica, dimA 1 .. HL_NAF_MAX_DIMA; every sampler, removal rule and return estimator.  Steps are eager launches
 * (no graph replay).  hl_forward returns the hl_num_outputs outputs: the policy mean sits at 1 + nL, the ParamLayer's sigma
 * parameter behind it.  Acting from device memory, the snapshot source and the rollout buffer are not wired for these learners.
 */
#ifndef SMARTIES_HIP_NAF_H
#define SMARTIES_HIP_NAF_H

#include "smarties_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HL_NAF_MAX_DIMA 17   /* nL = 153, 1 + 153 + 17 = 171 dense outputs: three output columns per lane of the head's wavefront */

typedef struct hl_naf_config {
  int32_t struct_size;   /* sizeof(hl_naf_config) */
  int32_t reserved;
  double targetDelay;    /* settings targetDelay: 0 < d < 1: tgt += d (w - tgt) every step; d >= 1: copy every (int)d steps, first on
                            the first step; d <= 0: the target weights stay as initialised (Network/Optimizer.cpp:162-177) */
} hl_naf_config;

/* hl_create for a NAF learner.  cfg->adv_kind is ignored.  Status: whatever hl_create answers for the configuration, and
 * HL_ERR_UNSUPPORTED (without a device the bare status; with one a handle that holds the message) for recurrent nn_type, convolutions,
 * encoder_rnn, n_ranks > 1, dimA > HL_NAF_MAX_DIMA, appended observations, dimS > 512 and local batches beyond 1024. */
HL_API int hl_create_naf(const hl_config* cfg, const hl_naf_config* naf, hl_learner** out);

/* the target weights: the padded blob in the layout of hl_get_params.  HL_ERR_BAD_ARG for a learner that is no NAF learner. */
HL_API int hl_naf_get_target(hl_learner* h, float* w);
HL_API int hl_naf_set_target(hl_learner* h, const float* w);

#ifdef __cplusplus
}
#endif

#endif
