/*
 * include/smarties_hip_dqn.h -- the DQN learner (double Q-learning with a softmax behaviour policy; Learners/DQN.cpp of the reference).
 *
 * An addition to the C-ABI of include/smarties_hip.h in a header of its own, as include/smarties_hip_naf.h and
 * include/smarties_hip_discrete.h are (hl_config keeps its layout and size; the CPU oracle has no twin of these calls).
 *
 * One dense feed-forward network whose hl_num_outputs = nOpt outputs are the Q values of the nOpt options (no value column, no
 * ParamLayer); nOpt is the product of the variables' option counts, labels as in hl_create_discrete.  The policy is the softmax
 * p_i = exp(clamp(Q_i, -8, 8)) / sum_j exp(..); the stored policy vector of a step holds the nOpt behaviour probabilities.  The training
 * step is ReF-ER's: rho = p_a / beta_a, D_KL, the far-policy rule, the beta-mixed penalty, the write-backs and the bookkeeping are
 * hl_create's; the error is e = target - Q_a.  With returnsEstimator HL_RET_NONE the target is r_t + gamma sum_i p^_i Q~_i (double Q: p^ the
 * live net's policy on s_{t+1}, Q~ the target net's outputs there), with any other estimator it is the stored return estimate.  The
 * target net is a second weight set kept by the optimiser step.
 *
 * Served: nn_type HL_NN_FFNN without convolutions, encoder_rnn or appended observations, states of up to 512 components, local batches
 * up to 1024, one replica, 2 .. HL_DISCRETE_MAX_OPTIONS options; every sampler, removal rule and return estimator.  Steps are eager
 * launches (no graph replay).  hl_forward returns the nOpt Q values.  Acting from device memory, the window calls, the snapshot source
 * and the rollout buffer are not wired for these learners.
 */
#ifndef SMARTIES_HIP_DQN_H
#define SMARTIES_HIP_DQN_H

#include "smarties_hip_discrete.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hl_dqn_config {
  int32_t struct_size;   /* sizeof(hl_dqn_config) */
  int32_t reserved;
  double targetDelay;    /* as hl_naf_config::targetDelay -- 0 < d < 1: tgt += d (w - tgt) every step; d >= 1: copy every (int)d steps --,
                            and d <= 0: no target net, the double-Q target evaluates the live net's own Q values (DQN.cpp:179) */
} hl_dqn_config;

/* hl_create_discrete for a DQN learner: `values` gives the options of each of the cfg->dimA action variables, cfg->n_options their
 * product.  cfg->adv_kind is ignored.  Status: whatever hl_create_discrete answers for the configuration, and HL_ERR_UNSUPPORTED (without
 * a device the bare status; with one a handle that holds a message naming DQN) for recurrent nn_type, convolutions, encoder_rnn,
 * n_ranks > 1, more than HL_DISCRETE_MAX_OPTIONS options, appended observations, dimS > 512 and local batches beyond 1024. */
HL_API int hl_create_dqn(const hl_config* cfg, const hl_dqn_config* dqn, const int32_t* values, hl_learner** out);

/* the target weights: the padded blob in the layout of hl_get_params.  HL_ERR_BAD_ARG for a learner that is no DQN learner. */
HL_API int hl_dqn_get_target(hl_learner* h, float* w);
HL_API int hl_dqn_set_target(hl_learner* h, const float* w);

#ifdef __cplusplus
}
#endif

#endif
