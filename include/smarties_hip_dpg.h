/*
 * include/smarties_hip_dpg.h -- the DPG learner (deterministic policy gradient with ReF-ER; Learners/DPG.cpp of the reference, settings
 * learner "DDPG" / "DPG").
 *
 * An addition to the C-ABI of include/smarties_hip.h in a header of its own, as include/smarties_hip_naf.h and include/smarties_hip_dqn.h
 * are (hl_config keeps its layout and size; the CPU oracle has no twin of these calls).
 *
 * Two dense feed-forward networks.  The ACTOR is the handle's network (hl_get_params, hl_param_layout, hl_forward): dimA outputs -- the
 * policy mean under nnOutputFunc -- and a ParamLayer of dimA standard-deviation parameters started from explNoise; hl_num_outputs =
 * 2 dimA.  The CRITIC has the same hidden layers on an input of dimS + dimA -- the standardised state, then the action -- and one Linear
 * output; its learning rate is 10 x learnrate and its nnLambda 1e-4 (the DPG constructor).  Both keep target weights.  The critic's
 * action input is the stored action of the step (the action as the policy drew it, what the replay holds beside mu) for q, and the
 * actor's output vector -- the mean as the net emits it, no bound applied -- for Q~(s, mu~(s)): bounded action spaces change the
 * importance weight's mean (Continuous_policy.h: SquashedNormalPolicy::getMean clips it), never the critic's input.
 *
 * One step (DPG::Train): rho, D_KL and the far-policy rule from the live actor; q = Q(s_t, a_t) from the live critic;
 * p = Q~(s_t, mu~(s_t)) from both target nets, whose gradient with respect to the action input is the policy gradient on the mean
 * (zero for far-policy samples); the standard-deviation slots get fixExplorationGrad(explNoise); both are mixed with
 * KLDivGradient(mu, -1) by beta.  The critic's output gradient is target - q (0 if far-policy), target = r_t + gamma Q~(s_{t+1},
 * mu~(s_{t+1})) unless t+1 is terminal or the sample far-policy.  Write-backs: error target - q, D_KL, rho, stateValue[t] = p,
 * actionAdvantage[t] = q - p, stateValue[t+1] = Q~_next (where t+1 is itself sampled that step's own write wins).
 *
 * As in the reference, where the constructor's learnrate x 10 stays in the settings the replay reads, the state and reward statistics
 * of every 1000th step move with 10 x learnrate as well.
 *
 * Served: returnsEstimator HL_RET_NONE, nn_type HL_NN_FFNN without convolutions, encoder layers (the reference shares one encoder
 * between both nets; there is no shared layer here), encoder_rnn or appended observations, 1 to
 * HL_MAX_HIDDEN hidden layers of up to 512 units whose activation derivatives fit the target kernel's LDS (dpgt.hip: two 512-wide
 * layers, six 256-wide ones, eight up to 128), dimS <= 512, dimA <= HL_DPG_MAX_DIMA, local batches up to 1024, one replica; every
 * sampler and removal rule.  Steps are eager launches.  Acting from device memory, the window calls, the snapshot source and the
 * rollout buffer are not wired for these learners; the Ornstein-Uhlenbeck noise of selectAction stays with the caller.
 */
#ifndef SMARTIES_HIP_DPG_H
#define SMARTIES_HIP_DPG_H

#include "smarties_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HL_DPG_MAX_DIMA 16

typedef struct hl_dpg_config {
  int32_t struct_size;   /* sizeof(hl_dpg_config) */
  int32_t reserved;
  double targetDelay;    /* as hl_naf_config::targetDelay -- 0 < d < 1: tgt += d (w - tgt) every step; d >= 1: copy every (int)d steps;
                            d <= 0: the target weights stay as they are --, for both nets */
} hl_dpg_config;

/* hl_create for a DPG learner.  cfg->adv_kind is ignored.  Status: whatever hl_create answers for the configuration, and
 * HL_ERR_UNSUPPORTED (without a device the bare status; with one a handle that holds a message naming DPG) for return estimators
 * other than HL_RET_NONE, recurrent nn_type, encoder_rnn, n_encoder > 0, convolutions, appended observations, n_ranks > 1 and the sizes beyond
 * the served ones. */
HL_API int hl_create_dpg(const hl_config* cfg, const hl_dpg_config* dpg, hl_learner** out);

/* the critic's padded blob (layers: dense 1, (dense, residual) ..., output; every block on a multiple of 8 floats, as hl_param_layout
 * describes the actor's) and its Adam moments; NULL = skip / keep.  HL_ERR_BAD_ARG for a learner that is no DPG learner. */
HL_API int64_t hl_dpg_critic_num_params(const hl_learner* h);      /* -1: no DPG learner */
HL_API int hl_dpg_get_critic(hl_learner* h, float* w, float* m1, float* m2);
HL_API int hl_dpg_set_critic(hl_learner* h, const float* w, const float* m1, const float* m2);
/* the target weights: which = 0 the actor's (layout of hl_get_params), 1 the critic's */
HL_API int hl_dpg_get_target(hl_learner* h, int32_t which, float* w);
HL_API int hl_dpg_set_target(hl_learner* h, int32_t which, const float* w);

/* development read-back of the last step (for the tests; UNSTABLE, no part of the interface a caller may build on): what = 0 Q~_t [B], 1 Q~_next [B], 2 dQ~/da [B][dimA], 3 q [B], 4 the critic's output
 * gradient [B], 5 the critic's summed weight gradient [hl_dpg_critic_num_params] */
HL_API int hl_dpg_readback(hl_learner* h, int32_t what, double* dst, int64_t cap);

#ifdef __cplusplus
}
#endif

#endif
