/*
 * include/smarties_hip_ppo.h -- the PPO learner (proximal policy optimisation with the adaptive KL penalty; Learners/PPO.cpp,
 * PPO_train.cpp, PPO_common.cpp of the reference, settings learner "PPO"), the reference's only on-policy method.
 *
 * An addition to the C-ABI of include/smarties_hip.h in a header of its own, as include/smarties_hip_naf.h, _dqn.h and _dpg.h are
 * (hl_config keeps its layout and size; the CPU oracle has no twin of these calls).
 *
 * Two dense feed-forward networks (PPO_common.cpp: setupNet).  The ACTOR is the handle's network (hl_get_params, hl_param_layout,
 * hl_forward): continuous actions -- dimA outputs, the policy mean under nnOutputFunc, and a ParamLayer of dimA standard-deviation
 * parameters started from explNoise, hl_num_outputs = 2 dimA; discrete actions (n_vars > 0) -- one output per option, the product of the
 * variables' counts, read through SoftPlus as Discrete_policy does, hl_num_outputs = n_options.  No value column.  The CRITIC has the
 * same hidden layers on the dimS state components and one Linear output; its learning rate is 3 x learnrate.  No target weights.
 *
 * One step (PPO::Train): rho, D_KL from the live actor; isOff = rho outside [1 - C, 1 + C], C = clipImpWeight < 1; gain = rho (ret - Vold)
 * on the STORED return estimate and state value, zeroed by the two clipping rules; the actor's gradient is
 * weightSum2Grads(policyGradient(a, gain), KLDivGradient(mu, -penalCoef), 1); the critic's output gradient is (ret - V) x isOff, as the
 * reference writes it.  Write-backs: error ret - V, D_KL, rho, stateValue[t] = V, actionAdvantage[t] = 0.  After the rows, in ascending
 * row order: the penalty accumulators, DKL_target's adaptation and updatePenalizationCoef.
 *
 * On-policy life cycle (PPO::setupTasks), nHorizon = maxTotObsNum: hl_step answers HL_ERR_STATE while fewer than nHorizon steps are
 * stored; every step adds batchSize to cntBatch; at cntBatch >= nHorizon the reward / state statistics move (updateRewardsStats, with
 * 3 x learnrate: the constructor's factor stays in the settings the replay reads), cntBatch = 0, cntEpoch += 1; at cntEpoch >= nEpochs
 * every stored episode is dropped (clearAll; the seen counters stay) and the counters start over.  hl_step(h, n, ..) with n beyond the
 * steps left before the clear answers HL_ERR_STATE and runs none.  hl_step_begin answers HL_ERR_UNSUPPORTED: the life cycle is hl_step's.  The caller appends the behaviour-time values V(s) of hl_ppo_values
 * through values[] of hl_append_episode (selectAction's appendValues; 0 behind a terminal state); the return estimate is swept when an
 * episode arrives and at hl_initialize, not per step.
 *
 * Served: every returnsEstimator (PPO's default is GAE), nn_type HL_NN_FFNN without convolutions, encoder layers (the reference shares
 * one encoder under both nets), encoder_rnn or appended observations, dimS <= 512, dimA <= HL_PPO_MAX_DIMA continuous, up to
 * HL_DISCRETE_MAX_OPTIONS options discrete, local batches up to 1024, one replica.  Steps are eager launches.  Acting from device memory,
 * the window calls, the snapshot source and the rollout buffer are not wired for these learners.
 */
#ifndef SMARTIES_HIP_PPO_H
#define SMARTIES_HIP_PPO_H

#include "smarties_hip.h"
#include "smarties_hip_discrete.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HL_PPO_MAX_DIMA 16

typedef struct hl_ppo_config {
  int32_t struct_size;     /* sizeof(hl_ppo_config) */
  int32_t nEpochs;         /* the reference's batchSize / obsPerStep, >= 1 */
  double klDivConstraint;  /* the initial DKL_target */
  int32_t n_vars;          /* 0: continuous actions; else cfg->dimA discrete variables, as hl_create_discrete takes them */
  int32_t values[HL_DISCRETE_MAX_VARS];      /* their option counts; the product is cfg->n_options */
} hl_ppo_config;

/* hl_create for a PPO learner.  cfg->adv_kind is ignored.  Status: whatever hl_create answers for the configuration, and
 * HL_ERR_UNSUPPORTED (without a device the bare status; with one a handle that holds a message naming PPO) for recurrent nn_type,
 * encoder_rnn, n_encoder > 0, convolutions, appended observations, n_ranks > 1, clipImpWeight >= 1, nEpochs < 1 and the sizes beyond the
 * served ones. */
HL_API int hl_create_ppo(const hl_config* cfg, const hl_ppo_config* ppo, hl_learner** out);

/* V(s) of the critic for n raw states [n][dimS] (standardised on load, as hl_forward) */
HL_API int hl_ppo_values(hl_learner* h, int32_t n, const float* states, double* v);

/* the critic's padded blob (layers: dense 1, (dense, residual) ..., output; every block on a multiple of 8 floats) and its Adam
 * moments; NULL = skip / keep.  HL_ERR_BAD_ARG for a learner that is no PPO learner. */
HL_API int64_t hl_ppo_critic_num_params(const hl_learner* h);      /* -1: no PPO learner */
HL_API int hl_ppo_get_critic(hl_learner* h, float* w, float* m1, float* m2);
HL_API int hl_ppo_set_critic(hl_learner* h, const float* w, const float* m1, const float* m2);

typedef struct hl_ppo_state {
  double penalCoef, DKL_target;
  int64_t cntBatch, cntEpoch;
  int64_t stepsLeft;       /* gradient steps before the clear (read only: hl_ppo_set_state ignores it) */
} hl_ppo_state;
HL_API int hl_ppo_get_state(hl_learner* h, hl_ppo_state* st);
HL_API int hl_ppo_set_state(hl_learner* h, const hl_ppo_state* st);      /* a restart, and the tests, place penalCoef and DKL_target */

/* development read-back of the last step (for the tests; UNSTABLE, no part of the interface a caller may build on): what = 0 rho [B],
 * 1 D_KL [B], 2 isOff [B], 3 gain [B], 4 V [B], 5 the critic's output gradient [B], 6 the critic's summed weight gradient
 * [hl_ppo_critic_num_params] */
HL_API int hl_ppo_readback(hl_learner* h, int32_t what, double* dst, int64_t cap);

#ifdef __cplusplus
}
#endif

#endif
