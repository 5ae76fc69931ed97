/*
 * include/smarties_hip_discrete.h -- discrete actions of several variables and of up to 512 options.
 *
 * An addition to the C-ABI of include/smarties_hip.h, in a header of its own as include/smarties_hip_act.h, include/smarties_hip_dev.h
 * and include/smarties_hip_rollout.h are (the CPU oracle mirrors smarties_hip.h declaration by declaration and needs no twin of this
 * call; hl_config keeps its size).
 *
 * hl_create serves ONE discrete action variable of up to 64 options.  The reference takes any number of them and flattens them to one
 * label (MDPdescriptor::discreteActionValues / discreteActionShifts / maxActionLabel, Core/StateAction.cpp:134-156):
 *   shifts[0] = 1, shifts[i] = shifts[i-1] * values[i-1], maxActionLabel = prod values[i]
 *   label   = sum_i shifts[i] * floor(message[i])                      (ActionInfo::actionMessage2label, Core/StateAction.h:304-320)
 *   message = for i = dimA-1 .. 0: label / shifts[i] + 0.1, label %= shifts[i]          (label2actionMessage, :327-341)
 * and builds the RACER head over maxActionLabel options (RACER_common.cpp:119-146).  hl_create_discrete is hl_create -- the same body,
 * every other check and refusal of it unchanged -- for such an action space.
 *
 * Everything that carries an action then carries dimA entries per step, each `index_i + 0.1`: hl_append_episode*, the packed wire format
 * (hl_packed_episode_size keeps its formula: dimA action floats, n_options policy floats), hl_get_episode_field, the acting calls of
 * smarties_hip_dev.h and the rollout buffer (whose noise stays ONE uniform per step, component 0).  Stored behaviour policies are the
 * n_options probabilities of the labels.  hl_append_episode and hl_append_packed_episode check every entry of every step but the last
 * against its variable's count (HL_ERR_BAD_ARG); the device ingestion cannot: beyond 64 options the head (head_wide_kernel) clamps a label
 * outside the options to the nearest one, up to 64 options the heads take the label as they take hl_create's.
 */
#ifndef SMARTIES_HIP_DISCRETE_H
#define SMARTIES_HIP_DISCRETE_H

#include "smarties_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HL_DISCRETE_MAX_OPTIONS 512   /* prod values[i]: 1 + 2 x 512 = 1025 network outputs */
#define HL_DISCRETE_MAX_VARS    9     /* follows from it: every variable has at least two options */

/* hl_create for cfg->adv_kind == HL_ADV_DISCRETE with n_vars == cfg->dimA action variables of values[i] >= 2 options each and
 * cfg->n_options == prod values[i], 2 .. HL_DISCRETE_MAX_OPTIONS.
 *
 * Which head serves which net:
 *   up to 64 options   every net hl_create serves with one variable of as many options, on the head it takes there -- the fused and
 *                      panel heads (fusedw.hip, headp.hip, the one-launch recurrent step of rec.hip) up to their 16 / 32 options, the
 *                      step-chain launch (gemm16.hip) and the head launch (head.hip) up to 64.  Each of them forms the label from the
 *                      dimA entries; with one variable the results are hl_create's bit for bit.
 *   65 .. 512 options  the head launch alone (headw.hip: head_wide_kernel, a wavefront per sample, options strided over its lanes in
 *                      tiles of 64).  Every net takes it: the fused, panel and one-launch recurrent heads already hand nets beyond
 *                      their 16 / 32 options to the head launch, and a dense net that takes the step-chain launch up to 64 options
 *                      runs its forward chain, the head launch and the input-gradient launches on their own beyond.  No launch behind
 *                      the head bounds the output layer below 1025 columns: its weight gradient is the 16 x 16 tiles that serve hidden
 *                      layers of 2048 columns, the acting kernels loop over the output columns.
 *
 * Status: HL_ERR_BAD_ARG for adv_kind other than HL_ADV_DISCRETE, n_vars != dimA, n_vars outside 1 .. HL_MAX_DIMA, a NULL values, a
 * variable of fewer than two options, a product that differs from n_options, and whatever hl_create answers so; HL_ERR_UNSUPPORTED for
 * more than HL_DISCRETE_MAX_OPTIONS options (without a device the bare status and no handle; with one a handle that holds the message
 * alone, as hl_create's size refusals); HL_ERR_NO_DEVICE behind those checks. */
HL_API int hl_create_discrete(const hl_config* cfg, int32_t n_vars, const int32_t* values, hl_learner** out);

#ifdef __cplusplus
}
#endif

#endif
