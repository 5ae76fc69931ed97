/*
 * include/smarties_hip_dev.h -- acting and episode ingestion for simulators that keep their rollouts in DEVICE memory.
 *
 * An addition to the C-ABI of include/smarties_hip.h (same library, same conventions: plain C, an int status per call).  It lives in
 * a header of its own, as include/smarties_hip_act.h does, because the CPU oracle (oracle/port) mirrors smarties_hip.h declaration
 * by declaration and needs no twin of these calls: hl_forward, hl_append_episode and the host code of
 * smarties_amd/host/vracer_hip.h define their results.
 *
 * hl_forward takes its rows from a host pointer (pinned staging, a poll of the kernel's stamps, a copy out), hl_append_episode copies
 * an episode into a pinned buffer the ingest kernel reads over the bus, and the action head of RACER::selectAction runs per agent in
 * host fp64.  A simulator on the learner's GPU holds states, actions and rewards as device arrays already: the calls below take
 * DEVICE pointers (a torch tensor's data_ptr(): the library shares the process's HIP runtime) and never touch host copies of the data.
 * hl_forward_dev and hl_select_actions_dev act on rows (dense nets), hl_forward_sequences_dev and hl_select_actions_sequences_dev on
 * windows of a strided rollout buffer (recurrent nets, dense nets whose appended observations they stack, and feed-forward nets behind
 * convolutions, the Nature-DQN stack among them, whose stacked frames they read from a one-frame-per-step buffer), hl_append_episodes_dev stores the finished episodes
 * of any net.
 *
 * Streams.  `stream` is the caller's hipStream_t passed as void*; NULL is the null stream.  Every call takes the learner's lock,
 * refuses between hl_step_begin and hl_step_end (HL_ERR_STATE, as hl_forward), records an event on `stream` that the learner's stream
 * waits for, enqueues its work on the learner's stream, makes `stream` wait for the learner's completion event, and returns WITHOUT
 * waiting on the host: the inputs may be written by work queued on `stream` before the call, the outputs are valid for work queued
 * on `stream` after it, and gradient steps queued by an earlier hl_step are ahead of the call as they are ahead of hl_forward.
 * The arrays must stay allocated until that work has run.
 */
#ifndef SMARTIES_HIP_DEV_H
#define SMARTIES_HIP_DEV_H

#include "smarties_hip_act.h"

#ifdef __cplusplus
extern "C" {
#endif

/* widest input row (dense nets) and feature row (behind convolutions) the calls below serve, floats */
#define HL_ACT_DEV_MAX_ROW 8192

/* hl_forward for rows in device memory.  dStates: [n][dimS (1 + nAppendedObs)] floats (appended observations stacked in the row by
 * the caller, as for hl_forward), dOutputs: [n][nOutputs] doubles, both device memory.
 *
 * Served: dense nets without convolutions whose input row and layers are at most 2048 wide (the nets hl_forward's many-row route
 * takes).  The kernels are hl_forward's own, run straight on the caller's arrays -- no staging copy, no host poll, their completion
 * stamps go to a scratch block: up to 64 rows of a net at most 1024 wide the one-kernel route (a workgroup per row), everything else
 * the row-block kernel in chunks of HL_ACT_ROWS_CHUNK rows.  Where hl_forward picks the same kernel the result is the same bit for bit;
 * that is every call except a net beyond HL_ACT_ROWS_SMALL_NET weights below HL_ACT_ROWS_WIDE_MIN_N or 4 x batchSize rows, which
 * hl_forward sends over the training buffers and this call does not (the two agree to rounding there).
 * Served as well, input rows of 2049 .. HL_ACT_DEV_MAX_ROW floats (layers still at most 2048 wide): rows in device memory need not be
 * resident in a workgroup's LDS, so act_rows_panel_kernel (smarties_amd/csrc/actband.hip) stages the first layer's input in panels of up
 * to 1024 columns, its accumulators kept across the panels, and runs every other layer as the row-block kernel does.  Its sums run in
 * the row-block kernel's order; hl_forward sends such rows over the training buffers, so the two calls agree to rounding there.
 * The minibatch buffers and a minibatch drawn ahead are not touched.
 *
 * Status: HL_ERR_UNSUPPORTED (with a message) for every other net -- recurrent layers (hl_forward_sequences_dev below),
 * convolutions in front (hl_forward_sequences_dev below as well, the message names it: the conv-stack kernel reads an agent's row from
 * the states of its window; a net without appended observations passes windows of one state), input rows beyond HL_ACT_DEV_MAX_ROW,
 * layers beyond 2048, SMARTIES_HIP_GENERIC bit 2 (the message names the bound).  HL_ERR_STATE between hl_step_begin and hl_step_end.  n == 0: HL_OK, nothing is enqueued. */
HL_API int hl_forward_dev(hl_learner* h, int32_t n, const float* dStates, double* dOutputs, void* stream);

/* RACER::selectAction (Learners/RACER.cpp:30-47) for n agents without leaving the device: the forward pass of hl_forward_dev into a
 * buffer of the library, then ONE launch of the fp64 head kernel (smarties_amd/csrc/actdev.hip: act_head_kernel), which restates
 * smarties_amd/host/vracer_hip.h:209-258 for HL_ADV_ZERO, HL_ADV_GAUSSIAN and HL_ADV_DISCRETE:
 *   continuous  stdev = SoftPlus of the ParamLayer value; a = mean + stdev * noise (Continuous_policy.h:192-194), clipped to
 *               +-8.31776613503286 on bounded components; V = scaleNet2V(output 0); the Gaussian advantage with the clipped mean.
 *   discrete    SoftPlus-normalised probabilities; the label by inverse CDF -- the first option whose running sum in option order
 *               exceeds u --; the action stored as label + 0.1; the advantage A[label] - sum p A.
 * dNoise: [n][dimA] doubles already clipped to +-NORMDIST_MAX (Agent::sampleActionNoise); discrete head: [n] uniforms in [0, 1).
 * dNoise == NULL: the evaluation action (the mean; the arg-max option, Continuous_policy.h:779).
 * Outputs, device memory, in exactly the types hl_append_episode takes so that a simulator writes them straight into its rollout
 * buffers: dActions f64 [n][dimA], dMu f64 [n][polDim] (mean | stdev, or the probabilities), dValues f32 [n],
 * dAdvantages f32 [n] = (Fval)((Fval)(V + A) - (Fval)V).
 * The env-facing scaling of actions (tanh, bounds) is the caller's, as it is for the host code.
 * Status: as hl_forward_dev. */
HL_API int hl_select_actions_dev(hl_learner* h, int32_t n, const float* dStates, const double* dNoise, double* dActions, double* dMu,
                                 float* dValues, float* dAdvantages, void* stream);

/* hl_forward_sequences for windows in device memory: what a partially observable simulator on the learner's GPU calls to act.
 * dFirstRow [n] int64 and dNSteps [n] int32 are DEVICE arrays (the simulator knows its episode starts on the device; the host never
 * reads them), dStates is a [rows][dimS] float array in device memory, dOutputs [n][nOutputs] doubles in device memory.  The addressing is
 * hl_append_episodes_dev's: a [T][nEnv] buffer gives row_stride = nEnv and first_row = t0 * nEnv + env, a packed one row_stride = 1.
 *
 * The window of agent i, with len = dNSteps[i]:
 *     ns   = max(1, min(len, nnBPTTseq + 1 + nAppendedObs))        states read
 *     skip = max(len, 1) - ns                                      older states left out
 *     state g of the window (0 = oldest) is row dFirstRow[i] + (skip + g) * row_stride
 * A longer window is truncated to its newest nnBPTTseq + 1 + nAppendedObs states -- the window MemoryBuffer::agentToMinibatch forms
 * (MemoryBuffer.cpp:440-467) --, so a simulator passes the episode's start row and t + 1 and never computes the truncation itself
 * (hl_forward_sequences refuses such a window instead).  dNSteps[i] < 1 reads one row, dFirstRow[i].  Every row read must lie inside
 * dStates: the library cannot check that.  Row arithmetic is done in 64 bits.
 *
 * Served, recurrent nets: those of hl_forward_sequences' one-launch batched kernel (smarties_amd/csrc/actseq.hip) -- LSTM / MGU / RNN
 * layers of one type, no convolutions in front, no encoder_rnn layers, every layer at most 256 cells and 1024 inputs, the window within
 * 64 KB.  The kernel is that call's own with the windows gathered, truncated and standardised in the kernel from the caller's array:
 * ONE launch for any n (there is no staging, so HL_ACT_SEQ_CHUNK does not apply), min(n, compute units) workgroups walking the agents,
 * outputs written to dOutputs, no stamps and no system-scope fence -- completion is stream order.  From the standardised window on the
 * arithmetic and its order are the host route's: an agent's outputs equal hl_forward_sequences' on the same window bit for bit.
 * Served, recurrent nets on wide inputs: every net hl_create admits on a state beyond 256 components or a stacked input
 * dimS (1 + nAppendedObs) beyond 1024, up to 8192 -- LSTM / MGU / RNN layers of one type in multiples of 16 cells up to 1024, no
 * convolutions or encoder layers in front.  The route is hl_forward_sequences' for these nets, the time-step-major launches
 * (smarties_amd/csrc/rectm.hip) with the agents as the samples of one chain, behind a prepare launch of its own
 * (lstm_tm_prepare_acts_dev_kernel) that forms every agent's window by the rule above and gathers, truncates and standardises its states
 * from the caller's array into the first layer's input rows (16-byte loads where dimS is a multiple of 4 and dStates is 16-byte aligned,
 * scalar loads of the same values otherwise).  The agents go in chunks of min(local batch, HL_ACT_SEQ_CHUNK): a chain borrows the training
 * rows of that many samples between steps, as hl_forward_sequences does; nothing is staged, so HL_ACT_WIN_STAGE_BYTES does not apply, and
 * all chunks are enqueued back to back, chunk i0 reading the tables at offset i0.  The host never reads the tables, so it cannot know a
 * chunk's longest window: the chain always runs nnBPTTseq + 1 steps -- nnBPTTseq + number of layers diagonals, twice as many launches for
 * MGU -- whatever the windows are; an agent whose window has ended is left out by the forward tiles, and its outputs come from its own
 * last step.  The output layer writes straight to dOutputs, no stamps.  The input rows are the host route's bit for bit and the launches
 * behind them are the same: an agent's outputs equal hl_forward_sequences' on the same window bit for bit.
 * Served, dense nets: those hl_forward_dev serves.  One small launch (smarties_amd/csrc/actdev.hip: act_stack_dev_kernel) builds the
 * agents' rows [n][dimS (1 + nAppendedObs)] -- the last state, then the ones before it, steps before the first given state repeating
 * it -- into a buffer of the library, then hl_forward_dev's kernels run on those rows (no truncation: a dense net reads
 * 1 + nAppendedObs states whatever the window's length).
 * Served, feed-forward nets behind convolutions: those of hl_forward's conv-stack route (smarties_amd/csrc/actconv.hip) -- image, maps
 * and offset tables within 160 KB of a workgroup's LDS, feature rows and the dense layers behind at most 2048 wide, SMARTIES_HIP_GENERIC
 * bit 2 clear -- WHATEVER the row size: HL_ACT_CONV_MAX_ROW_BYTES is a switch of the host route's copy into pinned staging and does not
 * apply to rows that lie in device memory (the stack of settings/RACER_atari.json, rows of 110 KB, is served without any environment
 * switch).  With frame stacking (nAppendedObs = k: the image's channels are the last k + 1 frames) the simulator stores ONE frame per
 * step in a [T][nEnv][dimS] buffer and passes the episode's start row and t + 1.  Element c of agent i's stacked row
 * [dimS (1 + nAppendedObs)] is component c % dimS of the state j = c / dimS steps before the newest, read from row
 *     dFirstRow[i] + max(max(dNSteps[i], 1) - 1 - j, 0) * row_stride
 * -- steps before the first given state repeat it, a longer window is read from its newest 1 + nAppendedObs states only.  Two launches
 * in the learner's stream: act_conv_dev_kernel, ONE launch for any n of min(n, compute units) workgroups walking the agents, each
 * loading its agent's row straight from those states (no [n][row] intermediate; 16-byte loads where dimS, the row and the image are
 * multiples of 4 floats and dStates is 16-byte aligned, scalar loads of the same values otherwise), standardising it on load and running
 * the whole conv stack out of LDS; then the row-block kernel on the feature rows per HL_ACT_ROWS_CHUNK agents, outputs to dOutputs.
 * From the standardised row on the arithmetic and its order are act_conv_kernel's: an agent's outputs equal hl_forward's on the same
 * stacked row bit for bit wherever hl_forward takes the conv-stack route (rows up to HL_ACT_CONV_MAX_ROW_BYTES; beyond them hl_forward
 * runs the training launches, which agree to rounding).
 * Served, feed-forward nets behind convolutions beyond that plan (smarties_amd/csrc/actband.hip; the Nature-DQN stack of
 * Network/Builder.cpp:189-194 -- conv 32 / 64 / 64 on 84 x 84 x 4, a feature row of 3136 -- takes both kernels):
 *   an image that does not fit the LDS beside the maps (above about 150 KB, or the Nature stack's 110 KB beside maps of 70 KB) runs
 *   act_conv_band_dev_kernel in place of act_conv_dev_kernel: the FIRST layer in the smallest number of bands of output rows, from 2 on,
 *   whose input rows fit -- a band's rows of every channel are loaded from the agent's window into LDS, rows two bands share are read
 *   again from device memory --, every other layer as before; refused only where a MAP exceeds the LDS at any band count;
 *   a feature row of 2049 .. HL_ACT_DEV_MAX_ROW floats runs act_rows_panel_kernel in place of the row-block kernel (see hl_forward_dev).
 * Both keep the order of every sum of the kernels they stand in for (tests: equal bits on every net both forms can run); hl_forward
 * sends these nets over the training buffers, so the device and the host calls agree to rounding there.
 *
 * Status: HL_ERR_UNSUPPORTED, with a message naming hl_forward_sequences, for every other recurrent net -- layers beyond 256 cells on
 * narrow inputs (the other time-step-major nets), convolutions in front, encoder_rnn layers: they act on windows in host memory -- and, with
 * a message naming hl_forward and the bound, for feed-forward nets behind convolutions beyond the plans above (a map beyond 160 KB of
 * LDS at any band count; feature rows beyond HL_ACT_DEV_MAX_ROW; dense layers beyond 2048; SMARTIES_HIP_GENERIC bit 2).
 * HL_ERR_BAD_ARG for a null handle or array, n < 0 or row_stride < 1.  HL_ERR_STATE between hl_step_begin and hl_step_end.
 * n == 0: HL_OK, nothing is enqueued.  The minibatch buffers and a minibatch drawn ahead are not touched. */
HL_API int hl_forward_sequences_dev(hl_learner* h, int32_t n, const int64_t* dFirstRow, const int32_t* dNSteps, int64_t row_stride,
                                    const float* dStates, double* dOutputs, void* stream);

/* hl_select_actions_dev on windows: the forward pass of hl_forward_sequences_dev into a buffer of the library, then the same ONE launch
 * of act_head_kernel.  dNoise and the four outputs as for hl_select_actions_dev; the windows, nets and status as for
 * hl_forward_sequences_dev.  With hl_append_episodes_dev the loop act -> simulate -> append -> step of a recurrent net, or of a net
 * behind convolutions, never leaves the device. */
HL_API int hl_select_actions_sequences_dev(hl_learner* h, int32_t n, const int64_t* dFirstRow, const int32_t* dNSteps, int64_t row_stride,
                                           const float* dStates, const double* dNoise, double* dActions, double* dMu, float* dValues,
                                           float* dAdvantages, void* stream);

/* hl_append_episode for a batch of finished episodes held in device memory.  nsteps, terminated, tags, first_row: HOST arrays of nEp
 * entries (free after return).  Step t of episode e is row first_row[e] + t * row_stride of each device array: dStates f32
 * [rows][dimS], dActions f64 [rows][dimA], dMu f64 [rows][polDim], dRewards f64 [rows], dValues f32 [rows], dAdvantages f32 [rows] or
 * NULL.  A [T][nEnv] rollout buffer is ingested with row_stride = nEnv and first_row = t0 * nEnv + env, a packed one with
 * row_stride = 1.  Every row first_row[e] + t * row_stride, t < nsteps[e], must lie inside the arrays: the library cannot check that.
 *
 * The host bookkeeping is hl_append_episode's, episode by episode in the order given (slots, episode ids, counters, order, pending
 * Retrace; eviction follows with the next step).  The data moves with ingest_dev_kernel (smarties_amd/csrc/actdev.hip): a strided
 * gather into the replay's arrays with the insertion values of the derived fields, the episode's reward sum formed in step order in
 * fp64 -- the host route's value bit for bit.  Episodes staged by earlier hl_append_episode calls are handed to the device first.
 * With hl_set_episode_log on, the call reads the sums back (one device wait) and writes hl_append_episode's log lines; otherwise it
 * waits for nothing.
 * Status: HL_ERR_BAD_ARG for nEp < 0, a null table or array, row_stride < 1, an episode of fewer than 2 steps or a negative first
 * row -- checked before anything is stored.  HL_ERR_STATE between hl_step_begin and hl_step_end.  nEp == 0: HL_OK. */
HL_API int hl_append_episodes_dev(hl_learner* h, int32_t nEp, const int32_t* nsteps, const int32_t* terminated, const int64_t* tags,
                                  const int64_t* first_row, int64_t row_stride, const float* dStates, const double* dActions,
                                  const double* dMu, const double* dRewards, const float* dValues, const float* dAdvantages, void* stream);

/* ---- acting on a policy snapshot while gradient steps run -------------------------------------------------------------------------
 * The four acting calls above are enqueued on the learner's stream: behind hl_step(2000) an answer of tens of microseconds waits for every
 * queued step, and it cannot be had earlier from the live weights, which Adam rewrites in every weight-gradient launch.  The calls below let
 * the learner publish a SNAPSHOT of what acting reads, in stream order, and switch the acting calls to read it on a stream of their own,
 * concurrently with the queued steps.  The default is unchanged; the training launches are not touched; results are bit for bit those of live
 * acting at the moment the snapshot was taken. */
enum { HL_ACT_LIVE = 0, HL_ACT_SNAPSHOT = 1 };

/* Enqueues on the learner's stream, behind every step queued so far, a copy of everything the acting kernels read of the learner's mutable
 * state: the parameter blob (hl_num_params floats) and the state standardisation (means and scales, dimS floats each; the head kernel
 * reads network outputs, noise and the configuration only).  ONE launch (smarties_amd/csrc/actdev.hip: policy_snapshot_kernel, 16-byte
 * accesses; timed label policy_snapshot); returns without waiting.  Two buffers, allocated at the first call; the copy goes to the one that
 * is not current: the learner's stream first waits for an event recorded on the acting stream behind the last acting call that read that
 * buffer, after the copy it records the buffer's "ready" event, and the host marks the buffer current -- acting calls from here on read it,
 * calls enqueued before keep the other one.  Stream order and events are the only synchronisation: no device-side protocol, no wait inside a
 * kernel.  A snapshot is not changed by later steps, hl_set_params, hl_set_scaling or hl_restart.
 * Status: HL_ERR_BAD_ARG for a null handle. */
HL_API int hl_policy_snapshot(hl_learner* h);

/* Two host-side numbers, no device wait: the snapshots taken so far, and nGradSteps as queued when the current one was taken (-1 before the
 * first) -- hl_get_counts' nGradSteps minus this is the policy lag of the actions being produced.  Either pointer may be NULL. */
HL_API int hl_policy_snapshot_info(hl_learner* h, int64_t* n_snapshots, int64_t* nGradSteps);

/* What hl_forward_dev, hl_select_actions_dev, hl_forward_sequences_dev and hl_select_actions_sequences_dev read and where they run.
 * HL_ACT_LIVE (the default): as described above -- every code path, launch, label and buffer as without this call.
 * HL_ACT_SNAPSHOT: the calls run on an acting stream the learner owns (created at first use, default priority).  The handshake with the
 * caller's `stream` is the same, against the acting stream; the acting stream also waits for the current snapshot's "ready" event and for
 * nothing else of the learner's stream, so a call completes while gradient steps queued before it still run.  The kernels are the ones the
 * live source picks for the same net and n, on arguments that differ in the three pointers to the blob, the means and the scales only; the
 * scratch (stamps, network outputs, stacked rows, feature rows, the stamps' tag) is a set of its own, grown behind a wait for the acting
 * stream only.  Nothing writable is shared between the two streams, and nothing the acting stream runs waits inside a kernel: the step
 * kernels' bounded waits for peer workgroups can be delayed by one acting launch at most, never held.
 * hl_append_episodes_dev and every host-pointer call are unaffected by the source.
 * Status: HL_ERR_BAD_ARG for a null handle or an unknown source.  From the acting calls under HL_ACT_SNAPSHOT: HL_ERR_STATE before any
 * snapshot exists (the message names hl_policy_snapshot) and between hl_step_begin and hl_step_end; HL_ERR_UNSUPPORTED, with a message
 * naming HL_ACT_LIVE, from the window calls for recurrent nets on wide inputs -- their chain borrows training rows, the step tables and the
 * last hidden layer's activations, so it cannot run beside a step --; every net a live call refuses is refused alike.
 * hl_destroy waits for the acting stream and releases the stream, the events and the buffers. */
HL_API int hl_act_dev_source(hl_learner* h, int32_t source);

#ifdef __cplusplus
}
#endif
#endif
