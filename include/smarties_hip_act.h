/*
 * include/smarties_hip_act.h -- batched acting: the network evaluated for MANY agents' windows in one call.
 *
 * An addition to the C-ABI of include/smarties_hip.h (same library, same conventions: plain C, an int status per call).
 * It lives in a header of its own because the CPU oracle (oracle/port) mirrors smarties_hip.h declaration by declaration
 * and needs no twin of this call: ol_forward_sequence, called once per agent, defines the result.
 *
 * What it replaces in the reference (paths relative to source/smarties/): what every agent's Learner::select does for its
 * action -- MemoryBuffer::agentToMinibatch (ReplayMemory/MemoryBuffer.cpp:440-467: the agent's last min(nnBPTTseq, t) + 1
 * steps become a one-sample minibatch) followed by Approximator::forward(agent) (every step of that window forwarded from a
 * zero recurrent state; the last step's output feeds the policy) -- for n agents at once instead of one at a time.
 *
 * Which call when:
 *   hl_forward            dense nets, n raw states (rows).  Up to 64 rows of a net whose layers and input rows are at most 1024 wide: one
 *                         kernel, a workgroup per row.  More rows, or a wider layer or input row (up to 2048): the many-row route -- per
 *                         chunk of HL_ACT_ROWS_CHUNK rows ONE launch in which a workgroup runs the whole net for a block of 16 rows on
 *                         the MFMA, rows and outputs through pinned host memory; the minibatch buffers are not touched and a minibatch
 *                         drawn ahead stays as it is.  Nets beyond HL_ACT_ROWS_SMALL_NET weights take it only from HL_ACT_ROWS_WIDE_MIN_N
 *                         rows and 4 x batchSize rows on (below).  Feed-forward nets with convolutional layers in front whose raw rows
 *                         are at most HL_ACT_CONV_MAX_ROW_BYTES long, any n >= 1: per chunk (HL_ACT_CONV_STAGE_BYTES below) the raw rows
 *                         go into pinned staging, then TWO launches -- the whole conv stack of a row per workgroup with every map in LDS,
 *                         the rows read from the mapped staging, the filters from the parameter blob as the reference lays them out
 *                         (right directly behind hl_set_params / hl_restart); the dense layers on the feature rows by the many-row
 *                         kernel --, completion by that kernel's stamps.  It leaves alone the minibatch buffers, the training
 *                         activations, the prepared filter copies, a minibatch drawn ahead and the stream (no synchronisation); the
 *                         choice depends on the net only, so a row's result is the same bit for bit alone, among others and through
 *                         hl_forward_sequence(s).  Conv nets that fall back: longer raw rows (RACER_atari.json's 110 KB among them: the
 *                         figures below), image, maps and offset tables beyond the 160 KB of LDS of a workgroup, a feature row
 *                         [extras | last map] or a dense layer wider than 2048, recurrent layers behind.  Everything
 *                         else (those, input rows of dense nets beyond 2048, SMARTIES_HIP_GENERIC bit 2): the
 *                         training forward launches over minibatch buffer 0, a minibatch drawn ahead dropped and drawn again.  The two
 *                         dense routes form their sums in different orders: they agree to rounding (both within 1e-5 of the CPU
 *                         oracle), not bit for bit; a row's result on the many-row route depends neither on n nor on its place.
 *   hl_forward_sequence   ONE agent's window, any net.  The cheapest call for a single agent of a recurrent net.
 *   hl_forward_sequences  n agents' windows, any net.  Per chunk of agents one launch, or -- layers wider than 256 cells, recurrent
 *                         layers behind convolutions, RNN encoder layers under MGU layers, nets of at most 256 cells whose window
 *                         is beyond the one launch's 64 KB -- one chain of hl_forward_sequence's own launches (listed below).
 *   hl_forward_dev,       dense nets, rows, actions and finished episodes that live in DEVICE memory (a simulator on the learner's GPU):
 *   hl_select_actions_dev, include/smarties_hip_dev.h.  The two acting kernels of hl_forward on the caller's arrays, ordered against the caller's
 *   hl_append_episodes_dev stream, without staging and without a host wait.
 *   hl_forward_sequences_dev,        n agents' windows that live in DEVICE memory as rows of a strided rollout buffer: recurrent nets of
 *   hl_select_actions_sequences_dev  hl_forward_sequences' one-launch route (one layer type, no convolutions, no encoder_rnn, layers up to
 *                         256 cells and 1024 inputs) -- that kernel with the windows gathered and truncated in the kernel, ONE launch
 *                         for any n, no chunks --, and the dense nets hl_forward_dev serves (appended observations stacked on the
 *                         device).  Every other recurrent net acts through hl_forward_sequences.
 */
#ifndef SMARTIES_HIP_ACT_H
#define SMARTIES_HIP_ACT_H

#include "smarties_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* agents per launch: the pinned staging of the library (states, window offsets, outputs, completion stamps) is sized once,
 * at the first acting call, for this many windows of nnBPTTseq + 1 + nAppendedObs states; a call with more agents is cut
 * into ceil(n / HL_ACT_SEQ_CHUNK) launches (the nets served by a chain of launches: chunks of min(local batch size,
 * HL_ACT_SEQ_CHUNK)) */
#define HL_ACT_SEQ_CHUNK 512
/* rows per launch of hl_forward's many-row route (dense nets): its pinned staging (raw rows, outputs, one completion stamp per
 * block of 16 rows) is sized for this many rows at the first call that takes the route; a call with more rows is cut into
 * ceil(n / HL_ACT_ROWS_CHUNK) launches */
#define HL_ACT_ROWS_CHUNK 1024
/* where hl_forward switches to the many-row route (measured on an MI355X at batchSize 256, profiles/act_rows_timing.json; us per
 * call, many-row route against the launches over the training buffers).  A workgroup streams all weights of the net for its 16
 * rows, so the call costs about 24 us + 0.146 us per 1024 weights whatever n is up to 4096, the training launches about
 * 43 us + 0.067 us per 1024 weights per round of 2 x batchSize rows:
 *     2 x 256 (74 K weights)   34 against 48 at 65 rows, 43 against 106 at 1024        -- the route wins everywhere
 *     2 x 512 (275 K weights)  64 against 62 at 65 rows, 72 against 134 at 1024         -- loses the bare call below one round
 *     3 x 1024 (2.1 M weights) 338 against 91 at 65 rows, 353 against 384 at 1024       -- wins only against two rounds
 * (The 65-row figures of 2 x 512 and 3 x 1024 are the route's with the switch held open; the profile holds what the library does:
 * the training launches there.)
 * A dense net of up to HL_ACT_ROWS_SMALL_NET weights (floats, all layers; the two lines cross at 248 K, the constant keeps a
 * margin below that) takes the route whenever the one-kernel route does not apply.  A larger net takes it only for
 * n >= HL_ACT_ROWS_WIDE_MIN_N and n >= 4 x batchSize (two rounds of the training launches; 1024 rows is the measured point, at
 * batchSize 256), and runs the training launches below that -- also for a single row of a net with a 1025 - 2048 wide layer. */
#define HL_ACT_ROWS_SMALL_NET (192 * 1024)
#define HL_ACT_ROWS_WIDE_MIN_N 1024
/* recurrent layers behind convolutions: the stacked window rows of a chunk's agents (nnBPTTseq + 1 rows of
 * dimS (1 + nAppendedObs) floats each) are staged in pinned host memory, and a chunk holds no more agents than fit this many
 * bytes (512 agents of an 84 x 84 x 4 image window would pin hundreds of megabytes), though never fewer than one */
#define HL_ACT_WIN_STAGE_BYTES (32u << 20)
/* hl_forward behind convolutions: the raw rows of a chunk (dimS (1 + nAppendedObs) floats each) are staged in pinned, device-mapped
 * host memory, and a chunk holds no more rows than fit this many bytes -- HL_ACT_ROWS_CHUNK rows of an 84 x 84 x 4 image would pin
 * 116 MB --: min(HL_ACT_ROWS_CHUNK, HL_ACT_CONV_STAGE_BYTES / row bytes) rows, rounded down to whole blocks of 16 and never below 16
 * (288 rows of 84 x 84 x 4).  The kernel reads the rows from the mapped staging itself.  The alternative, one hipMemcpyAsync from the
 * staging into a device buffer ahead of the launch, was tried during development and was slower by 11 - 24 us per call (one and 16 rows
 * of 110 KB, 16 rows of 2.3 KB); that variant is not in the tree and its run is not in the profile, so these figures cannot be
 * reproduced from the repository. */
#define HL_ACT_CONV_STAGE_BYTES (32u << 20)
/* which conv nets take the route: raw rows of at most this many bytes.  Measured on an MI355X at batchSize 128
 * (profiles/act_conv_timing.json: this build with the switch held open, SMARTIES_HIP_GENERIC=4096, against the parent commit's
 * training forward launches; us per iteration of hl_step(1) + hl_forward(n), in brackets the bare call):
 *     rows of 2.3 KB  (12 x 12 x 4, two layers)            n = 1: 119 against 153 (44 / 50), n = 1024: 190 against 435 (167 / 333)  -- wins
 *     rows of 12.5 KB (20 x 20 x 8, one layer)             n = 1: 175 against 135 (93 / 51), n = 1024: 669 against 605 (637 / 512)  -- loses
 *     rows of 27.6 KB (42 x 42 x 4, two layers)            n = 1: 272 against 212 (145 / 62), n = 1024: 1764 against 1039            -- loses
 *     rows of 110 KB  (RACER_atari.json, four layers)      n = 1: 304 against 220 (181 / 74), n = 1024: 7658 against 2628            -- loses
 * One workgroup per row is latency-bound on its row (the load over the bus, then a chain of filter loads and MFMA blocks of ONE
 * compute unit); at 1024 rows of 110 KB the call costs 7.4 us per row against 2.4 (which part of it -- the host copy into the staging,
 * the reads over the bus, the kernel -- was not measured apart).  The crossing lies between 2.3 and 12.5 KB and was not located more
 * finely: the constant sits between the two measured points, and every longer row keeps the training forward launches.  Row bytes
 * stand in for the conv work per row as well, WITHOUT a measurement of that: a net with short rows and much conv work (4.1 KB rows
 * through 32- and 64-channel layers, about ten times the MFMA steps of the measured 2.3 KB net) takes the route unmeasured. */
#define HL_ACT_CONV_MAX_ROW_BYTES (6u << 10)

/* n agents.  n_steps[i] = min(nnBPTTseq, t_i) + 1 (+ up to nAppendedObs states in front), as for hl_forward_sequence.
 * states: the windows back to back, oldest state first in each (sum of n_steps[i] rows of dimS raw floats).
 * outputs[i * nOutputs .. ]: nOutputs doubles, those of agent i's last state.
 *
 * Agent i's result is what hl_forward_sequence(h, n_steps[i], window_i, outputs_i) defines: the window forwarded from a
 * zero recurrent state, appended observations filled from the leading context states, steps before the first given state
 * repeating it (Episode::standardizedState, Episode.h:172-183); output layer, nnOutputFunc and the ParamLayer values.
 *
 * Status: HL_ERR_STATE between hl_step_begin and hl_step_end.  HL_ERR_BAD_ARG if any n_steps[i] < 1 or, for a net with
 * recurrent layers, n_steps[i] > nnBPTTseq + 1 + nAppendedObs (dense nets read the last 1 + nAppendedObs states of a window
 * of any length, as hl_forward_sequence does): nothing is launched and `outputs` is not written.  n == 0: HL_OK, the device
 * is not touched.  n has no upper limit.
 *
 * Batched (one kernel per chunk: a workgroup per agent up to the number of compute units, further agents walked by the same
 * workgroups, which stage the weights once; states and outputs through pinned host memory, completion by per-agent stamps;
 * the minibatch buffers are not touched and a minibatch drawn ahead stays as it is):
 *     nnType LSTM, MGU or RNN without convolutional layers and without encoder_rnn, every layer <= 256 cells with
 *     <= 1024 inputs, any nAppendedObs, (nnBPTTseq + 1 + nAppendedObs) x dimS floats of window within 64 KB.
 *     The gate sums are formed in another order than by hl_forward_sequence's kernels: the two agree to rounding
 *     (both within 1e-5 of the CPU oracle), not bit for bit.
 * Batched, layers wider than 256 cells (the nets whose single window hl_forward_sequence runs through the time-step-major
 * launches: LSTM, MGU or RNN without convolutional layers and without encoder_rnn, a layer above 256 cells, every layer a
 * multiple of 16 cells up to 1024): agent i of a chunk is sample row i of ONE chain of those launches -- a prepare kernel over
 * (agent, window step), the forward diagonals up to the chunk's longest window, the output layer on the chunk's rows --
 * instead of one chain per agent.  A chunk holds min(local batch size, HL_ACT_SEQ_CHUNK) agents: the chain borrows the
 * training rows of that many samples between steps (as hl_forward_sequence borrows those of one); the minibatch index
 * buffers and a minibatch drawn ahead stay as they are.  The kernels and their order of summation are those of the
 * single-agent call, an agent's row of a tile does not see the other rows: bit-identical to hl_forward_sequence.
 * Batched, wide inputs (a state beyond 256 components or dimS (1 + nAppendedObs) beyond 1024, up to 8192, in front of LSTM, MGU
 * or RNN layers of any multiple of 16 cells up to 1024; smarties_hip.h): the same chain with one launch more in front of the
 * diagonals, the first layer's input product of the chunk's agents x steps rows.  hl_forward_sequence runs that chain on its one
 * window.  A chunk holds min(local batch size, HL_ACT_SEQ_CHUNK) agents and no more than whose windows of
 * nnBPTTseq + 1 + nAppendedObs states fit HL_ACT_WIN_STAGE_BYTES of pinned staging (60 agents of 17 states of 8192 floats),
 * though never fewer than one.  An element of the product is one chain of MFMAs over its row's inputs whatever the row's
 * place in the launch: bit-identical to hl_forward_sequence.
 * Dense nets: the [n][dimS (1 + nAppendedObs)] rows are built on the host and go through ONE hl_forward(n) call.
 * Batched, every other recurrent net -- recurrent layers behind convolutions, RNN encoder layers under MGU layers (encoder_rnn),
 * nets of at most 256 cells whose window exceeds the 64 KB above; every layer <= 256 cells with <= 1024 inputs --: agent i of a
 * chunk is sample i of ONE chain of hl_forward_sequence's own launches.  Its window kernels run a workgroup per sample; here
 * workgroup i takes agent i's window from a per-agent table of offsets and lengths and walks that window alone (no padding to
 * the chunk's longest), the two launches of an encoder_rnn stack and the output layer follow on the chunk's rows.  Behind
 * convolutions the host stacks the rows of all agents of the chunk (agent i's window step k at row i (nnBPTTseq + 1) + k, the
 * rows of steps a window lacks repeating its last one) and they pass the convolutional front as one set of launches.  A chunk
 * holds min(local batch size, HL_ACT_SEQ_CHUNK) agents -- the chain borrows the training rows of that many samples -- and behind
 * convolutions no more than HL_ACT_WIN_STAGE_BYTES of staged rows allow.  The same kernels on the same rows in the same order
 * of summation: bit-identical to hl_forward_sequence.  Behind convolutions a minibatch drawn ahead is dropped and drawn again
 * with the same generator state, as by hl_forward_sequence.
 * Looped, agent by agent through hl_forward_sequence's own route: only a net beyond those bounds (more than 1024 inputs to the
 * first recurrent layer behind convolutions) which the time-step-major launches do not take either.
 *
 * For a single agent the call costs more than hl_forward_sequence (which runs the window with the weights in registers
 * where the shape allows): hl_forward_sequence stays the call for one agent. */
HL_API int hl_forward_sequences(hl_learner* h, int32_t n, const int32_t* n_steps, const float* states, double* outputs);

#ifdef __cplusplus
}
#endif
#endif
