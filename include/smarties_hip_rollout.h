/*
 * include/smarties_hip_rollout.h -- a rollout buffer for vectorised simulators on the learner's GPU: ONE call per simulator step.
 *
 * An addition to the C-ABI of include/smarties_hip.h, in a header of its own as include/smarties_hip_act.h and
 * include/smarties_hip_dev.h are (the CPU oracle mirrors smarties_hip.h declaration by declaration and needs no twin of these calls).
 *
 * hl_select_actions_sequences_dev and hl_append_episodes_dev move the DATA of the loop act -> simulate -> append -> step without
 * leaving the device; the bookkeeping around them -- a buffer that holds whole episodes, per-environment start rows and lengths, the
 * terminal row in the shape hl_append_episode documents, which environments ended, the clipped action noise -- was every caller's to
 * write.  A rollout object owns it: it holds the episodes in flight of nEnv environments in device memory, and hl_rollout_step takes the
 * simulator's current states, rewards and end flags and returns the actions to apply.  The forward pass, the action head and the
 * ingestion are the existing calls' own bodies on the same kernels: the actions equal hl_select_actions_sequences_dev's bit for bit, the
 * stored episodes hl_append_episodes_dev's.  New kernels (smarties_amd/csrc/rollout.hip) do the bookkeeping, the noise and the scatter.
 *
 * The buffer: one slab of maxSteps rows per environment; row env * maxSteps + t is state t of that environment's current episode, in the
 * types hl_append_episodes_dev takes (states f32, actions and policies f64, rewards f64, values and advantages f32).  The window calls
 * and the ingestion see first_row = env * maxSteps and row_stride = 1; row arithmetic is in 64 bits.
 */
#ifndef SMARTIES_HIP_ROLLOUT_H
#define SMARTIES_HIP_ROLLOUT_H

#include "smarties_hip_dev.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hl_rollout hl_rollout;

/* host-side numbers of a rollout (hl_rollout_info) */
typedef struct hl_rollout_counts {
  int64_t calls;        /* hl_rollout_step calls that ran */
  int64_t episodes;     /* episodes handed to the replay memory */
  int64_t steps;        /* ... and the states they hold, terminal rows included */
  int64_t capped;       /* episodes closed because they reached maxSteps states without a flag */
  int64_t no_room;      /* finished episodes dropped because the replay memory had no room for them */
} hl_rollout_counts;

/* A rollout of nEnv environments with episodes of at most maxSteps states, owned by the learner h.  `seed` keys the library's action
 * noise (below); episode number k this rollout hands to the replay memory gets the tag tag_base + k, episodes counted in call order
 * and, within a call, in ascending environment index.
 * Served: every net hl_select_actions_sequences_dev serves.  A net that call refuses is refused here, HL_ERR_UNSUPPORTED with that
 * call's message (it names hl_forward_sequences or hl_forward).
 * Status: HL_ERR_BAD_ARG for a null handle or `out`, nEnv < 1, nEnv > 65536 or maxSteps < 2 (checked without a device);
 * HL_ERR_HIP, with the byte count in the message, if the buffer cannot be allocated.
 * hl_destroy of the learner destroys the rollouts still open: their handles are dead afterwards. */
HL_API int hl_rollout_create(hl_learner* h, int32_t nEnv, int32_t maxSteps, uint64_t seed, int64_t tag_base, hl_rollout** out);
HL_API int hl_rollout_destroy(hl_rollout* r);

/* flags of hl_rollout_step */
enum { HL_ROLLOUT_EVALUATE = 1, HL_ROLLOUT_NO_STORE = 2 };

/* One simulator step of all nEnv environments.  All arrays are DEVICE memory; `stream` and the stream semantics are exactly those of
 * include/smarties_hip_dev.h (the inputs may be written by work queued on `stream` before the call, dActions is valid for work queued
 * on `stream` after it).
 *   dStates  [nEnv][dimS] f32   the state every environment is in now
 *   dRewards [nEnv] f64         the reward received on arriving there; ignored at an episode's first state, where row 0 stores 0
 *   dEnd     [nEnv] int32       0 running, 1 terminal, 2 (any other value) truncated by the environment
 *   dActions [nEnv][dimA] f64   OUT: the action to apply; zeros for an environment whose state ended its episode
 * After an environment has ended, its state in the NEXT call is the first state of a new episode (its dRewards entry is ignored, dEnd
 * applies as usual).  An episode has at most maxSteps states: one that reaches the cap without a flag is closed as truncated by the
 * bookkeeping kernel, so nothing is ever written past an environment's slab -- the cap is the CALLER'S CONTRACT: a simulator whose
 * episodes can be longer sets its own truncation flag, or sees them cut (counted in hl_rollout_counts::capped).  A state flagged at an
 * episode's first step makes an episode of one state, which holds no transition: it is not stored, the slab is reused.
 *
 * Noise.  dNoise != NULL: hl_select_actions_dev's layout, [nEnv][dimA] normal deviates already clipped to +-3 (discrete head: [nEnv]
 * uniforms in [0, 1)).  dNoise == NULL: the library's generator.  It is counter-based -- Philox4x32-10 -- so that a draw depends on
 * (seed, environment, episode, step, component) and on nothing else: not on nEnv, not on the number of calls, not on which other
 * environments ended.  The mapping, exactly (restated in tests/rollout.py, evaluated on the host by hl_rollout_noise):
 *   key      (seed mod 2^32, seed >> 32)
 *   counter  (env, episode mod 2^32, t, component + 65536 b): episode = episodes this environment has started before the current one,
 *            t = index of the state in its episode, b = 0 for the block x below and 1 for the block y
 *   U53(hi, lo) = ((hi >> 5) 2^26 + (lo >> 6)) 2^-53, in [0, 1)
 *   continuous heads  z = sqrt(-2 log(1 - U53(x0, x1))) cos(2 pi U53(x2, x3))   (Box-Muller in fp64, every operation rounded on its own);
 *                     a value beyond +-NORMDIST_MAX = 3 is replaced by (2 U53(y0, y1) - 1) 3, uniform in [-3, 3), as
 *                     Agent::sampleClippedGaussian replaces it (Core/Agent.h:321-330)
 *   discrete head     u = U53(x0, x1), component 0
 * This is NOT the reference's stream: there every agent owns an mt19937 on the host that is consumed in agent order, which has no
 * parallel form.  The distribution is the same.
 * flags: HL_ROLLOUT_EVALUATE -- evaluation actions, no noise: the head's dNoise == NULL behaviour (the mean; the arg-max option).
 *        HL_ROLLOUT_NO_STORE -- finished episodes are not handed to the replay memory (evaluation runs); the slab is simply reused.
 *
 * What a call enqueues on the learner's stream, inside the handshake with `stream`: rollout_book_kernel (state and reward rows, window
 * tables, the ended environments compacted in ascending order into mapped pinned memory), rollout_noise_kernel where the library draws,
 * the launches of hl_select_actions_sequences_dev on the slabs, rollout_store_kernel (results into row t, terminal rows, dActions),
 * and -- after ONE host poll of the bookkeeping kernel's stamp, which overlaps the forward pass; 2 s, then a stream synchronisation --
 * the launches of hl_append_episodes_dev for the episodes that ended, in chunks of 64.  The poll makes the call wait for whatever was
 * queued on the learner's stream before it, gradient steps included.  An episode that finds no room ends the batch as it does there; the
 * ones left are dropped and counted (hl_rollout_counts::no_room), hl_last_error keeps the reason, the call returns HL_OK.
 * Status: HL_ERR_BAD_ARG for a null handle or array; HL_ERR_STATE between hl_step_begin and hl_step_end; HL_ERR_UNSUPPORTED, with a
 * message naming HL_ACT_LIVE, while the acting source is HL_ACT_SNAPSHOT: the rollout writes the buffer the ingestion reads on the
 * learner's stream.  (A rollout given a staging ring, hl_rollout_staging below, is served under that source.)
 *
 * Timing (tools/rollout_timing.py, profiles/rollout_timing.json): see DESIGN.md 4.4 for the figures of that file. */
HL_API int hl_rollout_step(hl_rollout* r, const float* dStates, const double* dRewards, const int32_t* dEnd, const double* dNoise,
                           int32_t flags, double* dActions, void* stream);

/* the host-side numbers so far; no device wait */
HL_API int hl_rollout_info(hl_rollout* r, hl_rollout_counts* out);

/* ---- hl_rollout_step beside queued gradient steps: the staging ring ----
 * Gives the rollout a staging ring of `rows` rows in device memory (states f32, actions and policies f64, rewards f64, values and
 * advantages f32: the slab's types).  From then on hl_rollout_step serves HL_ACT_SNAPSHOT too.
 *
 * Under HL_ACT_SNAPSHOT the call runs on the acting stream (include/smarties_hip_dev.h: hl_act_dev_source) from the current snapshot: the
 * bookkeeping kernel, the noise, the acting launches and the store kernel are enqueued there, the caller's stream waits for exactly
 * these, and the one host poll waits for the acting stream only -- not for the gradient steps queued on the learner's.  The episodes
 * that ended leave their slabs on the acting stream, before the slabs are reused: rollout_stage_kernel copies them into the ring, in
 * batches of at most 64 episodes (one ingest launch) and at most rows / 2 rows, each batch one contiguous region; a batch that does not
 * fit between the head and the ring's end starts again at row 0.  The learner's stream waits for the batch's copy, runs
 * hl_append_episodes_dev's launch on the ring's rows -- whenever the steps queued there let it -- and records the region's `consumed`
 * event.  A region is written again only behind that event: the host QUERIES it and, where it has not completed, makes the acting
 * stream wait for it (a stall; it delays the next call's bookkeeping kernel -- and so that call's host poll: the ring bounds how far the
 * rollout runs ahead of a backlog --, never this call's actions).  The host never blocks on the ring.  Order, tags, the terminal row and hl_rollout_counts are the live call's; an episode that finds no room ends the call's
 * hand-off, later batches of that call are not staged, the rest is counted in no_room.
 * A ring that holds the episodes ending between two bursts of queued steps never stalls: rows >= (episodes per burst) * maxSteps.
 * Under HL_ACT_LIVE a rollout with a ring behaves like one without: direct ingestion from the slabs, no staging launch, the counters
 * below untouched.  A rollout without a ring is refused under HL_ACT_SNAPSHOT as before.  The source may change with episodes in flight:
 * the first call on the other stream waits for an event behind everything the last call enqueued.
 * Known limits: hl_step after new episodes still waits for the learner's stream when it uploads the episode table; with
 * hl_set_episode_log on, the ingestion reads the episodes' sums back behind the queued steps; a replay memory that has to grow for an
 * episode waits for the learner's stream as it does in every appending call.
 * Status: HL_ERR_BAD_ARG for a null handle (checked without a device), rows < 2 * maxSteps or rows >= 2^31; HL_ERR_STATE if the rollout
 * already has a ring; HL_ERR_UNSUPPORTED, with a message naming HL_ACT_LIVE, for a net whose window route the snapshot source refuses
 * (recurrent nets on wide inputs); HL_ERR_HIP, with the byte count in the message, if the ring cannot be allocated.
 * hl_rollout_step under HL_ACT_SNAPSHOT, before its first launch: HL_ERR_STATE naming hl_policy_snapshot before any snapshot exists;
 * HL_ERR_STATE between hl_step_begin and hl_step_end.
 * hl_rollout_read and hl_rollout_destroy of a rollout with a ring wait for both streams.
 * Timing (tools/rollout_snapshot_timing.py, profiles/rollout_snapshot_timing.json): see DESIGN.md 4.4. */
HL_API int hl_rollout_staging(hl_rollout* r, int64_t rows);

typedef struct hl_rollout_stage_counts {
  int64_t capacity;   /* rows of the ring (0: none) */
  int64_t batches;    /* staging launches so far */
  int64_t episodes;   /* episodes copied into the ring */
  int64_t rows;       /* ... and their rows */
  int64_t wraps;      /* batches that started again at row 0 */
  int64_t stalls;     /* batches whose region was not yet consumed when the host queried its event: the acting stream was made to wait */
} hl_rollout_stage_counts;
HL_API int hl_rollout_stage_info(hl_rollout* r, hl_rollout_stage_counts* out);   /* host numbers, no device wait */

/* Diagnostics and tests (waits for the learner's stream): environment env's slab as it is.  *nStates: states of its episode in flight;
 * every array, each optional (NULL), receives ALL maxSteps rows of the slab -- rows below *nStates belong to the episode in flight, the
 * ones behind them are what earlier episodes left: states [maxSteps][dimS], actions [maxSteps][dimA], mu [maxSteps][polDim],
 * rewards, values, advantages [maxSteps]. */
HL_API int hl_rollout_read(hl_rollout* r, int32_t env, int32_t* nStates, float* states, double* actions, double* mu, double* rewards,
                           float* values, float* advantages);

/* The library's draw for (seed, env, episode, t, component) evaluated on the HOST by the text the device compiles (discrete != 0: the
 * uniform of the discrete head).  The Philox block is the device's bit for bit; the normal deviate goes through the host's log, cos and
 * sqrt, which may differ from the device's in the last places.  Needs no device.  HL_ERR_BAD_ARG for a null `out` or a negative index. */
HL_API int hl_rollout_noise(uint64_t seed, int32_t env, int64_t episode, int32_t t, int32_t component, int32_t discrete, double* out);

#ifdef __cplusplus
}
#endif
#endif
