// smarties_amd/csrc/learner_rollout.h -- part of learner.cpp's ONE translation unit (included there, behind learner_dev.h): the rollout buffer of a vectorised simulator on the learner's GPU: hl_rollout_create, hl_rollout_destroy, hl_rollout_step, hl_rollout_info, hl_rollout_read, hl_rollout_noise; its staging ring, which lets the call run under the snapshot source: hl_rollout_staging, hl_rollout_stage_info
#pragma once
#include "../../include/smarties_hip_rollout.h"
#include "rollout_rng.h"
#include "rollout_ring.h"
static_assert(ROLLOUT_MAX_ENV == 65536, "the bound on nEnv the header states");
static_assert(RING_BATCH_EP == INGEST_DEV_MAX_EP && RING_BATCH_EP == ROLLOUT_STAGE_MAX_EP, "a batch of the ring is one staging launch and one ingest launch");

// One device block carved into the slabs [nEnv maxSteps] rows, the per-environment tables and the head's contiguous scratch; one mapped
// pinned block for the table of ended episodes the bookkeeping kernel writes (kernels.h: RolloutBookArgs)
struct hl_rollout {
  hl_learner* h = nullptr;
  int nEnv = 0, maxSteps = 0; uint64_t seed = 0; int64_t tagBase = 0;
  unsigned char* dev = nullptr; size_t devBytes = 0;
  float* S = nullptr; double *A = nullptr, *MU = nullptr, *R = nullptr; float *V = nullptr, *ADV = nullptr;      // the slabs
  int *len = nullptr, *episode = nullptr, *nSteps = nullptr, *kind = nullptr; long long* firstRow = nullptr;     // [nEnv]
  double *noise = nullptr, *act = nullptr, *mu = nullptr; float *v = nullptr, *adv = nullptr;                    // [nEnv] rows, contiguous
  int* host = nullptr; unsigned tag = 0;
  hl_rollout_counts counts{};
  // The staging ring (hl_rollout_staging): one device block carved into the six arrays of `capacity` rows.  Under the snapshot source an
  // ended episode leaves its slab on the acting stream (rollout_stage_kernel) before the slab is reused, and reaches the replay memory from
  // the ring on the learner's stream, whenever the steps queued there let it.  `staged`: recorded on the acting stream behind a batch's
  // copy, the learner's stream waits for it; a region's `consumed` event (RingRegion::event indexes `events`): recorded on the learner's
  // stream behind the ingest launch that read it, the acting stream waits for it before it writes those rows again
  unsigned char* ringDev = nullptr;
  float* gS = nullptr; double *gA = nullptr, *gMU = nullptr, *gR = nullptr; float *gV = nullptr, *gADV = nullptr;
  RolloutRing ring;
  std::vector<hipEvent_t> events; std::vector<int> freeEvents;      // the pool of `consumed` events
  hipEvent_t staged = nullptr;
  hl_rollout_stage_counts stage{};
  // a rollout with a ring remembers the stream of its last call and an event behind all that call enqueued there: the other source's first
  // call waits for it
  hipStream_t lastStream = nullptr; hipEvent_t lastEv = nullptr;
};

extern "C++" {
namespace {
void rolloutFree(hl_rollout* r) {
  if (r->dev) hipFree(r->dev);
  if (r->ringDev) hipFree(r->ringDev);
  if (r->host) hipHostFree(r->host);
  for (hipEvent_t ev : r->events) hipEventDestroy(ev);
  if (r->staged) hipEventDestroy(r->staged);
  if (r->lastEv) hipEventDestroy(r->lastEv);
  delete r;
}
// an event of the pool (a new one where none is free); -1: the runtime refused
int rolloutEventTake(hl_rollout* r) {
  if (!r->freeEvents.empty()) { const int i = r->freeEvents.back(); r->freeEvents.pop_back(); return i; }
  hipEvent_t ev = nullptr;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return -1;
  r->events.push_back(ev);
  return (int)r->events.size() - 1;
}
void rolloutReleaseAll(hl_learner* h) {
  for (hl_rollout* r : h->rollouts) rolloutFree(r);
  h->rollouts.clear();
}
// The hand-off of a snapshot call's ended episodes (ascending environment order, as the bookkeeping kernel listed them), batch by batch
// (rollout_ring.h): the region's rows are free once the regions it takes over are consumed -- queried, never waited for on the host: the
// acting stream waits for the ones still being read (a stall; it holds back this copy and what the next call enqueues, not this call's
// actions, which the caller's stream has been handed already) --; rollout_stage_kernel on the acting stream; `staged` behind it, which
// the learner's stream waits for; the ingestion's own body on the ring's rows; `consumed` behind it.  No cycle: a region's `consumed`
// follows its `staged`, and its `staged` precedes every later copy.  An episode that finds no room ends the call's hand-off as it ends
// the live call's ingestion
int rolloutHandOff(hl_rollout* r, hipStream_t actSt, int nEnded, const int* envs, const int32_t* ns, const int32_t* term, const int64_t* tags, void* stream) {
  hl_learner* h = r->h;
  if (!r->staged) HIPCK(hipEventCreateWithFlags(&r->staged, hipEventDisableTiming));
  std::vector<RingRegion> released;
  int64_t first[RING_BATCH_EP];
  for (int k0 = 0; k0 < nEnded;) {
    int64_t rows = 0;
    const int m = ringBatch(ns + k0, nEnded - k0, r->ring.capacity, &rows);
    if (m < 1) return fail(h, HL_ERR_HIP, "hl_rollout_step: an episode longer than half the staging ring");      // (2 maxSteps <= capacity: never)
    const int ev = rolloutEventTake(r);
    if (ev < 0) return fail(h, HL_ERR_HIP, "hl_rollout_step: no event for a region of the staging ring");
    bool wrapped = false, stalled = false;
    const int64_t dst = r->ring.place(rows, ev, &wrapped, &released);
    for (const RingRegion& g : released) {
      const hipError_t q = hipEventQuery(r->events[(size_t)g.event]);
      if (q == hipErrorNotReady) {
        (void)hipGetLastError();      // (not an error: the launchers below read the thread's last one)
        stalled = true;
        HIPCK(hipStreamWaitEvent(actSt, r->events[(size_t)g.event], 0));
      } else HIPCK(q);
      r->freeEvents.push_back(g.event);      // (a wait holds the record it was given: the event may be recorded anew)
    }
    RolloutStageArgs sa{r->S, r->A, r->MU, r->R, r->V, r->ADV, r->gS, r->gA, r->gMU, r->gR, r->gV, r->gADV, (long long)r->ring.capacity,
                        r->nEnv, r->maxSteps, h->dS, h->dA, h->polDim, m, {}};
    int64_t at = dst;
    for (int k = 0; k < m; ++k) { sa.ep[k] = RolloutStageEp{envs[k0 + k], ns[k0 + k], (long long)at}; first[k] = at; at += ns[k0 + k]; }
    HIPCK(timed(h, "rollout_stage_kernel", actSt, [&] { return launch_rollout_stage(sa, actSt); }));
    ++r->stage.batches; r->stage.episodes += m; r->stage.rows += rows; r->stage.wraps += wrapped ? 1 : 0; r->stage.stalls += stalled ? 1 : 0;
    HIPCK(hipEventRecord(r->staged, actSt));
    HIPCK(hipStreamWaitEvent(h->stream, r->staged, 0));
    int booked = -1;
    const int rc = devIngest(h, m, ns + k0, term + k0, tags + k0, first, 1, r->gS, r->gA, r->gMU, r->gR, r->gV, r->gADV, stream, /*handshake*/false, &booked);
    if (booked < 0) return rc ? rc : HL_ERR_HIP;      // (the body returned before its launches were out)
    HIPCK(hipEventRecord(r->events[(size_t)ev], h->stream));
    for (int k = 0; k < booked; ++k) r->counts.steps += ns[k0 + k];
    r->counts.episodes += booked;
    if (booked < m) { r->counts.no_room += nEnded - k0 - booked; break; }      // (rc: why; hl_last_error keeps it.  The batches left are not staged)
    k0 += m;
  }
  return HL_OK;
}
}  // namespace
}  // extern "C++"

int hl_rollout_create(hl_learner* h, int32_t nEnv, int32_t maxSteps, uint64_t seed, int64_t tag_base, hl_rollout** out) {
  if (!h || !out || nEnv < 1 || nEnv > ROLLOUT_MAX_ENV || maxSteps < 2) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  const ActRoutes& rt = actResolve(h);
  if (rt.devSeq == ACT_DEV_SEQ_NONE) return fail(h, HL_ERR_UNSUPPORTED, "hl_rollout_create" + rt.devSeqNo);
  hl_rollout* r = new hl_rollout();
  r->h = h; r->nEnv = nEnv; r->maxSteps = maxSteps; r->seed = seed; r->tagBase = tag_base;
  // the carve: every array on a multiple of 256 bytes
  const size_t rows = (size_t)nEnv * maxSteps, n = (size_t)nEnv, dS = (size_t)h->dS, dA = (size_t)h->dA, pD = (size_t)h->polDim;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
  const size_t oS = take(rows * dS * 4), oA = take(rows * dA * 8), oMU = take(rows * pD * 8), oR = take(rows * 8), oV = take(rows * 4), oADV = take(rows * 4);
  const size_t oLen = take(n * 4), oEp = take(n * 4), oNs = take(n * 4), oKind = take(n * 4), oFirst = take(n * 8);
  const size_t oNoise = take(n * dA * 8), oAct = take(n * dA * 8), oMu = take(n * pD * 8), oVs = take(n * 4), oAdv = take(n * 4);
  r->devBytes = at;
  hipError_t e = hipMalloc((void**)&r->dev, at);
  if (e == hipSuccess) e = hipMemset(r->dev, 0, at);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);      // (devAlloc: the fill has run before the learner's stream writes)
  if (e != hipSuccess) {
    if (r->dev) hipFree(r->dev);
    delete r;
    return fail(h, HL_ERR_HIP, "hl_rollout_create: " + std::to_string(at) + " bytes of device memory: " + hipGetErrorString(e));
  }
  const size_t hostBytes = ((size_t)ROLLOUT_HOST_HEAD + 3 * n) * sizeof(int);
  e = actPinAlloc(reinterpret_cast<unsigned char**>(&r->host), hostBytes);
  if (e != hipSuccess) {
    hipFree(r->dev); delete r;
    return fail(h, HL_ERR_HIP, "hl_rollout_create: " + std::to_string(hostBytes) + " bytes of pinned host memory: " + hipGetErrorString(e));
  }
  unsigned char* b = r->dev;
  r->S = (float*)(b + oS); r->A = (double*)(b + oA); r->MU = (double*)(b + oMU); r->R = (double*)(b + oR); r->V = (float*)(b + oV); r->ADV = (float*)(b + oADV);
  r->len = (int*)(b + oLen); r->episode = (int*)(b + oEp); r->nSteps = (int*)(b + oNs); r->kind = (int*)(b + oKind); r->firstRow = (long long*)(b + oFirst);
  r->noise = (double*)(b + oNoise); r->act = (double*)(b + oAct); r->mu = (double*)(b + oMu); r->v = (float*)(b + oVs); r->adv = (float*)(b + oAdv);
  h->rollouts.push_back(r);
  *out = r;
  return HL_OK;
}

int hl_rollout_destroy(hl_rollout* r) {
  if (!r) return HL_OK;
  hl_learner* h = r->h;
  HL_LOCK(h);
  if (h->stream) hipStreamSynchronize(h->stream);      // the launches that read or write the buffer
  if (r->ringDev) actSnapSync(h);                      // ... a rollout with a ring: on the acting stream too
  h->rollouts.erase(std::remove(h->rollouts.begin(), h->rollouts.end(), r), h->rollouts.end());
  rolloutFree(r);
  return HL_OK;
}

int hl_rollout_step(hl_rollout* r, const float* dStates, const double* dRewards, const int32_t* dEnd, const double* dNoise, int32_t flags,
                    double* dActions, void* stream) {
  if (!r || !dStates || !dRewards || !dEnd || !dActions) return HL_ERR_BAD_ARG;
  hl_learner* h = r->h;
  HL_LOCK(h);
  if (h->inStep) return fail(h, HL_ERR_STATE, "hl_rollout_step between hl_step_begin and hl_step_end");
  const bool snap = h->act.source == HL_ACT_SNAPSHOT;
  if (snap && !r->ringDev)
    return fail(h, HL_ERR_UNSUPPORTED, "hl_rollout_step: the rollout writes the buffer the ingestion reads on the learner's stream: it is served by the source HL_ACT_LIVE only");
  if (snap) { int rc = devSnapEnsure(h, "hl_rollout_step"); if (rc) return rc; }      // (no snapshot yet: refused; the acting stream, before the context copies it)
  const int n = r->nEnv;
  // the stream of the call: the learner's, or (a rollout with a ring under the snapshot source) the acting stream beside the steps queued there
  const DevCtx d = devCtx(h, snap ? HL_ACT_SNAPSHOT : HL_ACT_LIVE);
  { int rc = devEnter(h, d, stream); if (rc) return rc; }
  if (r->ringDev) {      // the source changed with episodes in flight: behind all the last call enqueued on the other stream
    if (!r->lastEv) HIPCK(hipEventCreateWithFlags(&r->lastEv, hipEventDisableTiming));
    if (r->lastStream && r->lastStream != d.st) HIPCK(hipStreamWaitEvent(d.st, r->lastEv, 0));
  }
  // 1. the bookkeeping in front of the forward pass; its stamp is polled below
  if (++r->tag == 0) ++r->tag;      // (0 is what a fresh block holds)
  const RolloutBookArgs ba{dStates, dRewards, dEnd, r->S, r->R, r->len, r->firstRow, r->nSteps, r->kind, r->host, r->tag, n, r->maxSteps, h->dS};
  HIPCK(timed(h, "rollout_book_kernel", d.st, [&] { return launch_rollout_book(ba, d.st); }));
  // 2. the noise: none (evaluation), the caller's, or the library's draw
  const double* noise = (flags & HL_ROLLOUT_EVALUATE) ? nullptr : dNoise;
  if (!(flags & HL_ROLLOUT_EVALUATE) && !dNoise) {
    const RolloutNoiseArgs na{r->noise, r->nSteps, r->episode, (unsigned long long)r->seed, n, h->dA, h->nOpt > 0 ? 1 : 0};
    HIPCK(timed(h, "rollout_noise_kernel", d.st, [&] { return launch_rollout_noise(na, d.st); }));
    noise = r->noise;
  }
  // 3. hl_select_actions_sequences_dev's body on the slabs: windows of row stride 1 from env * maxSteps on, t + 1 states long
  const DevWindows w{reinterpret_cast<const int64_t*>(r->firstRow), r->nSteps, 1};
  const DevHeadIo head{noise, r->act, r->mu, r->v, r->adv};
  { int rc = devAct(h, "hl_rollout_step", n, r->S, &w, nullptr, &head, stream, /*handshake*/false); if (rc) return rc; }
  // 4. the results into row t, the terminal rows, the actions out
  const RolloutStoreArgs sa{r->act, r->mu, r->v, r->adv, r->A, r->MU, r->V, r->ADV, dActions, r->len, r->episode, r->nSteps, r->kind, n, r->maxSteps, h->dA, h->polDim};
  HIPCK(timed(h, "rollout_store_kernel", d.st, [&] { return launch_rollout_store(sa, d.st); }));
  // (snapshot source: the caller's stream waits for this much -- the actions --, not for the hand-off below; the snapshot buffer is read)
  if (snap) { int rc = devLeave(h, d, stream); if (rc) return rc; }
  // 5. the episodes that ended, as the bookkeeping kernel listed them, while 3. and 4. run.  The poll falls back to the CALL'S stream:
  // under the snapshot source it does not wait for the gradient steps queued on the learner's
  { int rc = actWaitOn(h, d.st, reinterpret_cast<volatile unsigned*>(r->host), 1, r->tag); if (rc) return rc; }
  const int nEnded = r->host[1];
  ++r->counts.calls; r->counts.capped += r->host[2];
  if (nEnded < 0 || nEnded > n) return fail(h, HL_ERR_HIP, "hl_rollout_step: the bookkeeping kernel's table is out of range");
  if (nEnded > 0 && !(flags & HL_ROLLOUT_NO_STORE)) {
    std::vector<int32_t> ns((size_t)nEnded), term((size_t)nEnded);
    std::vector<int64_t> tags((size_t)nEnded), first((size_t)nEnded);
    std::vector<int> envs((size_t)nEnded);
    const int* t = r->host + ROLLOUT_HOST_HEAD;
    for (int k = 0; k < nEnded; ++k) {
      const int env = t[3 * k];
      if (env < 0 || env >= n || t[3 * k + 1] < 2 || t[3 * k + 1] > r->maxSteps) return fail(h, HL_ERR_HIP, "hl_rollout_step: the bookkeeping kernel's table is out of range");
      ns[(size_t)k] = t[3 * k + 1]; term[(size_t)k] = t[3 * k + 2] == 1 ? 1 : 0; envs[(size_t)k] = env;
      tags[(size_t)k] = r->tagBase + r->counts.episodes + k; first[(size_t)k] = (int64_t)env * r->maxSteps;
    }
    if (snap) {      // out of the slabs on this stream, into the replay memory on the learner's
      const int rc = rolloutHandOff(r, d.st, nEnded, envs.data(), ns.data(), term.data(), tags.data(), stream); if (rc) return rc;
    } else {
      int booked = -1;
      const int rc = devIngest(h, nEnded, ns.data(), term.data(), tags.data(), first.data(), 1, r->S, r->A, r->MU, r->R, r->V, r->ADV, stream, /*handshake*/false, &booked);
      if (booked < 0) return rc ? rc : HL_ERR_HIP;      // (the body returned before its launches were out)
      for (int k = 0; k < booked; ++k) r->counts.steps += ns[(size_t)k];
      r->counts.episodes += booked; r->counts.no_room += nEnded - booked;      // (rc: why the ones left found no room; hl_last_error keeps it)
    }
  }
  if (r->ringDev) { HIPCK(hipEventRecord(r->lastEv, d.st)); r->lastStream = d.st; }
  return snap ? HL_OK : devLeave(h, d, stream);
}

int hl_rollout_staging(hl_rollout* r, int64_t rows) {
  if (!r) return HL_ERR_BAD_ARG;
  hl_learner* h = r->h;
  HL_LOCK(h);
  if (rows < 2 * (int64_t)r->maxSteps || rows >= ((int64_t)1 << 31)) return fail(h, HL_ERR_BAD_ARG, "hl_rollout_staging: a ring of fewer than 2 maxSteps rows, or of 2^31 and more");
  if (r->ringDev) return fail(h, HL_ERR_STATE, "hl_rollout_staging: the rollout has a staging ring already");
  if (!actResolve(h).devSeqSnap) return fail(h, HL_ERR_UNSUPPORTED, "hl_rollout_staging: recurrent nets on wide inputs act over the training buffers, which cannot run beside a gradient step: they are served by the source HL_ACT_LIVE only");
  // the carve of the slabs, on `rows` rows
  const size_t n = (size_t)rows, dS = (size_t)h->dS, dA = (size_t)h->dA, pD = (size_t)h->polDim;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
  const size_t oS = take(n * dS * 4), oA = take(n * dA * 8), oMU = take(n * pD * 8), oR = take(n * 8), oV = take(n * 4), oADV = take(n * 4);
  const hipError_t e = hipMalloc((void**)&r->ringDev, at);
  if (e != hipSuccess) {
    r->ringDev = nullptr;
    return fail(h, HL_ERR_HIP, "hl_rollout_staging: " + std::to_string(at) + " bytes of device memory: " + hipGetErrorString(e));
  }
  unsigned char* b = r->ringDev;
  r->gS = (float*)(b + oS); r->gA = (double*)(b + oA); r->gMU = (double*)(b + oMU); r->gR = (double*)(b + oR); r->gV = (float*)(b + oV); r->gADV = (float*)(b + oADV);
  r->ring = RolloutRing{}; r->ring.capacity = rows;
  r->stage = hl_rollout_stage_counts{}; r->stage.capacity = rows;
  return HL_OK;
}

int hl_rollout_stage_info(hl_rollout* r, hl_rollout_stage_counts* out) {
  if (!r || !out) return HL_ERR_BAD_ARG;
  HL_LOCK_RAW(r->h);      // (nothing is enqueued)
  *out = r->stage;
  return HL_OK;
}

int hl_rollout_info(hl_rollout* r, hl_rollout_counts* out) {
  if (!r || !out) return HL_ERR_BAD_ARG;
  HL_LOCK_RAW(r->h);      // (nothing is enqueued)
  *out = r->counts;
  return HL_OK;
}

int hl_rollout_read(hl_rollout* r, int32_t env, int32_t* nStates, float* states, double* actions, double* mu, double* rewards, float* values, float* advantages) {
  if (!r || env < 0 || env >= r->nEnv) return HL_ERR_BAD_ARG;
  hl_learner* h = r->h;
  HL_LOCK(h);
  const size_t T = (size_t)r->maxSteps, row = (size_t)env * T;
  if (r->ringDev && h->act.snapStream) HIPCK(hipStreamSynchronize(h->act.snapStream));      // a rollout with a ring: its snapshot calls wrote the slab there
  auto get = [&](void* dst, const void* src, size_t bytes) { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess; };
  HIPCK(get(nStates, r->len + env, sizeof(int)));
  HIPCK(get(states, r->S + row * h->dS, T * h->dS * sizeof(float)));
  HIPCK(get(actions, r->A + row * h->dA, T * h->dA * sizeof(double)));
  HIPCK(get(mu, r->MU + row * h->polDim, T * h->polDim * sizeof(double)));
  HIPCK(get(rewards, r->R + row, T * sizeof(double)));
  HIPCK(get(values, r->V + row, T * sizeof(float)));
  HIPCK(get(advantages, r->ADV + row, T * sizeof(float)));
  HIPCK(hipStreamSynchronize(h->stream));
  return HL_OK;
}

int hl_rollout_noise(uint64_t seed, int32_t env, int64_t episode, int32_t t, int32_t component, int32_t discrete, double* out) {
  if (!out || env < 0 || episode < 0 || t < 0 || component < 0 || component >= 65536) return HL_ERR_BAD_ARG;
  *out = hl::rolloutDraw(seed, (uint32_t)env, (uint32_t)episode, (uint32_t)t, (uint32_t)component, discrete != 0);
  return HL_OK;
}
