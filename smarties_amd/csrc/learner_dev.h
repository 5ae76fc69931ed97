// smarties_amd/csrc/learner_dev.h -- part of learner.cpp's ONE translation unit (included there, behind learner_act.h): acting and episode ingestion from device memory: hl_forward_dev, hl_select_actions_dev, hl_forward_sequences_dev, hl_select_actions_sequences_dev, hl_append_episodes_dev; acting on a policy snapshot beside queued gradient steps: hl_policy_snapshot, hl_policy_snapshot_info, hl_act_dev_source
#pragma once
#include "../../include/smarties_hip_dev.h"
static_assert(ACT_DEV_MAX_ROW == HL_ACT_DEV_MAX_ROW, "the row bound of the device calls the header states");
static_assert(HL_MAX_DIMA <= 64, "ActHeadArgs::bounded holds one bit per action component");

extern "C++" {
// Where an acting call runs and what it reads (hl_act_dev_source).  HL_ACT_LIVE: the learner's stream, the live blob and standardisation, the
// scratch of ActState -- everything as it was before the sources existed.  HL_ACT_SNAPSHOT: the acting stream, the current snapshot buffer,
// the scratch set ActState::snap; nothing the two streams share is writable
struct DevCtx {
  hipStream_t st; bool snap;
  const float *W, *stMean, *stScale;
  hipEvent_t *in, *done;
  unsigned* tag; unsigned** stamps;
  double** out; size_t* outCap; float** rows; size_t* rowsCap; float** feat; size_t* featCap;
};
static size_t snapMeanOff(const hl_learner* h) { return (size_t)h->nParams; }
static size_t snapScaleOff(const hl_learner* h) { return (size_t)h->nParams + (size_t)roundUp(h->dS, 4); }
static DevCtx devCtx(hl_learner* h, int source) {
  ActState& s = h->act;
  if (source == HL_ACT_SNAPSHOT) {
    const float* b = s.snapCur >= 0 ? s.snapBuf[s.snapCur] : nullptr;
    return DevCtx{s.snapStream, true, b, b ? b + snapMeanOff(h) : nullptr, b ? b + snapScaleOff(h) : nullptr, &s.snapIn, &s.snapDone,
                  &s.snap.tag, &s.snap.stamps, &s.snap.out, &s.snap.outCap, &s.snap.rows, &s.snap.rowsCap, &s.snap.feat, &s.snap.featCap};
  }
  return DevCtx{h->stream, false, h->W, h->rp.stMean, h->rp.stScale, &s.devIn, &s.devDone,
                &s.tag, &s.devStamps, &s.devOut, &s.devOutCap, &s.devRows, &s.devRowsCap, &s.devFeat, &s.devFeatCap};
}
// a cached plan's three pointers into the learner's mutable state, as actFillShared sets them (rows standardised already keep their nullptr)
template <typename A> static void devSource(const DevCtx& d, A& a) {
  a.W = d.W;
  if (a.stMean) { a.stMean = d.stMean; a.stScale = d.stScale; }
}
static unsigned devNextTag(const DevCtx& d) { if (++*d.tag == 0) ++*d.tag; return *d.tag; }      // (actNextTag on the source's own counter)
// the handshake with the caller's stream: the source's stream waits for what the caller queued so far -- and, under the snapshot source, for
// the copy into the current buffer (nothing else of the learner's stream) ...
static int devEnter(hl_learner* h, const DevCtx& d, void* stream) {
  if (!*d.in) HIPCK(hipEventCreateWithFlags(d.in, hipEventDisableTiming));
  if (!*d.done) HIPCK(hipEventCreateWithFlags(d.done, hipEventDisableTiming));
  HIPCK(hipEventRecord(*d.in, static_cast<hipStream_t>(stream)));
  HIPCK(hipStreamWaitEvent(d.st, *d.in, 0));
  if (d.snap) HIPCK(hipStreamWaitEvent(d.st, h->act.snapReady[h->act.snapCur], 0));
  return HL_OK;
}
// ... and what the caller queues from here on waits for the call's work; the host waits for neither.  Snapshot source: the event the next
// copy into the buffer just read waits for
static int devLeave(hl_learner* h, const DevCtx& d, void* stream) {
  HIPCK(hipEventRecord(*d.done, d.st));
  HIPCK(hipStreamWaitEvent(static_cast<hipStream_t>(stream), *d.done, 0));
  if (d.snap) { HIPCK(hipEventRecord(h->act.snapRead[h->act.snapCur], d.st)); h->act.snapReadSet[h->act.snapCur] = true; }
  return HL_OK;
}
// a device buffer of at least `need` elements (a larger one replaces it once the stream that uses it is done with the old one: the acting
// stream for the snapshot source's set, so that a growing call does not wait for the gradient steps queued on the learner's)
template <typename T> static int devEnsure(hl_learner* h, hipStream_t user, T** p, size_t* cap, size_t need) {
  if (need <= *cap) return HL_OK;
  if (*p) { HIPCK(hipStreamSynchronize(user)); hipFree(*p); *p = nullptr; *cap = 0; }
  HIPCK(devAlloc(p, need)); *cap = need;
  return HL_OK;
}
// the scratch block the dense acting kernels stamp, allocated once per source
static int devStampsEnsure(hl_learner* h, const DevCtx& d) {
  if (!*d.stamps) HIPCK(devAlloc(d.stamps, (size_t)std::max(ACT_MAXROWS, act_rows_blocks(ACT_ROWS_CHUNK))));
  return HL_OK;
}
// the snapshot source serves a call once a snapshot exists; its stream is created at first use, with default priority
// -- BEFORE the call's DevCtx is built, which copies the stream
static int devSnapEnsure(hl_learner* h, const char* who) {
  if (h->act.source != HL_ACT_SNAPSHOT) return HL_OK;
  if (h->act.snapCur < 0) return fail(h, HL_ERR_STATE, std::string(who) + ": the snapshot source before any snapshot was taken (hl_policy_snapshot)");
  if (!h->act.snapStream) HIPCK(hipStreamCreateWithFlags(&h->act.snapStream, hipStreamNonBlocking));
  return HL_OK;
}
// the windows of a device window call: agent i's newest states from row firstRow[i] on, rowStride rows apart (nullptr in their place: a row call)
struct DevWindows { const int64_t* firstRow; const int32_t* nSteps; int64_t rowStride; };
// the row-block kernel per chunk of ACT_ROWS_CHUNK rows [n][ldIn] in device memory: act_rows_kernel, or (panel) act_rows_panel_kernel, which
// stages the first layer's input row in panels
static int devRows(hl_learner* h, const DevCtx& d, const ActRowsArgs& plan, bool panel, int n, const float* in, size_t ldIn, double* out) {
  for (int r0 = 0; r0 < n; r0 += ACT_ROWS_CHUNK) {
    ActRowsArgs a = plan; devSource(d, a);
    a.in = in + (size_t)r0 * ldIn; a.out = out + (size_t)r0 * h->nOut; a.done = *d.stamps; a.n = std::min(ACT_ROWS_CHUNK, n - r0); a.tag = devNextTag(d);
    if (panel) HIPCK(timed(h, "act_rows_panel_dev", d.st, [&] { return launch_act_rows_panel(a, d.st); }));
    else HIPCK(timed(h, "act_rows_dev", d.st, [&] { return launch_act_rows(a, d.st); }));
  }
  return HL_OK;
}
// hl_forward's kernels on device rows, enqueued on the source's stream: up to ACT_MAXROWS rows of a net within the one-kernel route's
// bounds that kernel (as hl_forward picks it: the same bits), everything else the row-block kernel per chunk of ACT_ROWS_CHUNK rows (input
// rows beyond ACT_ROWS_MAXW: its panelled form)
static int devForward(hl_learner* h, const ActRoutes& r, const DevCtx& d, int n, const float* in, double* out) {
  const ActDevRowsRoute route = actDevRowsRoute(r, n);
  if (route == ACT_DEV_ROWS_FEW) {
    ActArgs aa = actFewArgs(h, in, out, *d.stamps, devNextTag(d)); devSource(d, aa);
    HIPCK(timed(h, "act_forward_dev", d.st, [&] { return launch_act_forward(aa, n, d.st); }));
    return HL_OK;
  }
  return devRows(h, d, *r.devRows, route == ACT_DEV_ROWS_PANEL, n, in, h->dIn, out);
}
static_assert(sizeof(long long) == sizeof(int64_t), "the row tables are passed on as they come");
// n windows of a recurrent net on wide inputs: agents in chunks of min(local batch, ACT_SEQ_CHUNK) -- the chain borrows the training rows of that many samples between
// steps, as actTmChain does; nothing is staged, so no stage-bytes cap -- each chunk the prepare launch on the tables at its offset, the input
// product and the chain over all recWin steps (the host does not know the windows: an agent whose window has ended is left out by the
// forward tiles), the output layer on the chunk's rows of Yout straight into `out`.  All chunks back to back in ONE timed bracket.
// Live source only (devAct)
static int devSeqTmForward(hl_learner* h, int n, const int64_t* firstRow, const int32_t* nSteps, int64_t rowStride, const float* states, double* out) {
  const int cap = std::min(h->B, ACT_SEQ_CHUNK);
  for (int m : {std::min(cap, n), n % cap})      // the two chunk sizes of the call
    if (m > 0 && !rec_tm_act_ok(actRecArgs(h, -1, m, states, nSteps, nSteps, h->recWin, 0)))
      return fail(h, HL_ERR_UNSUPPORTED, "hl_forward_sequences_dev: the time-step-major launches refuse the chunk");
  HIPCK(timed(h, "act_tm_dev", h->stream, [&] {
    for (int i0 = 0; i0 < n; i0 += cap) {
      const int m = std::min(cap, n - i0);
      // (actOff / actCnt: the many-agent form's marks for the host side of the launches; the kernels read the tables of TmActDev)
      const RecArgs ra = actRecArgs(h, -1, m, states, nSteps + i0, nSteps + i0, h->recWin, 0);
      const TmActDev t{reinterpret_cast<const long long*>(firstRow) + i0, nSteps + i0, rowStride};
      hipError_t e = launch_rec_tm_act_dev(ra, t, h->stream); if (e != hipSuccess) return e;
      e = actOutput(h, m, out + (size_t)i0 * h->nOut, nullptr, 0); if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }));
  return HL_OK;
}
// n windows of the caller's device arrays, enqueued on the source's stream.  Recurrent nets: ONE launch of the batched window kernel, which
// gathers and truncates the windows itself (no staging, so no chunks); on wide inputs the chain above.  Behind convolutions: ONE launch of the
// conv-stack kernel, which reads every agent's stacked row from its window's states, then the row-block kernel on the feature rows per chunk of
// ACT_ROWS_CHUNK (hl_forward's two launches without the staging).  Dense nets: the agents' stacked rows built by one small launch, then devForward on them
static int devSeqForward(hl_learner* h, const ActRoutes& r, const DevCtx& d, int n, const DevWindows& w, const float* states, double* out) {
  const long long* firstRow = reinterpret_cast<const long long*>(w.firstRow);
  switch (r.devSeq) {
  case ACT_DEV_SEQ_TM: return devSeqTmForward(h, n, w.firstRow, w.nSteps, w.rowStride, states, out);
  case ACT_DEV_SEQ_BATCHED: {
    ActSeqArgs a = r.seqArgs; devSource(d, a);
    a.states = states; a.firstRow = firstRow; a.nSteps = w.nSteps; a.rowStride = w.rowStride; a.out = out; a.n = n;
    HIPCK(timed(h, "act_seq_dev", d.st, [&] { return launch_act_seq_dev(a, std::min(n, h->act.cus), d.st); }));
    return HL_OK;
  }
  case ACT_DEV_SEQ_CONV: {
    ActConvArgs c = *r.devConv; devSource(d, c);
    c.in = states; c.firstRow = firstRow; c.nSteps = w.nSteps; c.rowStride = w.rowStride; c.feat = *d.feat; c.n = n;
    if (r.devConvBand) HIPCK(timed(h, "act_conv_band_dev", d.st, [&] { return launch_act_conv_band_dev(c, h->act.cus, d.st); }));
    else HIPCK(timed(h, "act_conv_dev", d.st, [&] { return launch_act_conv_dev(c, h->act.cus, d.st); }));
    return devRows(h, d, *r.devConvRows, r.devConvPanel, n, *d.feat, (size_t)c.nF, out);
  }
  case ACT_DEV_SEQ_ROWS: {
    ActStackDevArgs sa{states, firstRow, w.nSteps, w.rowStride, *d.rows, n, h->dS, h->nApp};
    HIPCK(timed(h, "act_stack_dev", d.st, [&] { return launch_act_stack_dev(sa, d.st); }));
    return devForward(h, r, d, n, *d.rows, out);
  }
  case ACT_DEV_SEQ_NONE: break;      // (devAct refused the call before)
  }
  return HL_ERR_UNSUPPORTED;
}
// RACER::selectAction's head on n rows of network outputs (actdev.hip: act_head_kernel): it reads those, the noise and the configuration
// only, so it is the same launch under either source
struct DevHeadIo { const double* noise; double *act, *mu; float *V, *ADV; };
static int devHead(hl_learner* h, const DevCtx& d, int n, const double* O, const DevHeadIo& io) {
  ActHeadArgs a{};
  a.O = O; a.noise = io.noise; a.act = io.act; a.mu = io.mu; a.V = io.V; a.ADV = io.ADV;
  a.n = n; a.dA = h->dA; a.nOut = h->nOut; a.nDense = h->nDense; a.nAdv = h->cfg.adv_kind == HL_ADV_GAUSSIAN ? h->nAdv : 0; a.nOpt = h->nOpt;
  for (int i = 0; i < h->dA; ++i) if (h->cfg.bounded[i]) a.bounded |= 1ull << i;
  HIPCK(timed(h, "act_head_kernel", d.st, [&] { return launch_act_head(a, d.st); }));
  return HL_OK;
}
// The one body of the four _dev acting calls, behind their argument checks: n rows [n][dIn] at `in` (w == nullptr), or n windows w of the
// states array `in`; the network outputs into `out`, or (head != nullptr) into the source's scratch and RACER::selectAction's head on them.
// In this order: the call between the two halves of a step; a net the resolved table (learner_act.h: actResolve) refuses -- the snapshot
// source on a route that acts over the training buffers included --; the snapshot source before any snapshot, whose stream is created
// here; the stamp block of the dense kernels; n == 0; row_stride; the library's buffers -- between a window call's two launches the
// stacked rows of a dense net or the feature rows behind convolutions, in front of the head the outputs --; the handshake with the
// caller's stream around the launches
// `handshake` false (learner_rollout.h): the caller has done devEnter on the live source and does devLeave behind its own launches
static int devAct(hl_learner* h, const char* who, int n, const float* in, const DevWindows* w, double* out, const DevHeadIo* head, void* stream, bool handshake = true) {
  HL_LOCK(h);
  if (h->inStep) return fail(h, HL_ERR_STATE, std::string(who) + " between hl_step_begin and hl_step_end");
  const ActRoutes& r = actResolve(h);
  if (w ? r.devSeq == ACT_DEV_SEQ_NONE : !r.devRows) return fail(h, HL_ERR_UNSUPPORTED, who + (w ? r.devSeqNo : r.devRowsNo));
  if (w && h->act.source == HL_ACT_SNAPSHOT && !r.devSeqSnap) return fail(h, HL_ERR_UNSUPPORTED, std::string(who) + ": recurrent nets on wide inputs act over the training buffers, which cannot run beside a gradient step: they are served by the source HL_ACT_LIVE only");
  { int rc = devSnapEnsure(h, who); if (rc) return rc; }
  const DevCtx d = devCtx(h, h->act.source);
  if (!w || r.devSeq == ACT_DEV_SEQ_CONV || r.devSeq == ACT_DEV_SEQ_ROWS) { int rc = devStampsEnsure(h, d); if (rc) return rc; }
  if (n == 0) return HL_OK;
  if (w && w->rowStride < 1) return fail(h, HL_ERR_BAD_ARG, std::string(who) + ": row_stride below 1");
  if (w && r.devSeq == ACT_DEV_SEQ_CONV) { int rc = devEnsure(h, d.st, d.feat, d.featCap, (size_t)n * r.devConv->nF); if (rc) return rc; }
  if (w && r.devSeq == ACT_DEV_SEQ_ROWS) { int rc = devEnsure(h, d.st, d.rows, d.rowsCap, (size_t)n * h->dIn); if (rc) return rc; }
  if (head) { int rc = devEnsure(h, d.st, d.out, d.outCap, (size_t)n * h->nOut); if (rc) return rc; out = *d.out; }
  if (handshake) { int rc = devEnter(h, d, stream); if (rc) return rc; }
  { int rc = w ? devSeqForward(h, r, d, n, *w, in, out) : devForward(h, r, d, n, in, out); if (rc) return rc; }
  if (head) { int rc = devHead(h, d, n, out, *head); if (rc) return rc; }
  return handshake ? devLeave(h, d, stream) : HL_OK;
}
// The one body of hl_append_episodes_dev and of hl_rollout_step's ingestion, behind their argument checks: nEp > 0 episodes, every one of
// at least 2 steps.  *nBooked (where given) is set once the launches are out: the episodes stored, the ones behind them found no room
static int devIngest(hl_learner* h, int nEp, const int32_t* nsteps, const int32_t* terminated, const int64_t* tags, const int64_t* first_row,
                     int64_t row_stride, const float* dStates, const double* dActions, const double* dMu, const double* dRewards,
                     const float* dValues, const float* dAdvantages, void* stream, bool handshake = true, int* nBooked = nullptr) {
  { int rc = flushStaging(h); if (rc) return rc; }      // episodes staged by hl_append_episode go first
  const bool log = !h->episodeLog.empty();
  const DevCtx d = devCtx(h, HL_ACT_LIVE);      // (ingestion writes the replay the steps read: the learner's stream whatever the acting source)
  if (log) { int rc = devEnsure(h, h->stream, &h->act.devSums, &h->act.devSumsCap, (size_t)2 * nEp); if (rc) return rc; }
  if (handshake) { int rc = devEnter(h, d, stream); if (rc) return rc; }
  // the bookkeeping of hl_append_episode, episode by episode; an episode that finds no room ends the batch, the ones before it are stored
  std::vector<long long> ids((size_t)nEp);
  int booked = 0, rcBook = HL_OK;
  for (; booked < nEp; ++booked) {
    long long off = 0; int eid = 0;
    rcBook = appendAlloc(h, nsteps[booked], &off, &eid); if (rcBook) break;
    ids[(size_t)booked] = appendBook(h, eid, off, nsteps[booked], terminated[booked] != 0, tags[booked]);
  }
  // (a later episode's allocation may have re-packed the replay: the slot offsets are read from the order now; episode e sits at position booked - 1 - e)
  { int rc = refreshInsertionStats(h); if (rc) return rc; }
  for (int e0 = 0; e0 < booked; e0 += INGEST_DEV_MAX_EP) {
    IngestDevArgs ia{};
    ia.rp = h->rp; ia.S = dStates; ia.A = dActions; ia.MU = dMu; ia.R = dRewards; ia.V = dValues; ia.ADV = dAdvantages;
    ia.rowStride = row_stride; ia.nEp = std::min(INGEST_DEV_MAX_EP, booked - e0); ia.dS = h->dS; ia.dA = h->dA; ia.polDim = h->polDim;
    ia.stats = h->dStatsIns; ia.nEpTable = h->anyStep ? h->tableCount : 0;
    ia.sums = log ? h->act.devSums + (size_t)2 * e0 : nullptr;
    for (int k = 0; k < ia.nEp; ++k) {
      const EpMeta& m = h->order[(size_t)(booked - 1 - (e0 + k))];
      ia.d[k] = IngestDevDesc{m.off, m.tag, first_row[e0 + k], m.N, m.eid, m.term ? 1 : 0, 0};
    }
    HIPCK(timed(h, "ingest_dev_kernel", h->stream, [&] { return launch_ingest_dev(ia, h->stream); }));
  }
  if (handshake) { int rc = devLeave(h, d, stream); if (rc) return rc; }
  if (log && booked > 0) {
    std::vector<double> sums((size_t)2 * booked);
    HIPCK(hipMemcpyAsync(sums.data(), h->act.devSums, sums.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));
    for (int e = 0; e < booked && !h->episodeLog.empty(); ++e) appendLogLine(h, ids[(size_t)e], nsteps[e], (float)sums[(size_t)2 * e + 1]);
  }
  if (nBooked) *nBooked = booked;
  return rcBook;
}
}  // extern "C++"

int hl_act_dev_source(hl_learner* h, int32_t source) {
  if (!h) return HL_ERR_BAD_ARG;
  HL_LOCK_RAW(h);      // (nothing is enqueued)
  if (source != HL_ACT_LIVE && source != HL_ACT_SNAPSHOT) return fail(h, HL_ERR_BAD_ARG, "hl_act_dev_source: neither HL_ACT_LIVE nor HL_ACT_SNAPSHOT");
  h->act.source = source;
  return HL_OK;
}

int hl_policy_snapshot(hl_learner* h) {
  if (!h) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  ActState& s = h->act;
  if (!s.snapBuf[0]) {      // the two buffers and their events, once
    if (h->nParams % 8) return fail(h, HL_ERR_STATE, "hl_policy_snapshot: the blob is no multiple of 8 floats");
    const size_t len = snapScaleOff(h) + (size_t)roundUp(h->dS, 4);
    for (int b = 0; b < 2; ++b) {
      HIPCK(hipEventCreateWithFlags(&s.snapReady[b], hipEventDisableTiming));
      HIPCK(hipEventCreateWithFlags(&s.snapRead[b], hipEventDisableTiming));
    }
    HIPCK(devAlloc(&s.snapBuf[1], len)); HIPCK(devAlloc(&s.snapBuf[0], len));
  }
  const int b = s.snapCur < 0 ? 0 : s.snapCur ^ 1;      // the buffer that is not current
  if (s.snapReadSet[b]) HIPCK(hipStreamWaitEvent(h->stream, s.snapRead[b], 0));      // the last acting call that read it
  PolicySnapshotArgs a{h->W, h->rp.stMean, h->rp.stScale, s.snapBuf[b], s.snapBuf[b] + snapMeanOff(h), s.snapBuf[b] + snapScaleOff(h), h->nParams, h->dS};
  HIPCK(timed(h, "policy_snapshot", h->stream, [&] { return launch_policy_snapshot(a, h->stream); }));
  HIPCK(hipEventRecord(s.snapReady[b], h->stream));
  s.snapCur = b; s.snapGrad[b] = h->nGradSteps; ++s.nSnap;
  return HL_OK;
}

int hl_policy_snapshot_info(hl_learner* h, int64_t* n_snapshots, int64_t* nGradSteps) {
  if (!h) return HL_ERR_BAD_ARG;
  HL_LOCK_RAW(h);
  if (n_snapshots) *n_snapshots = h->act.nSnap;
  if (nGradSteps) *nGradSteps = h->act.snapCur >= 0 ? h->act.snapGrad[h->act.snapCur] : -1;
  return HL_OK;
}

int hl_forward_dev(hl_learner* h, int32_t n, const float* dStates, double* dOutputs, void* stream) {
  if (!h || n < 0 || (n > 0 && (!dStates || !dOutputs))) return HL_ERR_BAD_ARG;
  return devAct(h, "hl_forward_dev", n, dStates, nullptr, dOutputs, nullptr, stream);
}

int hl_select_actions_dev(hl_learner* h, int32_t n, const float* dStates, const double* dNoise, double* dActions, double* dMu,
                          float* dValues, float* dAdvantages, void* stream) {
  if (!h || n < 0 || (n > 0 && (!dStates || !dActions || !dMu || !dValues || !dAdvantages))) return HL_ERR_BAD_ARG;
  const DevHeadIo head{dNoise, dActions, dMu, dValues, dAdvantages};
  return devAct(h, "hl_select_actions_dev", n, dStates, nullptr, nullptr, &head, stream);
}

int hl_forward_sequences_dev(hl_learner* h, int32_t n, const int64_t* dFirstRow, const int32_t* dNSteps, int64_t row_stride, const float* dStates,
                             double* dOutputs, void* stream) {
  if (!h || n < 0 || (n > 0 && (!dFirstRow || !dNSteps || !dStates || !dOutputs))) return HL_ERR_BAD_ARG;
  const DevWindows w{dFirstRow, dNSteps, row_stride};
  return devAct(h, "hl_forward_sequences_dev", n, dStates, &w, dOutputs, nullptr, stream);
}

int hl_select_actions_sequences_dev(hl_learner* h, int32_t n, const int64_t* dFirstRow, const int32_t* dNSteps, int64_t row_stride, const float* dStates,
                                    const double* dNoise, double* dActions, double* dMu, float* dValues, float* dAdvantages, void* stream) {
  if (!h || n < 0 || (n > 0 && (!dFirstRow || !dNSteps || !dStates || !dActions || !dMu || !dValues || !dAdvantages))) return HL_ERR_BAD_ARG;
  const DevWindows w{dFirstRow, dNSteps, row_stride};
  const DevHeadIo head{dNoise, dActions, dMu, dValues, dAdvantages};
  return devAct(h, "hl_select_actions_sequences_dev", n, dStates, &w, nullptr, &head, stream);
}

int hl_append_episodes_dev(hl_learner* h, int32_t nEp, const int32_t* nsteps, const int32_t* terminated, const int64_t* tags,
                           const int64_t* first_row, int64_t row_stride, const float* dStates, const double* dActions,
                           const double* dMu, const double* dRewards, const float* dValues, const float* dAdvantages, void* stream) {
  if (!h || nEp < 0) return HL_ERR_BAD_ARG;
  if (nEp > 0 && (!nsteps || !terminated || !tags || !first_row || !dStates || !dActions || !dMu || !dRewards || !dValues)) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  if (h->inStep) return fail(h, HL_ERR_STATE, "hl_append_episodes_dev between hl_step_begin and hl_step_end");
  if (nEp > 0 && row_stride < 1) return fail(h, HL_ERR_BAD_ARG, "hl_append_episodes_dev: row_stride below 1");
  for (int e = 0; e < nEp; ++e) {
    if (nsteps[e] < 2) return fail(h, HL_ERR_BAD_ARG, "Episode must at least have s0 and sT");
    if (first_row[e] < 0) return fail(h, HL_ERR_BAD_ARG, "hl_append_episodes_dev: a negative first row");
  }
  if (nEp == 0) return HL_OK;
  return devIngest(h, nEp, nsteps, terminated, tags, first_row, row_stride, dStates, dActions, dMu, dRewards, dValues, dAdvantages, stream);
}
