// smarties_amd/csrc/learner_dev.h -- part of learner.cpp's ONE translation unit (included there, behind learner_act.h): acting and episode ingestion from device memory: hl_forward_dev, hl_select_actions_dev, hl_forward_sequences_dev, hl_select_actions_sequences_dev, hl_append_episodes_dev
#pragma once
#include "../../include/smarties_hip_dev.h"
static_assert(ACT_DEV_MAX_ROW == HL_ACT_DEV_MAX_ROW, "the row bound of the device calls the header states");
static_assert(HL_MAX_DIMA <= 64, "ActHeadArgs::bounded holds one bit per action component");

extern "C++" {
// the handshake with the caller's stream: the learner's stream waits for what the caller queued so far ...
static int devEnter(hl_learner* h, void* stream) {
  if (!h->act.devIn) HIPCK(hipEventCreateWithFlags(&h->act.devIn, hipEventDisableTiming));
  if (!h->act.devDone) HIPCK(hipEventCreateWithFlags(&h->act.devDone, hipEventDisableTiming));
  HIPCK(hipEventRecord(h->act.devIn, static_cast<hipStream_t>(stream)));
  HIPCK(hipStreamWaitEvent(h->stream, h->act.devIn, 0));
  return HL_OK;
}
// ... and what the caller queues from here on waits for the learner's work; the host waits for neither
static int devLeave(hl_learner* h, void* stream) {
  HIPCK(hipEventRecord(h->act.devDone, h->stream));
  HIPCK(hipStreamWaitEvent(static_cast<hipStream_t>(stream), h->act.devDone, 0));
  return HL_OK;
}
// a device buffer of at least `need` elements (a larger one replaces it once the stream is done with the old one)
template <typename T> static int devEnsure(hl_learner* h, T** p, size_t* cap, size_t need) {
  if (need <= *cap) return HL_OK;
  if (*p) { HIPCK(hipStreamSynchronize(h->stream)); hipFree(*p); *p = nullptr; *cap = 0; }
  HIPCK(devAlloc(p, need)); *cap = need;
  return HL_OK;
}
// the scratch block the dense acting kernels stamp, allocated once
static int devStampsEnsure(hl_learner* h) {
  if (!h->act.devStamps) HIPCK(devAlloc(&h->act.devStamps, (size_t)std::max(ACT_MAXROWS, act_rows_blocks(ACT_ROWS_CHUNK))));
  return HL_OK;
}
// which nets the row calls serve
static int devActEnsure(hl_learner* h, const char* who) {
  if (h->inStep) return fail(h, HL_ERR_STATE, std::string(who) + " between hl_step_begin and hl_step_end");
  if (h->recurrent) return fail(h, HL_ERR_UNSUPPORTED, std::string(who) + ": recurrent nets act on windows in host memory (hl_forward_sequences)");
  if (h->nConv > 0) return fail(h, HL_ERR_UNSUPPORTED, std::string(who) + ": nets with convolutional layers in front act on windows in device memory (hl_forward_sequences_dev; without appended observations: windows of one state)");
  if (!act_dev_rows_ok(h)) return fail(h, HL_ERR_UNSUPPORTED, std::string(who) + ": an input row beyond 8192 or a layer beyond 2048, or SMARTIES_HIP_GENERIC bit 2 -- here: " + h->act.devWhy);
  return devStampsEnsure(h);
}
// ... and the window calls: the recurrent nets of the one-launch batched kernel (actSeqOk) and those on wide inputs (act_dev_tm_ok), the dense nets above, the feed-forward nets behind
// convolutions of the conv-stack kernel's plan (act_conv_plan_ok: whatever the row size -- the rows lie in device memory) and, beyond it, of the
// banded and panelled kernels' (act_dev_conv_ok, act_dev_rows_ok: neither the image nor the input row has to be resident in LDS)
static int devSeqEnsure(hl_learner* h, const char* who) {
  if (h->inStep) return fail(h, HL_ERR_STATE, std::string(who) + " between hl_step_begin and hl_step_end");
  const char* host = ": this net acts on windows in host memory (hl_forward_sequences); served here: ";
  if (h->recurrent) {
    if (act_dev_tm_ok(h)) return HL_OK;      // wide inputs: the time-step-major chain on windows gathered from the caller's array
    if (!actSeqOk(h)) return fail(h, HL_ERR_UNSUPPORTED, std::string(who) + host + "one recurrent layer type without convolutions or encoder_rnn, layers up to 256 cells and 1024 inputs or wide inputs");
    return HL_OK;
  }
  if (h->nConv > 0) {
    if (!act_dev_conv_ok(h)) return fail(h, HL_ERR_UNSUPPORTED, std::string(who) + ": this net acts on rows in host memory (hl_forward); served here behind convolutions: every map within 160 KB of LDS beside a band of the image, feature rows up to 8192 and dense layers up to 2048 wide, SMARTIES_HIP_GENERIC bit 2 clear -- here: " + h->act.devWhy);
    return devStampsEnsure(h);
  }
  if (!act_dev_rows_ok(h)) return fail(h, HL_ERR_UNSUPPORTED, std::string(who) + host + "dense nets with input rows up to 8192 and layers up to 2048 wide, SMARTIES_HIP_GENERIC bit 2 clear -- here: " + h->act.devWhy);
  return devStampsEnsure(h);
}
// the library's buffer between the window calls' two launches: the stacked rows of a dense net, the feature rows of a net behind convolutions
static int devSeqRowsEnsure(hl_learner* h, int n) {
  if (h->recurrent) return HL_OK;
  if (h->nConv > 0) return devEnsure(h, &h->act.devFeat, &h->act.devFeatCap, (size_t)n * h->act.devConvArgs.nF);
  return devEnsure(h, &h->act.devRows, &h->act.devRowsCap, (size_t)n * h->dIn);
}
// the row-block kernel per chunk of ACT_ROWS_CHUNK rows [n][ldIn] in device memory: act_rows_kernel, or (panel) act_rows_panel_kernel, which
// stages the first layer's input row in panels
static int devRows(hl_learner* h, const ActRowsArgs& plan, bool panel, int n, const float* in, size_t ldIn, double* out) {
  for (int r0 = 0; r0 < n; r0 += ACT_ROWS_CHUNK) {
    ActRowsArgs a = plan;
    a.in = in + (size_t)r0 * ldIn; a.out = out + (size_t)r0 * h->nOut; a.done = h->act.devStamps; a.n = std::min(ACT_ROWS_CHUNK, n - r0); a.tag = actNextTag(h);
    if (panel) HIPCK(timed(h, "act_rows_panel_dev", h->stream, [&] { return launch_act_rows_panel(a, h->stream); }));
    else HIPCK(timed(h, "act_rows_dev", h->stream, [&] { return launch_act_rows(a, h->stream); }));
  }
  return HL_OK;
}
// hl_forward's kernels on device rows, enqueued on the learner's stream: up to ACT_MAXROWS rows of a net within the one-kernel route's
// bounds that kernel (as hl_forward picks it: the same bits), everything else the row-block kernel per chunk of ACT_ROWS_CHUNK rows (input
// rows beyond ACT_ROWS_MAXW: its panelled form)
static int devForward(hl_learner* h, int n, const float* in, double* out) {
  if (n <= ACT_MAXROWS && actFewOk(h)) {
    const ActArgs aa = actFewArgs(h, in, out, h->act.devStamps, actNextTag(h));
    HIPCK(timed(h, "act_forward_dev", h->stream, [&] { return launch_act_forward(aa, n, h->stream); }));
    return HL_OK;
  }
  return devRows(h, h->act.devRowsArgs, h->act.devRowsPanel, n, in, h->dIn, out);
}
static_assert(sizeof(long long) == sizeof(int64_t), "the row tables are passed on as they come");
// n windows of a recurrent net on wide inputs: agents in chunks of min(local batch, ACT_SEQ_CHUNK) -- the chain borrows the training rows of that many samples between
// steps, as actTmChain does; nothing is staged, so no stage-bytes cap -- each chunk the prepare launch on the tables at its offset, the input
// product and the chain over all recWin steps (the host does not know the windows: an agent whose window has ended is left out by the
// forward tiles), the output layer on the chunk's rows of Yout straight into `out`.  All chunks back to back in ONE timed bracket
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
// n windows of the caller's device arrays, enqueued on the learner's stream.  Recurrent nets: ONE launch of the batched window kernel, which
// gathers and truncates the windows itself (no staging, so no chunks); on wide inputs the chain above.  Behind convolutions: ONE launch of the
// conv-stack kernel, which reads every agent's stacked row from its window's states, then the row-block kernel on the feature rows per chunk of
// ACT_ROWS_CHUNK (hl_forward's two launches without the staging).  Dense nets: the agents' stacked rows built by one small launch, then devForward on them
static int devSeqForward(hl_learner* h, int n, const int64_t* firstRow, const int32_t* nSteps, int64_t rowStride, const float* states, double* out) {
  if (h->recurrent && act_dev_tm_ok(h)) return devSeqTmForward(h, n, firstRow, nSteps, rowStride, states, out);
  if (h->recurrent) {
    ActSeqArgs a = h->act.seqArgs;
    a.states = states; a.firstRow = reinterpret_cast<const long long*>(firstRow); a.nSteps = nSteps; a.rowStride = rowStride; a.out = out; a.n = n;
    HIPCK(timed(h, "act_seq_dev", h->stream, [&] { return launch_act_seq_dev(a, std::min(n, h->act.cus), h->stream); }));
    return HL_OK;
  }
  if (h->nConv > 0) {
    ActConvArgs c = h->act.devConvArgs;
    c.in = states; c.firstRow = reinterpret_cast<const long long*>(firstRow); c.nSteps = nSteps; c.rowStride = rowStride; c.feat = h->act.devFeat; c.n = n;
    if (h->act.devConvBand) HIPCK(timed(h, "act_conv_band_dev", h->stream, [&] { return launch_act_conv_band_dev(c, h->act.cus, h->stream); }));
    else HIPCK(timed(h, "act_conv_dev", h->stream, [&] { return launch_act_conv_dev(c, h->act.cus, h->stream); }));
    return devRows(h, h->act.devConvRowsArgs, h->act.devConvPanel, n, h->act.devFeat, (size_t)c.nF, out);
  }
  ActStackDevArgs sa{states, reinterpret_cast<const long long*>(firstRow), nSteps, rowStride, h->act.devRows, n, h->dS, h->nApp};
  HIPCK(timed(h, "act_stack_dev", h->stream, [&] { return launch_act_stack_dev(sa, h->stream); }));
  return devForward(h, n, h->act.devRows, out);
}
// RACER::selectAction's head on n rows of network outputs (actdev.hip: act_head_kernel)
static int devHead(hl_learner* h, int n, const double* O, const double* dNoise, double* dActions, double* dMu, float* dValues, float* dAdvantages) {
  ActHeadArgs a{};
  a.O = O; a.noise = dNoise; a.act = dActions; a.mu = dMu; a.V = dValues; a.ADV = dAdvantages;
  a.n = n; a.dA = h->dA; a.nOut = h->nOut; a.nDense = h->nDense; a.nAdv = h->cfg.adv_kind == HL_ADV_GAUSSIAN ? h->nAdv : 0; a.nOpt = h->nOpt;
  for (int i = 0; i < h->dA; ++i) if (h->cfg.bounded[i]) a.bounded |= 1ull << i;
  HIPCK(timed(h, "act_head_kernel", h->stream, [&] { return launch_act_head(a, h->stream); }));
  return HL_OK;
}
}  // extern "C++"

int hl_forward_dev(hl_learner* h, int32_t n, const float* dStates, double* dOutputs, void* stream) {
  if (!h || n < 0 || (n > 0 && (!dStates || !dOutputs))) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  { int rc = devActEnsure(h, "hl_forward_dev"); if (rc) return rc; }
  if (n == 0) return HL_OK;
  { int rc = devEnter(h, stream); if (rc) return rc; }
  { int rc = devForward(h, n, dStates, dOutputs); if (rc) return rc; }
  return devLeave(h, stream);
}

int hl_select_actions_dev(hl_learner* h, int32_t n, const float* dStates, const double* dNoise, double* dActions, double* dMu,
                          float* dValues, float* dAdvantages, void* stream) {
  if (!h || n < 0 || (n > 0 && (!dStates || !dActions || !dMu || !dValues || !dAdvantages))) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  { int rc = devActEnsure(h, "hl_select_actions_dev"); if (rc) return rc; }
  if (n == 0) return HL_OK;
  { int rc = devEnsure(h, &h->act.devOut, &h->act.devOutCap, (size_t)n * h->nOut); if (rc) return rc; }
  { int rc = devEnter(h, stream); if (rc) return rc; }
  { int rc = devForward(h, n, dStates, h->act.devOut); if (rc) return rc; }
  { int rc = devHead(h, n, h->act.devOut, dNoise, dActions, dMu, dValues, dAdvantages); if (rc) return rc; }
  return devLeave(h, stream);
}

int hl_forward_sequences_dev(hl_learner* h, int32_t n, const int64_t* dFirstRow, const int32_t* dNSteps, int64_t row_stride, const float* dStates,
                             double* dOutputs, void* stream) {
  if (!h || n < 0 || (n > 0 && (!dFirstRow || !dNSteps || !dStates || !dOutputs))) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  { int rc = devSeqEnsure(h, "hl_forward_sequences_dev"); if (rc) return rc; }
  if (n == 0) return HL_OK;
  if (row_stride < 1) return fail(h, HL_ERR_BAD_ARG, "hl_forward_sequences_dev: row_stride below 1");
  { int rc = devSeqRowsEnsure(h, n); if (rc) return rc; }
  { int rc = devEnter(h, stream); if (rc) return rc; }
  { int rc = devSeqForward(h, n, dFirstRow, dNSteps, row_stride, dStates, dOutputs); if (rc) return rc; }
  return devLeave(h, stream);
}

int hl_select_actions_sequences_dev(hl_learner* h, int32_t n, const int64_t* dFirstRow, const int32_t* dNSteps, int64_t row_stride, const float* dStates,
                                    const double* dNoise, double* dActions, double* dMu, float* dValues, float* dAdvantages, void* stream) {
  if (!h || n < 0 || (n > 0 && (!dFirstRow || !dNSteps || !dStates || !dActions || !dMu || !dValues || !dAdvantages))) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  { int rc = devSeqEnsure(h, "hl_select_actions_sequences_dev"); if (rc) return rc; }
  if (n == 0) return HL_OK;
  if (row_stride < 1) return fail(h, HL_ERR_BAD_ARG, "hl_select_actions_sequences_dev: row_stride below 1");
  { int rc = devSeqRowsEnsure(h, n); if (rc) return rc; }
  { int rc = devEnsure(h, &h->act.devOut, &h->act.devOutCap, (size_t)n * h->nOut); if (rc) return rc; }
  { int rc = devEnter(h, stream); if (rc) return rc; }
  { int rc = devSeqForward(h, n, dFirstRow, dNSteps, row_stride, dStates, h->act.devOut); if (rc) return rc; }
  { int rc = devHead(h, n, h->act.devOut, dNoise, dActions, dMu, dValues, dAdvantages); if (rc) return rc; }
  return devLeave(h, stream);
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
  { int rc = flushStaging(h); if (rc) return rc; }      // episodes staged by hl_append_episode go first
  const bool log = !h->episodeLog.empty();
  if (log) { int rc = devEnsure(h, &h->act.devSums, &h->act.devSumsCap, (size_t)2 * nEp); if (rc) return rc; }
  { int rc = devEnter(h, stream); if (rc) return rc; }
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
  { int rc = devLeave(h, stream); if (rc) return rc; }
  if (log && booked > 0) {
    std::vector<double> sums((size_t)2 * booked);
    HIPCK(hipMemcpyAsync(sums.data(), h->act.devSums, sums.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));
    for (int e = 0; e < booked && !h->episodeLog.empty(); ++e) appendLogLine(h, ids[(size_t)e], nsteps[e], (float)sums[(size_t)2 * e + 1]);
  }
  return rcBook;
}
