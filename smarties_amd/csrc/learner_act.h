// smarties_amd/csrc/learner_act.h -- part of learner.cpp's ONE translation unit (included there, like step_exec.h): rollout inference (Learner::select's network evaluation): hl_forward, hl_forward_sequence, hl_forward_sequences
#pragma once
#include "../../include/smarties_hip_act.h"
#include "act_host.h"
#include "act_plan.h"
static_assert(ACT_SEQ_CHUNK == HL_ACT_SEQ_CHUNK, "the chunk capacity the header states");
static_assert(ACT_ROWS_CHUNK == HL_ACT_ROWS_CHUNK, "the chunk capacity the header states");
static_assert(ACT_ROWS_SMALL_NET == HL_ACT_ROWS_SMALL_NET && ACT_ROWS_WIDE_MIN_N == HL_ACT_ROWS_WIDE_MIN_N, "the switch the header states");

extern "C++" {      // (learner.cpp includes this file among its extern "C" entry points; the chunk drivers below are templates)
static unsigned actNextTag(hl_learner* h) { if (++h->act.tag == 0) ++h->act.tag; return h->act.tag; }      // (0 is what a fresh stage holds)
// compute units of the device (0: the runtime does not say)
static int actCus(hl_learner* h) {
  int dev = 0, cus = 0;
  if (!h->act.cus && hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) h->act.cus = cus;
  return h->act.cus;
}
// the kernel stamps a row once its outputs are in host memory: poll the stamps (a stream synchronisation costs ~10 us more),
// give up after 2 s and fall back to it
static int actWait(hl_learner* h, volatile unsigned* pDone, int n, unsigned tag) {
  const auto t0 = std::chrono::steady_clock::now();
  for (int r = 0; r < n; ++r)
    while (pDone[r] != tag) {
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) { HIPCK(hipStreamSynchronize(h->stream)); break; }
    }
  std::atomic_thread_fence(std::memory_order_acquire);
  return HL_OK;
}
// the output layer on the first `rows` rows of the last hidden layer's activations; done != nullptr: the rows' stamps
static hipError_t actOutput(hl_learner* h, int rows, double* out, volatile unsigned* done, unsigned tag) {
  const DevHidden& q = h->hid[h->nHidden - 1];
  return launch_act_output(q.hasRes ? q.Rr : q.Y, q.ldA, q.size, h->W, h->indWo, h->indBo, h->indBp, h->ldWo, h->nDense, h->nSig, rows,
                           out, h->stream, const_cast<unsigned*>(done), tag, h->cfg.nnOutputFunc);
}
// what ActArgs, ActRowsArgs and ActSeqArgs spell alike: the blob, the standardisation, the output layer (all fixed from hl_create on)
template <typename A> static void actFillShared(const hl_learner* h, A& a) {
  a.W = h->W; a.stMean = h->rp.stMean; a.stScale = h->rp.stScale;
  a.nDense = h->nDense; a.nSig = h->nSig; a.nOut = h->nOut; a.ldWo = h->ldWo; a.indWo = h->indWo; a.indBo = h->indBo; a.indBp = h->indBp;
  a.outFunc = h->cfg.nnOutputFunc;
}
static int actFillLayers(const hl_learner* h, int first, ActLayer* L) {      // hid[first ..]; returns their number
  for (int j = first; j < h->nHidden; ++j) { const DevHidden& d = h->hid[j];
    L[j - first] = ActLayer{d.nIn, d.size, d.ldW, d.func, d.hasRes, d.resW, d.indW, d.indB, d.indWr, d.indBr}; }
  return h->nHidden - first;
}
// the window launches' arguments for acting (segment seg of a stack of two layer types, -1: the whole stack): B windows of raw states;
// off / cnt: the per-agent tables of a chain (nullptr: one window of `steps` states behind `ctx` context states)
static RecArgs actRecArgs(hl_learner* h, int seg, int B, const float* states, const int* off, const int* cnt, int steps, int ctx) {
  RecArgs ra = recArgs(h, 0, seg); ra.B = B; ra.actStates = states; ra.actOff = off; ra.actCnt = cnt; ra.actSteps = steps; ra.actCtx = ctx;
  return ra;
}
// the one-kernel route's arguments (misc.hip: act_forward_kernel) on the given rows, outputs and stamps
static ActArgs actFewArgs(const hl_learner* h, const float* in, double* out, volatile unsigned* done, unsigned tag) {
  ActArgs aa{}; actFillShared(h, aa);
  aa.in = in; aa.out = out; aa.done = done; aa.tag = tag;
  aa.dS = h->dS; aa.dIn = h->dIn; aa.nL = actFillLayers(h, 0, aa.L);
  return aa;
}
static const float actNoState = 0.f;      // (a predicate asks for given states, it does not read them)
// a few rows of a dense net, one workgroup per row (misc.hip: act_forward_kernel): layers and input rows within its bounds;
// SMARTIES_HIP_GENERIC bit 2 keeps the route over the training buffers
static bool actFewOk(hl_learner* h) {
  if (h->act.fewOk) return h->act.fewOk > 0;
  bool ok = !h->recurrent && h->nConv == 0 && !(h->generic & 2) && h->dIn <= ACT_MAXW;
  for (int j = 0; j < h->nHidden; ++j) if (h->hid[j].size > ACT_MAXW || h->hid[j].nIn > ACT_MAXW) ok = false;
  h->act.fewOk = ok ? 1 : -1;
  return ok;
}
// the batched window kernel (actseq.hip) serves this net: one recurrent layer type, no convolutions in front, layers within its bounds
static bool actSeqOk(hl_learner* h) {
  if (h->act.seqOk) return h->act.seqOk > 0;
  h->act.seqOk = -1;
  if (!h->recurrent || h->nConv > 0 || h->recSplit || h->wideIn) return false;      // (wide inputs: the time-step-major chain, as hl_forward_sequence)
  const RecArgs ra = recArgs(h, 0);
  ActSeqArgs& a = h->act.seqArgs; a = ActSeqArgs{};
  actFillShared(h, a);
  a.dS = h->dS; a.nApp = h->nApp; a.recWin = h->recWin; a.nL = ra.nL; a.gates = ra.gates; a.func = ra.func;
  for (int j = 0; j < ra.nL; ++j) { const RecLayer& L = ra.L[j]; a.L[j] = ActSeqLayer{L.nIn, L.nC, L.hasRes, L.resW, L.indW, L.indB, L.indWr, L.indBr, 0, 0}; }
  if (!act_seq_plan(&a) || actCus(h) < 1) return false;
  h->act.seqOk = 1;
  return true;
}
// the time-step-major launches (rectm.hip) serve this net's acting window -- hl_forward_sequence's route where a layer is wider than 256
// cells --: many agents' windows then run as the samples of one chain of those launches
static bool actTmOk(hl_learner* h) {
  if (h->act.tmOk) return h->act.tmOk > 0;
  const bool ok = h->recurrent && h->nConv == 0 && !h->recSplit && rec_tm_act_ok(actRecArgs(h, -1, 1, &actNoState, nullptr, nullptr, 1, 0));
  h->act.tmOk = ok ? 1 : -1;
  return ok;
}
// the workgroup-per-sample window kernels (rec.hip) serve this net's acting window -- hl_forward_sequence's route for every net the two
// predicates above leave: convolutions in front, RNN encoder layers under MGU layers, a window beyond the batched kernel's LDS --: many
// agents' windows then run as the samples of hl_forward_sequence's own launches, workgroup b on agent b's window
static bool actWinOk(hl_learner* h) {
  if (h->act.winOk) return h->act.winOk > 0;
  bool ok = h->recurrent;
  for (int seg = h->recSplit ? 0 : -1; ok && seg < (h->recSplit ? 2 : 0); ++seg) ok = rec_win_act_ok(actRecArgs(h, seg, 1, &actNoState, nullptr, nullptr, 1, 0));
  h->act.winOk = ok ? 1 : -1;
  return ok;
}
// the row-block kernel (actrows.hip) serves this net: dense, no convolutions in front, input rows and layers within its bounds;
// SMARTIES_HIP_GENERIC bit 2 keeps the route over the training buffers
static bool act_rows_ok(hl_learner* h) {
  if (h->act.rowsOk) return h->act.rowsOk > 0;
  h->act.rowsOk = -1;
  if (h->recurrent || h->nConv > 0 || h->dIn > ACT_ROWS_MAXW || (h->generic & 2)) return false;
  ActRowsArgs& a = h->act.rowsArgs; a = ActRowsArgs{};
  actFillShared(h, a);
  a.dS = h->dS; a.dIn = h->dIn; a.nL = actFillLayers(h, 0, a.L);
  if (!act_rows_plan(&a)) return false;
  long long nW = (long long)h->hid[h->nHidden - 1].size * h->ldWo;
  for (int j = 0; j < h->nHidden; ++j) nW += (long long)h->hid[j].nIn * h->hid[j].ldW;
  h->act.rowsSmall = nW <= ACT_ROWS_SMALL_NET;
  h->act.rowsOk = 1;
  return true;
}
// the conv-stack kernels (actconv.hip) and the row-block kernel behind them serve this net: feed-forward, convolutions in front, image and maps
// within a workgroup's LDS, feature rows and dense layers within the row-block kernel's bounds; SMARTIES_HIP_GENERIC bit 2 keeps the route
// over the training buffers.  Depends on the net only, never on n or on where the rows lie: hl_forward's route (act_conv_ok) and the
// window calls on device memory (learner_dev.h: devSeqEnsure) both ask it
static bool act_conv_plan_ok(hl_learner* h) {
  if (h->act.convPlanOk) return h->act.convPlanOk > 0;
  h->act.convPlanOk = -1;
  if (h->nConv < 1 || h->nHidden < 2 || (h->generic & 2)) return false;
  ActConvArgs& c = h->act.convArgs; c = ActConvArgs{};
  c.W = h->W; c.stMean = h->rp.stMean; c.stScale = h->rp.stScale;
  c.dS = h->dS; c.dIn = h->dIn; c.nL = h->nConv; c.recurrent = h->recurrent ? 1 : 0;
  for (int l = 0; l < h->nConv; ++l) { const ConvGeo& g = h->cg[l];
    c.L[l] = ActConvLayer{g.InC, g.InY, g.InX, g.KnC, g.KnY, g.KnX, g.S, g.OpY, g.OpX, g.K, g.P, g.indW, g.indB, 0, 0, 0}; }
  if (!act_conv_plan(&c) || c.extras != h->extras || c.nF != h->hid[1].nIn) return false;
  c.ldF = c.nF;
  // the dense layers behind: hid[1 ..] on feature rows [extras | last map], standardised already
  ActRowsArgs& a = h->act.convRowsArgs; a = ActRowsArgs{};
  actFillShared(h, a); a.stMean = nullptr; a.stScale = nullptr;
  a.dS = c.nF; a.dIn = c.nF; a.nL = actFillLayers(h, 1, a.L);
  if (!act_rows_plan(&a) || actCus(h) < 1) return false;
  h->act.convPlanOk = 1;
  return true;
}
// ... and hl_forward takes that route: rows in HOST memory go through pinned staging, so on top of the plan the row-size switch.
// A row's result is the same alone, among others and through the window calls
static bool act_conv_ok(hl_learner* h) {
  if (h->act.convOk) return h->act.convOk > 0;
  h->act.convOk = -1;
  // raw rows beyond HL_ACT_CONV_MAX_ROW_BYTES: the copy into pinned staging costs more than the route saves (the header's figures);
  // SMARTIES_HIP_GENERIC bit 4096 holds the switch open (tests, tools/act_conv_timing.py)
  if ((size_t)h->dIn * sizeof(float) > (size_t)HL_ACT_CONV_MAX_ROW_BYTES && !(h->generic & 4096)) return false;
  if (!act_conv_plan_ok(h)) return false;
  // rows per chunk: no more than HL_ACT_CONV_STAGE_BYTES of staged raw rows, whole blocks of 16 rows, at least one
  const size_t fit = (size_t)HL_ACT_CONV_STAGE_BYTES / ((size_t)h->dIn * sizeof(float));
  h->act.convCap = std::max(16, (int)(std::min((size_t)ACT_ROWS_CHUNK, fit) & ~(size_t)15));
  h->act.convOk = 1;
  return true;
}
// ---- the device calls (learner_dev.h) beyond the three predicates above, which they leave as they are: rows in device memory can be streamed,
// so neither the whole image nor the whole input row has to fit a workgroup's LDS (actband.hip, the plans of act_plan.h).
// SMARTIES_HIP_GENERIC bit 8192 sends every net those kernels can run through them -- three bands, panels of 64 columns --, nets the
// resident kernels serve among them (tests: the two forms give the same bits)
constexpr int ACT_DEV_FORCE_NB = 3, ACT_DEV_FORCE_PN = 64;
static bool actDevRefuse(hl_learner* h, const char* why) { h->act.devWhy = why; return false; }
// dense nets on rows in device memory: act_rows_kernel where act_rows_ok serves the net, act_rows_panel_kernel on input rows up to
// ACT_DEV_MAX_ROW wide otherwise
static bool act_dev_rows_ok(hl_learner* h) {
  if (h->act.devRowsOk) return h->act.devRowsOk > 0;
  h->act.devRowsOk = -1;
  if (h->recurrent || h->nConv > 0) return actDevRefuse(h, "a recurrent net or convolutions in front");
  if (h->generic & 2) return actDevRefuse(h, "SMARTIES_HIP_GENERIC bit 2");
  const bool force = (h->generic & 8192) != 0;
  ActRowsArgs& a = h->act.devRowsArgs;
  auto panels = [&] {
    a = ActRowsArgs{}; actFillShared(h, a);
    a.dS = h->dS; a.dIn = h->dIn; a.nL = actFillLayers(h, 0, a.L);
    return act_rows_panel_plan(&a, force ? ACT_DEV_FORCE_PN : 0);
  };
  if (force && panels()) h->act.devRowsPanel = true;
  else if (act_rows_ok(h)) { a = h->act.rowsArgs; h->act.devRowsPanel = false; }
  else if (!force && panels()) h->act.devRowsPanel = true;
  else {
    if (h->dIn > ACT_DEV_MAX_ROW) return actDevRefuse(h, "an input row beyond HL_ACT_DEV_MAX_ROW = 8192");
    for (int j = 0; j < h->nHidden; ++j) if (h->hid[j].size > ACT_ROWS_MAXW) return actDevRefuse(h, "a layer beyond 2048");
    return actDevRefuse(h, "the layers' activations beyond 160 KB of LDS");
  }
  h->act.devRowsOk = 1;
  return true;
}
// feed-forward nets behind convolutions on windows in device memory: today's two launches wherever act_conv_plan_ok serves the net; otherwise
// act_conv_band_dev_kernel where the image does not fit beside the maps, act_rows_panel_kernel where the feature row is beyond ACT_ROWS_MAXW
static bool act_dev_conv_ok(hl_learner* h) {
  if (h->act.devConvOk) return h->act.devConvOk > 0;
  h->act.devConvOk = -1;
  if (h->recurrent || h->nConv < 1 || h->nHidden < 2) return actDevRefuse(h, "a recurrent net, or no convolutions in front of dense layers");
  if (h->generic & 2) return actDevRefuse(h, "SMARTIES_HIP_GENERIC bit 2");
  const bool force = (h->generic & 8192) != 0;
  ActConvArgs& c = h->act.devConvArgs; ActRowsArgs& a = h->act.devConvRowsArgs;
  if (!force && act_conv_plan_ok(h)) {
    c = h->act.convArgs; a = h->act.convRowsArgs; h->act.devConvBand = h->act.devConvPanel = false;
    h->act.devConvOk = 1;
    return true;
  }
  auto conv = [&](bool bands) {
    c = ActConvArgs{};
    c.W = h->W; c.stMean = h->rp.stMean; c.stScale = h->rp.stScale;
    c.dS = h->dS; c.dIn = h->dIn; c.nL = h->nConv; c.recurrent = 0;
    for (int l = 0; l < h->nConv; ++l) { const ConvGeo& g = h->cg[l];
      c.L[l] = ActConvLayer{g.InC, g.InY, g.InX, g.KnC, g.KnY, g.KnX, g.S, g.OpY, g.OpX, g.K, g.P, g.indW, g.indB, 0, 0, 0}; }
    if (!(bands ? act_conv_band_plan(&c, force ? ACT_DEV_FORCE_NB : 0) : act_conv_wide_plan(&c))) return false;
    if (c.extras != h->extras || c.nF != h->hid[1].nIn) return false;
    c.ldF = c.nF;
    return true;
  };
  if (conv(force)) h->act.devConvBand = force;
  else if (conv(!force)) h->act.devConvBand = !force;
  else {
    long long tab, buf[2];
    if (act_conv_geometry(&c, &tab, buf)) return actDevRefuse(h, "a map of the conv stack beyond 160 KB of LDS at any band count");
    return actDevRefuse(h, "a feature row beyond HL_ACT_DEV_MAX_ROW = 8192, or the stack's geometry");
  }
  // the dense layers behind: hid[1 ..] on feature rows [extras | last map], standardised already
  auto dense = [&](bool panels) {
    a = ActRowsArgs{}; actFillShared(h, a); a.stMean = nullptr; a.stScale = nullptr;
    a.dS = c.nF; a.dIn = c.nF; a.nL = actFillLayers(h, 1, a.L);
    return panels ? act_rows_panel_plan(&a, force ? ACT_DEV_FORCE_PN : 0) : act_rows_plan(&a);
  };
  if (dense(force)) h->act.devConvPanel = force;
  else if (dense(!force)) h->act.devConvPanel = !force;
  else {
    for (int j = 1; j < h->nHidden; ++j) if (h->hid[j].size > ACT_ROWS_MAXW) return actDevRefuse(h, "a layer beyond 2048");
    return actDevRefuse(h, "the dense layers' activations beyond 160 KB of LDS");
  }
  if (actCus(h) < 1) return actDevRefuse(h, "the device does not say its compute units");
  h->act.devConvOk = 1;
  return true;
}
// recurrent nets on wide inputs on windows in device memory: the time-step-major chain of actTmChain behind a prepare launch that gathers
// the windows from the caller's array itself (rectm.hip: lstm_tm_prepare_acts_dev_kernel) -- every wide-input net hl_create admits
static bool act_dev_tm_ok(hl_learner* h) { return h->wideIn && actTmOk(h) && actCus(h) >= 1; }
// agents per chunk of hl_forward_sequences: ACT_SEQ_CHUNK windows of the batched window kernel; the chains of the other two routes borrow
// the training rows of the first agents-many samples, so a chunk holds no more agents than the local minibatch has samples -- and, behind
// convolutions, no more than whose stacked window rows fit HL_ACT_WIN_STAGE_BYTES of pinned staging (never fewer than one)
static int actChunkCap(hl_learner* h) {
  if (actSeqOk(h)) return ACT_SEQ_CHUNK;
  if (!actTmOk(h) && !actWinOk(h)) return 0;
  size_t cap = (size_t)std::min(h->B, ACT_SEQ_CHUNK);
  if (h->nConv > 0) cap = std::min(cap, (size_t)HL_ACT_WIN_STAGE_BYTES / ((size_t)h->recK * h->dIn * sizeof(float)));
  // (wide inputs: a window of nnBPTTseq + 1 + nAppendedObs states of up to 8192 floats -- the same bound on the staged states)
  if (h->wideIn) cap = std::min(cap, (size_t)HL_ACT_WIN_STAGE_BYTES / ((size_t)(h->recWin + h->nApp) * h->dS * sizeof(float)));
  return (int)std::max(cap, (size_t)1);
}
// a pinned, device-mapped block of zeros
static hipError_t actPinAlloc(unsigned char** pin, size_t bytes) {
  void* p = nullptr;
  const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocMapped);
  if (e == hipSuccess) *pin = static_cast<unsigned char*>(std::memset(p, 0, bytes));
  return e;
}
// the first block: a stage of ACT_MAXROWS rows of hl_forward, or of one window of hl_forward_sequence, and (recurrent nets) from the next multiple of
// 256 bytes on a stage of actChunkCap agents' windows with their tables; behind convolutions its inputs are the agents' stacked window rows [recK][dIn]
static int actPinEnsure(hl_learner* h) {
  if (h->act.pin) return HL_OK;
  const size_t window = (size_t)(std::max(h->recWin, 1) + h->nApp) * h->dS, cap = (size_t)actChunkCap(h);
  const ActCarve few = act_carve(ACT_MAXROWS, h->nOut, std::max((size_t)ACT_MAXROWS * h->dIn, window), ACT_MAXROWS, false);
  const ActCarve chunk = act_carve(cap, h->nOut, h->nConv > 0 ? cap * h->recK * h->dIn : cap * (h->recWin + h->nApp) * h->dS, cap, true);
  const size_t chunkAt = (few.bytes + 256 + 255) & ~(size_t)255;
  HIPCK(actPinAlloc(&h->act.pin, chunkAt + (cap ? chunk.bytes : 0)));
  h->act.few = act_stage(h->act.pin, few);
  if (cap) h->act.chunk = act_stage(h->act.pin + chunkAt, chunk);
  h->act.chunkCap = (int)cap;
  return HL_OK;
}
// a block of `cap` raw rows, their outputs and one stamp per block of 16 rows (the many-row routes)
static int actRowsPinEnsure(hl_learner* h, unsigned char** pin, ActStage* st, int cap) {
  if (*pin) return HL_OK;
  const ActCarve c = act_carve(cap, h->nOut, (size_t)cap * h->dIn, act_rows_blocks(cap), false);
  HIPCK(actPinAlloc(pin, c.bytes));
  *st = act_stage(*pin, c);
  return HL_OK;
}
// n rows in chunks of `cap` through a row stage: per chunk one copy in, a tag, launch(m, tag) -- whose last launch writes stamps(m) stamps --,
// a poll of those stamps, one copy out.  Neither the minibatch buffers nor a minibatch drawn ahead are touched, and the stream is not synchronised
template <typename Launch> static int actRowChunks(hl_learner* h, const ActStage& s, int cap, int (*stamps)(int), int n, const float* states, double* outputs, Launch&& launch) {
  for (int r0 = 0; r0 < n; r0 += cap) {
    const int m = std::min(cap, n - r0);
    std::memcpy(s.in, states + (size_t)r0 * h->dIn, (size_t)m * h->dIn * sizeof(float));
    const unsigned tag = actNextTag(h);
    { int rc = launch(m, tag); if (rc) return rc; }
    { int rc = actWait(h, s.done, stamps(m), tag); if (rc) return rc; }
    std::memcpy(outputs + (size_t)r0 * h->nOut, s.out, (size_t)m * h->nOut * sizeof(double));
  }
  return HL_OK;
}
// n checked windows in chunks of the chunk stage's capacity: per chunk the tables and the states (`stacked`, behind convolutions: every agent's recK
// stacked window rows instead, step k of agent i at row i recK + k; the window kernel reads its rows from Xin, the tables give it the window's length),
// check(m, winMax) -- the route's launch arguments, which may refuse the chunk --, a tag, launch(m, tag, &rc) -- the route's launches, rc an error
// of the training launches among them -- inside ONE timed bracket, a poll of the agents' stamps, one copy out
template <typename Check, typename Launch>
static int actWindowChunks(hl_learner* h, const char* label, bool stacked, int n, const int32_t* nSteps, const float* states, double* outputs, Check&& check, Launch&& launch) {
  { int rc = actPinEnsure(h); if (rc) return rc; }
  const ActStage& s = h->act.chunk;
  const int cap = h->act.chunkCap, K = h->recK;
  size_t first = 0;      // states in front of the chunk
  for (int i0 = 0; i0 < n; i0 += cap) {
    const int m = std::min(cap, n - i0);
    int sum = 0, winMax = 0;
    if (!stacked) {
      act_chunk_tables(nSteps + i0, m, h->recWin, s.off, s.cnt, &sum, &winMax);
      std::memcpy(s.in, states + first * h->dS, (size_t)sum * h->dS * sizeof(float));
    } else for (int i = 0; i < m; ++i) {
      const int steps = nSteps[i0 + i], win = std::min(steps, h->recWin);
      act_stack_window(s.in + (size_t)i * K * h->dIn, states + (first + sum) * h->dS, steps, h->recWin, K, h->nApp, h->dS);
      s.off[i] = i * K * (1 + h->nApp); s.cnt[i] = win; sum += steps; winMax = std::max(winMax, win);
    }
    int rc = check(m, winMax); if (rc) return rc;
    const unsigned tag = actNextTag(h);
    HIPCK(timed(h, label, h->stream, [&] { return launch(m, tag, &rc); }));
    if (rc) return rc;      // (carried out of the bracket: the events of a timed chain are recorded whatever a training launch says)
    rc = actWait(h, s.done, m, tag); if (rc) return rc;
    std::memcpy(outputs + (size_t)i0 * h->nOut, s.out, (size_t)m * h->nOut * sizeof(double));
    first += sum;
  }
  return HL_OK;
}
// the window kernels on B windows: one agent's last `win` states (`ctx` more in front of them for appended observations), or (off, cnt: the per-agent
// tables) a chunk's, workgroup b on agent b's; a stack of two layer types as two launches (lo, up), the lower segment's rows being the upper one's input
struct ActRecPair { RecArgs lo, up; bool split; };
static void actRecPair(hl_learner* h, ActRecPair& p, int B, const float* states, const int* off, const int* cnt, int win, int ctx) {
  p.split = h->recSplit;
  p.lo = actRecArgs(h, p.split ? 0 : -1, B, states, off, cnt, win, ctx);
  if (p.split) p.up = actRecArgs(h, 1, B, states, off, cnt, win, 0);
}
static hipError_t actRecLaunch(hl_learner* h, const ActRecPair& p) {
  const hipError_t e = launch_rec_forward(p.lo, h->stream);
  return e == hipSuccess && p.split ? launch_rec_forward(p.up, h->stream) : e;
}
// the routes that borrow minibatch buffer 0: the minibatch drawn ahead dropped; their device buffers -- raw rows in: convMmax rows for a recurrent
// net behind convolutions (the stacked window rows of a chunk), Mmax otherwise; outputs out: Mmax rows --; the filter layouts
static int actTrainEnsure(hl_learner* h) {
  int rc = dropPresample(h); if (rc) return rc;
  if (!h->act.dS) HIPCK(devAlloc(&h->act.dS, (size_t)(h->recurrent && h->nConv > 0 ? h->convMmax : h->Mmax) * h->dIn));
  if (!h->act.dO) HIPCK(devAlloc(&h->act.dO, (size_t)h->Mmax * h->nOut));
  return ensureConvPrep(h);
}
// ... and their launches: nRows raw rows to the device, standardised into X0, through the whole forward pass or (`rec`) the convolutional front
// followed by the window launches; then the output layer on the first nOut rows.  *rc: what the training launches say
static hipError_t actTrainTail(hl_learner* h, const float* rows, int nRows, const ActRecPair* rec, int nOut, double* out, volatile unsigned* done, unsigned tag, int* rc) {
  hipError_t e = hipMemcpyAsync(h->act.dS, rows, (size_t)nRows * h->dIn * sizeof(float), hipMemcpyHostToDevice, h->stream); if (e != hipSuccess) return e;
  e = launch_act_standardize(h->sc, h->rp, h->act.dS, nRows, h->dS, h->dIn, h->buf[0].X0, h->ldX0, h->stream); if (e != hipSuccess) return e;
  *rc = rec ? launchFront(h, 0, h->stream, /*gather*/false) : launchForward(h, 0, h->stream, false, /*gather*/false); if (*rc) return hipSuccess;
  if (rec) { e = actRecLaunch(h, *rec); if (e != hipSuccess) return e; }
  return actOutput(h, nOut, out, done, tag);
}
}  // extern "C++"

int hl_forward(hl_learner* h, int32_t n, const float* states, double* outputs) {
  if (!h || n < 0 || (n > 0 && (!states || !outputs))) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  if (h->inStep) return fail(h, HL_ERR_STATE, "hl_forward between hl_step_begin and hl_step_end");
  if (h->recurrent) return fail(h, HL_ERR_UNSUPPORTED, "forward of a recurrent net needs the agent's history");
  if (n == 0) return HL_OK;
  // a few agents, dense network: one kernel, states and outputs through pinned host memory (misc.hip: act_forward_kernel)
  if (n <= ACT_MAXROWS && actFewOk(h)) {
    { int rc = actPinEnsure(h); if (rc) return rc; }
    const ActStage& s = h->act.few;
    return actRowChunks(h, s, ACT_MAXROWS, [](int m) { return m; }, n, states, outputs, [&](int m, unsigned tag) -> int {
      HIPCK(launch_act_forward(actFewArgs(h, s.in, s.out, s.done, tag), m, h->stream));
      return HL_OK;
    });
  }
  // more rows than that, or a layer / an input row wider: the whole net per block of 16 rows on the MFMA (actrows.hip: act_rows_kernel),
  // one launch per chunk of ACT_ROWS_CHUNK rows
  // (a net beyond ACT_ROWS_SMALL_NET weights: only from ACT_ROWS_WIDE_MIN_N rows on and where the launches over the training buffers would
  // need two rounds of Mmax rows or more -- below, one workgroup per 16 rows streaming all weights takes longer than they do)
  if (act_rows_ok(h) && (h->act.rowsSmall || (n >= ACT_ROWS_WIDE_MIN_N && n >= 2 * h->Mmax))) {
    { int rc = actRowsPinEnsure(h, &h->act.rowsPin, &h->act.rows, ACT_ROWS_CHUNK); if (rc) return rc; }
    const ActStage& s = h->act.rows;
    return actRowChunks(h, s, ACT_ROWS_CHUNK, act_rows_blocks, n, states, outputs, [&](int m, unsigned tag) -> int {
      ActRowsArgs a = h->act.rowsArgs; a.in = s.in; a.out = s.out; a.done = s.done; a.n = m; a.tag = tag;
      HIPCK(timed(h, "act_rows", h->stream, [&] { return launch_act_rows(a, h->stream); }));
      return HL_OK;
    });
  }
  // convolutions in front of a feed-forward net, any n: per chunk of convCap rows two launches in the learner's stream -- the conv stack, a
  // workgroup per row up to the number of compute units, which reads the raw rows from the mapped staging itself (a device copy ahead of the
  // launch was slower in development, include/smarties_hip_act.h) and writes the chunk's feature rows; the dense layers on those.  The
  // training activations and the prepared filter layouts are not touched either
  if (act_conv_ok(h)) {
    const int cap = h->act.convCap;
    if (!h->act.convFeat) HIPCK(devAlloc(&h->act.convFeat, (size_t)cap * h->act.convArgs.nF));      // (kept if the pinned block fails: the next call tries that again)
    { int rc = actRowsPinEnsure(h, &h->act.convPin, &h->act.conv, cap); if (rc) return rc; }
    const ActStage& s = h->act.conv;
    return actRowChunks(h, s, cap, act_rows_blocks, n, states, outputs, [&](int m, unsigned tag) -> int {
      ActConvArgs c = h->act.convArgs; c.in = s.in; c.feat = h->act.convFeat; c.n = m;
      ActRowsArgs a = h->act.convRowsArgs; a.in = h->act.convFeat; a.out = s.out; a.done = s.done; a.n = m; a.tag = tag;
      HIPCK(timed(h, "act_conv", h->stream, [&] { return launch_act_conv(c, h->act.cus, h->stream); }));
      HIPCK(timed(h, "act_rows", h->stream, [&] { return launch_act_rows(a, h->stream); }));
      return HL_OK;
    });
  }
  { int rc = actTrainEnsure(h); if (rc) return rc; }      // the forward pass borrows minibatch buffer 0
  // (with appended observations a row holds the raw state of step t followed by those of t-1 .. t-nAppendedObs)
  for (int r0 = 0; r0 < n; r0 += h->Mmax) {
    const int m = std::min(h->Mmax, n - r0);
    int rc = HL_OK;
    HIPCK(actTrainTail(h, states + (size_t)r0 * h->dIn, m, nullptr, m, h->act.dO, nullptr, 0, &rc)); if (rc) return rc;
    HIPCK(hipMemcpyAsync(outputs + (size_t)r0 * h->nOut, h->act.dO, (size_t)m * h->nOut * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));
  }
  return HL_OK;
}

int hl_forward_sequence(hl_learner* h, int32_t nSteps, const float* states, double* outputs) {
  if (!h || nSteps < 1 || !states || !outputs) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  if (!h->recurrent) {
    if (h->nApp == 0) return hl_forward(h, 1, states + (size_t)(nSteps - 1) * h->dS, outputs);
    // appended observations: the row hl_forward reads is that of the last step
    std::vector<float> row((size_t)h->dIn);
    act_stack_row(row.data(), states, nSteps - 1, h->nApp, h->dS);
    return hl_forward(h, 1, row.data(), outputs);
  }
  if (h->inStep) return fail(h, HL_ERR_STATE, "hl_forward_sequence between hl_step_begin and hl_step_end");
  // (appended observations: up to nAppendedObs further states in front of the window, which only feed the window's first steps)
  if (nSteps > h->recWin + h->nApp) return fail(h, HL_ERR_BAD_ARG, "more steps than nnBPTTseq + 1 (+ nAppendedObs)");
  const int win = std::min(nSteps, h->recWin);
  ActRecPair rec;
  if (h->nConv > 0) {      // the window's stacked rows through the conv stack (as hl_forward does), then the window kernel on its rows
    int rc = actTrainEnsure(h); if (rc) return rc;
    std::vector<float> rows((size_t)win * h->dIn);
    act_stack_window(rows.data(), states, nSteps, h->recWin, win, h->nApp, h->dS);
    actRecPair(h, rec, 1, h->act.dS, nullptr, nullptr, win, 0);      // (the rows come from Xin; the states only mark the call as acting)
    HIPCK(actTrainTail(h, rows.data(), win, &rec, 1, h->act.dO, nullptr, 0, &rc)); if (rc) return rc;
    HIPCK(hipMemcpyAsync(outputs, h->act.dO, (size_t)h->nOut * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));
    return HL_OK;
  }
  // states and outputs through pinned host memory, completion by stamp (as hl_forward): two launches, no staged copies
  { int rc = actPinEnsure(h); if (rc) return rc; }
  const ActStage& s = h->act.few;
  std::memcpy(s.in, states, (size_t)nSteps * h->dS * sizeof(float));
  const unsigned tag = actNextTag(h);
  actRecPair(h, rec, 1, s.in, nullptr, nullptr, win, nSteps - win);
  HIPCK(actRecLaunch(h, rec));
  HIPCK(actOutput(h, 1, s.out, s.done, tag));
  { int rc = actWait(h, s.done, 1, tag); if (rc) return rc; }
  std::memcpy(outputs, s.out, (size_t)h->nOut * sizeof(double));
  return HL_OK;
}

// n checked windows of a net whose layers run time-step-major (actTmOk): agent i of a chunk is sample row i of ONE chain of launches --
// prepare, the forward diagonals up to the chunk's longest window, the output layer on the chunk's rows of Yout.  The chain borrows rows
// 0 .. m - 1 of the training buffers between steps, as hl_forward_sequence borrows row 0: every training step writes its rows anew
static int actTmChain(hl_learner* h, int n, const int32_t* nSteps, const float* states, double* outputs) {
  const ActStage& s = h->act.chunk;
  RecArgs ra;
  return actWindowChunks(h, "act_tm_chain", false, n, nSteps, states, outputs, [&](int m, int winMax) {
    ra = actRecArgs(h, -1, m, s.in, s.off, s.cnt, winMax, 0);
    return rec_tm_act_ok(ra) ? HL_OK : fail(h, HL_ERR_UNSUPPORTED, "hl_forward_sequences: the time-step-major launches refuse the chunk");
  }, [&](int m, unsigned tag, int*) {
    const hipError_t e = launch_rec_tm_forward(ra, h->stream);
    return e == hipSuccess ? actOutput(h, m, s.out, s.done, tag) : e;
  });
}
// n checked windows of a net whose windows the workgroup-per-sample kernels run (actWinOk): agent i of a chunk is sample i of ONE chain of
// hl_forward_sequence's own launches -- behind convolutions the chunk's stacked rows through the front; the window launch (two for a
// stack of two layer types) with the per-agent tables, workgroup i walking agent i's window alone; the output layer on the chunk's rows
// of Yout.  The chain borrows the training rows of the first m samples between steps, as hl_forward_sequence borrows those of the first
static int actWinChain(hl_learner* h, int n, const int32_t* nSteps, const float* states, double* outputs) {
  const bool conv = h->nConv > 0;
  if (conv) { int rc = actTrainEnsure(h); if (rc) return rc; }      // (as hl_forward_sequence: the front borrows minibatch buffer 0)
  const ActStage& s = h->act.chunk;
  ActRecPair rec;
  return actWindowChunks(h, "act_win_chain", conv, n, nSteps, states, outputs, [&](int m, int winMax) {
    actRecPair(h, rec, m, conv ? h->act.dS : s.in, s.off, s.cnt, winMax, 0);
    return rec_win_act_ok(rec.lo) && (!rec.split || rec_win_act_ok(rec.up)) ? HL_OK : fail(h, HL_ERR_UNSUPPORTED, "hl_forward_sequences: the window kernels refuse the chunk");
  }, [&](int m, unsigned tag, int* rc) {
    if (conv) return actTrainTail(h, s.in, m * h->recK, &rec, m, s.out, s.done, tag, rc);
    const hipError_t e = actRecLaunch(h, rec);
    return e == hipSuccess ? actOutput(h, m, s.out, s.done, tag) : e;
  });
}

// n agents' windows (include/smarties_hip_act.h)
int hl_forward_sequences(hl_learner* h, int32_t n, const int32_t* nSteps, const float* states, double* outputs) {
  if (!h || n < 0 || (n > 0 && (!nSteps || !states || !outputs))) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  if (h->inStep) return fail(h, HL_ERR_STATE, "hl_forward_sequences between hl_step_begin and hl_step_end");
  if (n == 0) return HL_OK;
  const int maxSteps = h->recWin + h->nApp;
  for (int i = 0; i < n; ++i) {
    if (nSteps[i] < 1) return fail(h, HL_ERR_BAD_ARG, "hl_forward_sequences: a window without a state");
    if (h->recurrent && nSteps[i] > maxSteps) return fail(h, HL_ERR_BAD_ARG, "more steps than nnBPTTseq + 1 (+ nAppendedObs)");
  }
  if (!h->recurrent) {
    // dense net: the rows hl_forward reads -- that of every agent's last step -- then ONE call for all agents
    std::vector<float> rows((size_t)n * h->dIn);
    size_t off = 0;
    for (int i = 0; i < n; ++i) { act_stack_row(rows.data() + (size_t)i * h->dIn, states + off * h->dS, nSteps[i] - 1, h->nApp, h->dS); off += nSteps[i]; }
    return hl_forward(h, n, rows.data(), outputs);
  }
  if (actSeqOk(h)) {      // one launch per chunk: a workgroup per agent up to the number of compute units
    const ActStage& s = h->act.chunk;
    return actWindowChunks(h, "act_seq", false, n, nSteps, states, outputs, [](int, int) { return HL_OK; }, [&](int m, unsigned tag, int*) {
      ActSeqArgs a = h->act.seqArgs; a.states = s.in; a.offset = s.off; a.out = s.out; a.done = s.done; a.n = m; a.tag = tag;
      return launch_act_seq(a, std::min(m, h->act.cus), h->stream);
    });
  }
  if (actTmOk(h)) return actTmChain(h, n, nSteps, states, outputs);       // layers wider than 256 cells
  if (actWinOk(h)) return actWinChain(h, n, nSteps, states, outputs);     // convolutions in front, two layer types, a window beyond the batched kernel's LDS
  // a net all three predicates refuse -- layers or inputs beyond the bounds the window kernels state (256 cells, 1024 inputs) that the
  // time-step-major launches do not take either --: hl_forward_sequence's own route, agent by agent, as before
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    const int rc = hl_forward_sequence(h, nSteps[i], states + off * h->dS, outputs + (size_t)i * h->nOut); if (rc) return rc;
    off += nSteps[i];
  }
  return HL_OK;
}
