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
// give up after 2 s and fall back to it.  `st`: the stream the stamping kernel runs on
static int actWaitOn(hl_learner* h, hipStream_t st, volatile unsigned* pDone, int n, unsigned tag) {
  const auto t0 = std::chrono::steady_clock::now();
  for (int r = 0; r < n; ++r)
    while (pDone[r] != tag) {
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) { HIPCK(hipStreamSynchronize(st)); break; }
    }
  std::atomic_thread_fence(std::memory_order_acquire);
  return HL_OK;
}
static int actWait(hl_learner* h, volatile unsigned* pDone, int n, unsigned tag) { return actWaitOn(h, h->stream, pDone, n, tag); }
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
// ---- the two builders of the argument records (no plan yet: the plans of kernels.h and act_plan.h fill in the LDS layout) ----
// the conv stack, from h->cg[]
static ActConvArgs actConvRecord(const hl_learner* h) {
  ActConvArgs c{};
  c.W = h->W; c.stMean = h->rp.stMean; c.stScale = h->rp.stScale;
  c.dS = h->dS; c.dIn = h->dIn; c.nL = h->nConv; c.recurrent = h->recurrent ? 1 : 0;
  for (int l = 0; l < h->nConv; ++l) { const ConvGeo& g = h->cg[l];
    c.L[l] = ActConvLayer{g.InC, g.InY, g.InX, g.KnC, g.KnY, g.KnX, g.S, g.OpY, g.OpX, g.K, g.P, g.indW, g.indB, 0, 0, 0}; }
  return c;
}
// the dense layers hid[first ..]: on raw rows, standardised on load (nF = 0), or on feature rows [extras | last map] of nF columns, standardised already
static ActRowsArgs actDenseRecord(const hl_learner* h, int first, int nF) {
  ActRowsArgs a{}; actFillShared(h, a);
  if (nF) a.stMean = a.stScale = nullptr;
  a.dS = nF ? nF : h->dS; a.dIn = nF ? nF : h->dIn; a.nL = actFillLayers(h, first, a.L);
  return a;
}
// ---- the resolved table (ActRoutes, learner_state.h).  SMARTIES_HIP_GENERIC bit 2 refuses every LDS route (the training buffers serve);
// bit 4096 holds the host conv row-size switch open; bit 8192 sends every net the banded / panelled kernels of actband.hip can run through
// them -- three bands, panels of 64 columns --, nets the resident kernels serve among them (tests: the two forms give the same bits):
// the forced form is tried first, then the other one
constexpr int ACT_DEV_FORCE_NB = 3, ACT_DEV_FORCE_PN = 64;
static const ActRoutes& actResolve(hl_learner* h) {
  ActRoutes& r = h->act.routes;
  if (r.resolved) return r;
  static const float noState = 0.f;      // (rec_tm_act_ok and rec_win_act_ok ask for given states, they do not read them)
  const bool lds = !(h->generic & 2), force = (h->generic & 8192) != 0, dense = !h->recurrent && h->nConv == 0;
  // a conv stack's plan serves the net: the geometry hl_create built, the feature row the first dense layer reads
  auto convFits = [&](ActConvArgs& c, bool planned) { if (!planned || c.extras != h->extras || c.nF != h->hid[1].nIn) return false; c.ldF = c.nF; return true; };
  // 1. a few rows of a dense net, one workgroup per row (misc.hip: act_forward_kernel): layers and input rows within its bounds
  r.few = dense && lds && h->dIn <= ACT_MAXW;
  for (int j = 0; j < h->nHidden; ++j) if (h->hid[j].size > ACT_MAXW || h->hid[j].nIn > ACT_MAXW) r.few = false;
  // 2. the row-block kernel (actrows.hip): dense, input rows and layers within its bounds
  if (dense && lds && h->dIn <= ACT_ROWS_MAXW) {
    ActRowsArgs a = actDenseRecord(h, 0, 0);
    if (act_rows_plan(&a)) {
      long long nW = (long long)h->hid[h->nHidden - 1].size * h->ldWo;
      for (int j = 0; j < h->nHidden; ++j) nW += (long long)h->hid[j].nIn * h->hid[j].ldW;
      r.rowsArgs = a; r.rows = true; r.rowsSmall = nW <= ACT_ROWS_SMALL_NET;
    }
  }
  // 3. the conv-stack kernel (actconv.hip) and the row-block kernel on hid[1 ..] behind it: feed-forward, image and maps within a workgroup's
  // LDS, feature rows and dense layers within the row-block kernel's bounds.  Wherever the rows lie: hl_forward and the device window calls
  // (resolved with everything else at the first acting call of any family, under bit 8192 too: actCus is then asked at calls that did not
  // ask it before the table existed -- hl_forward on rows beyond the row-size switch, for one; a device attribute, no result depends on when)
  if (h->nConv >= 1 && h->nHidden >= 2 && lds) {
    ActConvArgs c = actConvRecord(h);
    if (convFits(c, act_conv_plan(&c))) {
      ActRowsArgs a = actDenseRecord(h, 1, c.nF);
      if (act_rows_plan(&a) && actCus(h) >= 1) { r.convArgs = c; r.convRowsArgs = a; r.convPlan = true; }
    }
  }
  // 4. ... and hl_forward takes that route: rows in HOST memory go through pinned staging, and beyond HL_ACT_CONV_MAX_ROW_BYTES the copy costs
  // more than the route saves (the header's figures).  Rows per chunk: no more than HL_ACT_CONV_STAGE_BYTES of staged raw rows, whole
  // blocks of 16 rows, at least one
  r.conv = r.convPlan && ((size_t)h->dIn * sizeof(float) <= (size_t)HL_ACT_CONV_MAX_ROW_BYTES || (h->generic & 4096));
  if (r.conv) r.convCap = std::max(16, (int)(std::min((size_t)ACT_ROWS_CHUNK, (size_t)HL_ACT_CONV_STAGE_BYTES / ((size_t)h->dIn * sizeof(float))) & ~(size_t)15));
  // 5. the batched window kernel (actseq.hip): one recurrent layer type, no convolutions in front, layers within its bounds (wide inputs: 6.)
  if (h->recurrent && h->nConv == 0 && !h->recSplit && !h->wideIn) {
    const RecArgs ra = recArgs(h, 0);
    ActSeqArgs a{}; actFillShared(h, a);
    a.dS = h->dS; a.nApp = h->nApp; a.recWin = h->recWin; a.nL = ra.nL; a.gates = ra.gates; a.func = ra.func;
    for (int j = 0; j < ra.nL; ++j) { const RecLayer& L = ra.L[j]; a.L[j] = ActSeqLayer{L.nIn, L.nC, L.hasRes, L.resW, L.indW, L.indB, L.indWr, L.indBr, 0, 0}; }
    if (act_seq_plan(&a) && actCus(h) >= 1) { r.seqArgs = a; r.seq = true; }
  }
  // 6. the time-step-major launches (rectm.hip) serve the net's acting window -- hl_forward_sequence's route where a layer is wider than 256
  // cells or the input wide --: many agents' windows then run as the samples of one chain of those launches
  r.tm = h->recurrent && h->nConv == 0 && !h->recSplit && rec_tm_act_ok(actRecArgs(h, -1, 1, &noState, nullptr, nullptr, 1, 0));
  // 7. the workgroup-per-sample window kernels (rec.hip) serve it -- hl_forward_sequence's route for every net 5. and 6. leave: convolutions in
  // front, RNN encoder layers under MGU layers, a window beyond the batched kernel's LDS --: workgroup b on agent b's window
  r.win = h->recurrent;
  for (int seg = h->recSplit ? 0 : -1; r.win && seg < (h->recSplit ? 2 : 0); ++seg) r.win = rec_win_act_ok(actRecArgs(h, seg, 1, &noState, nullptr, nullptr, 1, 0));
  // ... and behind convolutions the nets beyond those kernels (hl_learner::convTm) keep the shape of that chain -- the chunk's stacked rows through
  // the front -- with the time-step-major launches behind it, the agents as their samples, the feature rows as their wide input rows
  if (h->convTm) r.win = rec_tm_act_ok(actRecArgs(h, -1, 1, &noState, nullptr, nullptr, 1, 0));
  // 8. dense nets on rows in device memory, which can be streamed: the row-block kernel where 2. serves the net, act_rows_panel_kernel on
  // input rows up to ACT_DEV_MAX_ROW wide otherwise
  const char* why = nullptr;
  if (!dense) why = "a recurrent net or convolutions in front";
  else if (!lds) why = "SMARTIES_HIP_GENERIC bit 2";
  else {
    auto panels = [&] {
      ActRowsArgs a = actDenseRecord(h, 0, 0);
      if (!act_rows_panel_plan(&a, force ? ACT_DEV_FORCE_PN : 0)) return false;
      r.panelArgs = a; r.devRows = &r.panelArgs; r.devRowsPanel = true;
      return true;
    };
    bool served = force && panels();                                         // the forced form first
    if (!served && r.rows) { r.devRows = &r.rowsArgs; served = true; }       // the resident plan of 2.
    if (!served && !force) served = panels();                                // beyond it: panels
    if (!served) {
      why = "the layers' activations beyond 160 KB of LDS";
      for (int j = 0; j < h->nHidden; ++j) if (h->hid[j].size > ACT_ROWS_MAXW) why = "a layer beyond 2048";
      if (h->dIn > ACT_DEV_MAX_ROW) why = "an input row beyond HL_ACT_DEV_MAX_ROW = 8192";
    }
  }
  if (h->recurrent) r.devRowsNo = ": recurrent nets act on windows in host memory (hl_forward_sequences)";
  else if (h->nConv > 0) r.devRowsNo = ": nets with convolutional layers in front act on windows in device memory (hl_forward_sequences_dev; without appended observations: windows of one state)";
  else if (why) r.devRowsNo = std::string(": an input row beyond 8192 or a layer beyond 2048, or SMARTIES_HIP_GENERIC bit 2 -- here: ") + why;
  // 9. windows in device memory.  Recurrent nets: on wide inputs the time-step-major chain behind a prepare launch that gathers the windows
  // itself (rectm.hip: lstm_tm_prepare_acts_dev_kernel; live source only: the chain borrows training rows, tmT / tmSteps and the last hidden
  // layer's activations, which a step queued beside it writes), otherwise the batched window kernel of 5.  Dense nets: 8. behind a stacking
  // launch.  Feed-forward nets behind convolutions: the two launches of 3. whatever the row size; beyond that plan act_conv_band_dev_kernel
  // where the image does not fit beside the maps, act_rows_panel_kernel where the feature row is beyond ACT_ROWS_MAXW
  const char* host = ": this net acts on windows in host memory (hl_forward_sequences); served here: ";
  if (h->recurrent) {
    if (h->wideIn && r.tm && actCus(h) >= 1) r.devSeq = ACT_DEV_SEQ_TM;
    else if (r.seq) { r.devSeq = ACT_DEV_SEQ_BATCHED; r.devSeqSnap = true; }
    else r.devSeqNo = std::string(host) + "one recurrent layer type without convolutions or encoder_rnn, layers up to 256 cells and 1024 inputs or wide inputs";
  } else if (h->nConv > 0) {
    why = nullptr;
    if (h->nHidden < 2) why = "a recurrent net, or no convolutions in front of dense layers";
    else if (!lds) why = "SMARTIES_HIP_GENERIC bit 2";
    else if (!force && r.convPlan) { r.devConv = &r.convArgs; r.devConvRows = &r.convRowsArgs; }
    else {      // (both records are planned on locals and committed together, once nothing refuses the net any more)
      ActConvArgs c{}; ActRowsArgs a{}; bool bands = force, panels = force;
      auto conv = [&](bool b) { c = actConvRecord(h); bands = b; return convFits(c, b ? act_conv_band_plan(&c, force ? ACT_DEV_FORCE_NB : 0) : act_conv_wide_plan(&c)); };
      auto denseBehind = [&](bool p) { a = actDenseRecord(h, 1, c.nF); panels = p; return p ? act_rows_panel_plan(&a, force ? ACT_DEV_FORCE_PN : 0) : act_rows_plan(&a); };
      if (!conv(force) && !conv(!force)) {
        c = actConvRecord(h); long long tab, buf[2];
        why = act_conv_geometry(&c, &tab, buf) ? "a map of the conv stack beyond 160 KB of LDS at any band count" : "a feature row beyond HL_ACT_DEV_MAX_ROW = 8192, or the stack's geometry";
      } else if (!denseBehind(force) && !denseBehind(!force)) {
        why = "the dense layers' activations beyond 160 KB of LDS";
        for (int j = 1; j < h->nHidden; ++j) if (h->hid[j].size > ACT_ROWS_MAXW) why = "a layer beyond 2048";
      } else if (actCus(h) < 1) why = "the device does not say its compute units";
      else { r.bandArgs = c; r.panelArgs = a; r.devConv = &r.bandArgs; r.devConvRows = &r.panelArgs; r.devConvBand = bands; r.devConvPanel = panels; }
    }
    if (why) r.devSeqNo = std::string(": this net acts on rows in host memory (hl_forward); served here behind convolutions: every map within 160 KB of LDS beside a band of the image, feature rows up to 8192 and dense layers up to 2048 wide, SMARTIES_HIP_GENERIC bit 2 clear -- here: ") + why;
    else { r.devSeq = ACT_DEV_SEQ_CONV; r.devSeqSnap = true; }
  } else if (r.devRows) { r.devSeq = ACT_DEV_SEQ_ROWS; r.devSeqSnap = true; }
  else r.devSeqNo = std::string(host) + "dense nets with input rows up to 8192 and layers up to 2048 wide, SMARTIES_HIP_GENERIC bit 2 clear -- here: " + why;
  r.resolved = true;
  return r;
}
// ---- the choice per call, on the resolved table and n.  Rows in host memory: a few rows the one-kernel route; the row-block route (a net
// beyond ACT_ROWS_SMALL_NET weights: only from ACT_ROWS_WIDE_MIN_N rows on and where the launches over the training buffers would need two
// rounds of Mmax rows or more -- below, one workgroup per 16 rows streaming all weights takes longer than they do); behind convolutions
// the conv-stack route; the forward pass over the training buffers
enum ActRowsRoute { ACT_ROWS_FEW, ACT_ROWS_BLOCK, ACT_ROWS_CONV, ACT_ROWS_TRAIN };
static ActRowsRoute actRowsRoute(const hl_learner* h, const ActRoutes& r, int n) {
  if (n <= ACT_MAXROWS && r.few) return ACT_ROWS_FEW;
  if (r.rows && (r.rowsSmall || (n >= ACT_ROWS_WIDE_MIN_N && n >= 2 * h->Mmax))) return ACT_ROWS_BLOCK;
  return r.conv ? ACT_ROWS_CONV : ACT_ROWS_TRAIN;
}
// windows in host memory: a dense net's through hl_forward, then the first of 5., 6., 7. that serves the net, else agent by agent
enum ActWindowsRoute { ACT_WIN_DENSE, ACT_WIN_BATCHED, ACT_WIN_TM, ACT_WIN_CHAIN, ACT_WIN_EACH };
static ActWindowsRoute actWindowsRoute(const hl_learner* h, const ActRoutes& r) {
  return !h->recurrent ? ACT_WIN_DENSE : r.seq ? ACT_WIN_BATCHED : r.tm ? ACT_WIN_TM : r.win ? ACT_WIN_CHAIN : ACT_WIN_EACH;
}
// rows in device memory of a net 8. serves: as hl_forward picks the one-kernel route (the same bits), else the row-block kernel or its panelled form
enum ActDevRowsRoute { ACT_DEV_ROWS_FEW, ACT_DEV_ROWS_BLOCK, ACT_DEV_ROWS_PANEL };
static ActDevRowsRoute actDevRowsRoute(const ActRoutes& r, int n) {
  return n <= ACT_MAXROWS && r.few ? ACT_DEV_ROWS_FEW : r.devRowsPanel ? ACT_DEV_ROWS_PANEL : ACT_DEV_ROWS_BLOCK;
}
// agents per chunk of hl_forward_sequences: ACT_SEQ_CHUNK windows of the batched window kernel; the two chains borrow the training rows of
// the first agents-many samples, so a chunk holds no more agents than the local minibatch has samples -- and, behind convolutions, no more
// than whose stacked window rows fit HL_ACT_WIN_STAGE_BYTES of pinned staging (never fewer than one)
static int actChunkCap(hl_learner* h) {
  const ActWindowsRoute route = actWindowsRoute(h, actResolve(h));
  if (route == ACT_WIN_BATCHED) return ACT_SEQ_CHUNK;
  if (route != ACT_WIN_TM && route != ACT_WIN_CHAIN) return 0;
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
  const ActRoutes& r = actResolve(h);
  switch (actRowsRoute(h, r, n)) {
  // a few agents, dense network: one kernel, states and outputs through pinned host memory (misc.hip: act_forward_kernel)
  case ACT_ROWS_FEW: {
    { int rc = actPinEnsure(h); if (rc) return rc; }
    const ActStage& s = h->act.few;
    return actRowChunks(h, s, ACT_MAXROWS, [](int m) { return m; }, n, states, outputs, [&](int m, unsigned tag) -> int {
      HIPCK(launch_act_forward(actFewArgs(h, s.in, s.out, s.done, tag), m, h->stream));
      return HL_OK;
    });
  }
  // more rows than that, or a layer / an input row wider: the whole net per block of 16 rows on the MFMA (actrows.hip: act_rows_kernel),
  // one launch per chunk of ACT_ROWS_CHUNK rows
  case ACT_ROWS_BLOCK: {
    { int rc = actRowsPinEnsure(h, &h->act.rowsPin, &h->act.rows, ACT_ROWS_CHUNK); if (rc) return rc; }
    const ActStage& s = h->act.rows;
    return actRowChunks(h, s, ACT_ROWS_CHUNK, act_rows_blocks, n, states, outputs, [&](int m, unsigned tag) -> int {
      ActRowsArgs a = r.rowsArgs; a.in = s.in; a.out = s.out; a.done = s.done; a.n = m; a.tag = tag;
      HIPCK(timed(h, "act_rows", h->stream, [&] { return launch_act_rows(a, h->stream); }));
      return HL_OK;
    });
  }
  // convolutions in front of a feed-forward net, any n: per chunk of convCap rows two launches in the learner's stream -- the conv stack, a
  // workgroup per row up to the number of compute units, which reads the raw rows from the mapped staging itself (a device copy ahead of the
  // launch was slower in development, include/smarties_hip_act.h) and writes the chunk's feature rows; the dense layers on those.  The
  // training activations and the prepared filter layouts are not touched either
  case ACT_ROWS_CONV: {
    const int cap = r.convCap;
    if (!h->act.convFeat) HIPCK(devAlloc(&h->act.convFeat, (size_t)cap * r.convArgs.nF));      // (kept if the pinned block fails: the next call tries that again)
    { int rc = actRowsPinEnsure(h, &h->act.convPin, &h->act.conv, cap); if (rc) return rc; }
    const ActStage& s = h->act.conv;
    return actRowChunks(h, s, cap, act_rows_blocks, n, states, outputs, [&](int m, unsigned tag) -> int {
      ActConvArgs c = r.convArgs; c.in = s.in; c.feat = h->act.convFeat; c.n = m;
      ActRowsArgs a = r.convRowsArgs; a.in = h->act.convFeat; a.out = s.out; a.done = s.done; a.n = m; a.tag = tag;
      HIPCK(timed(h, "act_conv", h->stream, [&] { return launch_act_conv(c, h->act.cus, h->stream); }));
      HIPCK(timed(h, "act_rows", h->stream, [&] { return launch_act_rows(a, h->stream); }));
      return HL_OK;
    });
  }
  case ACT_ROWS_TRAIN: break;
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

// n checked windows of a net whose layers run time-step-major (ActRoutes::tm): agent i of a chunk is sample row i of ONE chain of launches --
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
// n checked windows of a net whose windows the workgroup-per-sample kernels run (ActRoutes::win): agent i of a chunk is sample i of ONE chain of
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
    if (h->convTm) return rec_tm_act_ok(rec.lo) ? HL_OK : fail(h, HL_ERR_UNSUPPORTED, "hl_forward_sequences: the time-step-major launches refuse the chunk");
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
  const ActRoutes& r = actResolve(h);
  size_t off = 0;
  switch (actWindowsRoute(h, r)) {
  case ACT_WIN_DENSE: {
    // dense net: the rows hl_forward reads -- that of every agent's last step -- then ONE call for all agents
    std::vector<float> rows((size_t)n * h->dIn);
    for (int i = 0; i < n; ++i) { act_stack_row(rows.data() + (size_t)i * h->dIn, states + off * h->dS, nSteps[i] - 1, h->nApp, h->dS); off += nSteps[i]; }
    return hl_forward(h, n, rows.data(), outputs);
  }
  case ACT_WIN_BATCHED: {      // one launch per chunk: a workgroup per agent up to the number of compute units
    const ActStage& s = h->act.chunk;
    return actWindowChunks(h, "act_seq", false, n, nSteps, states, outputs, [](int, int) { return HL_OK; }, [&](int m, unsigned tag, int*) {
      ActSeqArgs a = r.seqArgs; a.states = s.in; a.offset = s.off; a.out = s.out; a.done = s.done; a.n = m; a.tag = tag;
      return launch_act_seq(a, std::min(m, h->act.cus), h->stream);
    });
  }
  case ACT_WIN_TM: return actTmChain(h, n, nSteps, states, outputs);         // layers wider than 256 cells, wide inputs
  case ACT_WIN_CHAIN: return actWinChain(h, n, nSteps, states, outputs);     // convolutions in front, two layer types, a window beyond the batched kernel's LDS
  // a net all three refuse -- layers or inputs beyond the bounds the window kernels state (256 cells, 1024 inputs) that the
  // time-step-major launches do not take either --: hl_forward_sequence's own route, agent by agent, as before
  case ACT_WIN_EACH: break;
  }
  for (int i = 0; i < n; ++i) {
    const int rc = hl_forward_sequence(h, nSteps[i], states + off * h->dS, outputs + (size_t)i * h->nOut); if (rc) return rc;
    off += nSteps[i];
  }
  return HL_OK;
}
