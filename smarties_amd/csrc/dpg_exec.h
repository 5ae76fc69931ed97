// smarties_amd/csrc/dpg_exec.h -- the second network and the launches of a DPG learner (hl_create_dpg; dpgt.hip) inside the step's launch
// sequence (included by learner.cpp beside naf_exec.h and dqn_exec.h, in front of step_exec.h, whose buildProblems / launchHead /
// launchAdam hand DPG learners over).  The actor is the handle's network and keeps the generic launches; everything of the critic is
// here.  Counters of their own, as NAF's and DQN's launches have: no launch-count table of the nets hl_create serves (tests/blocks.py)
// lists them, and none of them fires on such a net.  tools/dpg_timing.py reads them.
#pragma once

namespace {

void setTiles(GemmProblem& p, int& cursor, bool maySplit);      // (step_exec.h)

constexpr float DPG_CRITIC_ETA = 10.f, DPG_CRITIC_LAMBDA = 1e-4f;      // the DPG constructor: learnrate x 10, nnLambda 1e-4 for the critic

// a critic's description by the Builder's rules (buildNet's, for dense layers): the actor's hidden layers on dIn inputs -- DPG: dimS + dimA,
// PPO (ppo_exec.h): dimS --, one Linear output; the blob's blocks on multiples of 8 floats.  Then its arrays; withTarget: the target copy
// and the target launch's outputs (DPG)
int buildCritic(hl_learner* h, int dIn, bool withTarget) {
  hl_learner::DpgCritic& c = h->critic;
  c.nHidden = h->nHidden; c.dIn = dIn; c.ldX0 = (int)roundUp(c.dIn, 16);
  long long tot = 0; int prev = c.dIn;
  auto block = [&](long long n) { const long long at = tot; tot += roundUp(n, 8); return at; };
  h->criticLay.clear();
  for (int j = 0; j < c.nHidden; ++j) {
    DevHidden& d = c.hid[j]; d = DevHidden{};
    d.nIn = prev; d.size = h->hid[j].size; d.ldW = (int)roundUp(d.size, 8); d.func = h->hid[j].func; d.lstm = 0;
    d.indW = block((long long)d.ldW * d.nIn); d.indB = block(d.size);
    d.hasRes = j > 0 ? 1 : 0; d.resW = std::min(d.nIn, d.size);      // no skip connection after the first layer (Builder.cpp:89-95)
    h->criticLay.push_back({1, d.nIn, d.size, d.ldW, d.indW, d.indB});
    if (d.hasRes) { d.indWr = block(d.size); d.indBr = block(d.size); h->criticLay.push_back({2, 0, d.size, 0, d.indWr, d.indBr}); }
    d.ldA = (int)roundUp(d.size, 16); prev = d.size;
  }
  c.ldWo = 8; c.indWo = block((long long)c.ldWo * prev); c.indBo = block(1);
  h->criticLay.push_back({1, prev, 1, c.ldWo, c.indWo, c.indBo});
  c.nParams = tot;
  const size_t n = (size_t)c.nParams + PARAM_TAIL; const int B = h->B;
  for (float** p : {&c.W, &c.M1, &c.M2, &c.G}) HIPCK(devAlloc(p, n));
  HIPCK(devAlloc(&c.X0, (size_t)B * c.ldX0)); HIPCK(devAlloc(&c.dOut, (size_t)B * c.ldDo));
  if (withTarget) { HIPCK(devAlloc(&c.Wtgt, n)); HIPCK(devAlloc(&c.qT, (size_t)B)); HIPCK(devAlloc(&c.qN, (size_t)B)); HIPCK(devAlloc(&c.dQda, (size_t)B * DPG_MAX_DIMA)); }
  HIPCK(devAlloc(&c.q, (size_t)B)); HIPCK(devAlloc(&c.gOut, (size_t)B));
  for (int j = 0; j < c.nHidden; ++j) {
    DevHidden& d = c.hid[j]; const size_t m = (size_t)B * d.ldA;
    HIPCK(devAlloc(&d.X, m)); HIPCK(devAlloc(&d.Y, m)); HIPCK(devAlloc(&d.D, m)); HIPCK(devAlloc(&d.Dres, m));
    if (d.hasRes) HIPCK(devAlloc(&d.Rr, m));
  }
  return HL_OK;
}
void freeCritic(hl_learner* h) {
  hl_learner::DpgCritic& c = h->critic;
  for (void* p : {(void*)c.W, (void*)c.M1, (void*)c.M2, (void*)c.G, (void*)c.Wtgt, (void*)c.X0, (void*)c.dOut, (void*)c.qT, (void*)c.qN, (void*)c.dQda, (void*)c.q, (void*)c.gOut}) if (p) hipFree(p);
  for (int j = 0; j < HL_MAX_HIDDEN; ++j) for (float* p : {c.hid[j].X, c.hid[j].Y, c.hid[j].Rr, c.hid[j].D, c.hid[j].Dres}) if (p) hipFree(p);
}
// the record of the target launch: both nets' layers as the kernel walks them
DpgNetDesc dpgDesc(const DevHidden* hid, int nHidden, long long indWo, long long indBo, int ldWo) {
  DpgNetDesc n{}; n.nHidden = nHidden; n.func = hid[0].func; n.ldWo = ldWo; n.indWo = indWo; n.indBo = indBo;
  for (int j = 0; j < nHidden; ++j) { const DevHidden& d = hid[j]; n.L[j] = DpgLayer{d.nIn, d.size, d.ldW, d.hasRes, d.resW, d.indW, d.indB, d.indWr, d.indBr}; }
  return n;
}
// bytes of LDS the target launch of this configuration needs (hl_create_dpg's size check, in front of the device query)
size_t dpgTargetLdsOf(const hl_config& cfg) {
  DpgTargetArgs t{}; t.dS = cfg.dimS; t.dA = cfg.dimA; int need = std::max(t.dS + 16, t.dS + t.dA), n = 0;
  for (int j = 0; j < cfg.n_hidden; ++j) if (cfg.hidden[j] > 0 && n < HL_MAX_HIDDEN) { t.critic.L[n++].size = cfg.hidden[j]; need = std::max(need, cfg.hidden[j]); }
  t.critic.nHidden = n; t.ld = (int)roundUp(need, 16) + 4;
  return dpg_target_lds(t);
}

// the critic's forward, dX and dW records (buildProblems appends them): B rows, the same for both minibatch buffers; no input
// gradient of the first layer; no Adam in the epilogues (the optimiser launch takes both nets)
void dpgProblems(hl_learner* h, std::vector<GemmProblem>& P) {
  hl_learner::DpgCritic& c = h->critic; const int nH = c.nHidden, B = h->B;
  c.fwdIdx.clear(); c.fwdBlocks.clear(); c.dxIdx.clear(); c.dxBlocks.clear();
  for (int j = 0; j < nH; ++j) {
    const DevHidden& d = c.hid[j];
    GemmProblem p{}; p.flavor = GEMM_F; p.epi = EPI_FWD; p.M = B; p.N = d.size; p.K = d.nIn; p.dynRows = 0;
    if (j == 0) { p.A = c.X0; p.lda = c.ldX0; }
    else { const DevHidden& q = c.hid[j - 1]; p.A = q.hasRes ? q.Rr : q.Y; p.lda = q.ldA; }
    p.B = c.W + d.indW; p.ldb = d.ldW; p.bias = c.W + d.indB;
    p.C = d.X; p.C2 = d.Y; p.C3 = d.hasRes ? d.Rr : nullptr; p.ldc = d.ldA; p.func = d.func;
    if (d.hasRes) { p.resW = c.W + d.indWr; p.resB = c.W + d.indBr; p.resIn = p.A; p.ldRes = p.lda; p.resN = d.resW; }
    int cur = 0; setTiles(p, cur, false);
    c.fwdIdx.push_back((int)P.size()); c.fwdBlocks.push_back(cur); P.push_back(p);
  }
  for (int j = nH - 1; j >= 1; --j) {
    const DevHidden& d = c.hid[j]; const DevHidden& q = c.hid[j - 1];
    GemmProblem p{}; p.flavor = GEMM_X; p.epi = EPI_DX; p.M = B; p.N = d.nIn; p.K = d.size;
    p.A = d.D; p.lda = d.ldA; p.B = c.W + d.indW; p.ldb = d.ldW;
    p.C = q.Dres; p.C2 = q.D; p.ldc = q.ldA;
    if (d.hasRes) { p.resIn = d.Dres; p.ldRes = d.ldA; p.resW = c.W + d.indWr; p.resN = d.resW; }
    p.actX = q.X; p.actY = q.Y; p.ldAct = q.ldA; p.func = q.func;
    int cur = 0; setTiles(p, cur, false);
    c.dxIdx.push_back((int)P.size()); c.dxBlocks.push_back(cur); P.push_back(p);
  }
  c.dwIdx = (int)P.size(); int cur = 0;
  for (int j = 0; j < nH; ++j) {
    const DevHidden& d = c.hid[j];
    GemmProblem p{}; p.flavor = GEMM_W; p.epi = EPI_DW; p.M = d.nIn + 1; p.N = d.size; p.K = B;
    if (j == 0) { p.A = c.X0; p.lda = c.ldX0; }
    else { const DevHidden& q = c.hid[j - 1]; p.A = q.hasRes ? q.Rr : q.Y; p.lda = q.ldA; }
    p.B = d.D; p.ldb = d.ldA; p.C = c.G + d.indW; p.ldc = d.ldW; p.biasOut = c.G + d.indB;
    setTiles(p, cur, false); P.push_back(p);
    if (d.hasRes) {   // ParametricResidualLayer::backward (Layers.h:363-393)
      GemmProblem r{}; r.flavor = RED_COL; r.epi = EPI_NONE; r.N = d.resW; r.K = B;
      r.A = d.Dres; r.lda = d.ldA; r.B = p.A; r.ldb = p.lda; r.C = c.G + d.indWr;
      setTiles(r, cur, false); P.push_back(r);
      GemmProblem s{}; s.flavor = RED_COL; s.epi = EPI_NONE; s.N = d.resW; s.K = B;
      s.A = d.Dres; s.lda = d.ldA; s.B = nullptr; s.C = c.G + d.indBr;
      setTiles(s, cur, false); P.push_back(s);
    }
  }
  { const DevHidden& q = c.hid[nH - 1];      // the output layer: one column
    GemmProblem p{}; p.flavor = GEMM_W; p.epi = EPI_DW; p.M = q.size + 1; p.N = 1; p.K = B;
    p.A = q.hasRes ? q.Rr : q.Y; p.lda = q.ldA; p.B = c.dOut; p.ldb = c.ldDo;
    p.C = c.G + c.indWo; p.ldc = c.ldWo; p.biasOut = c.G + c.indBo;
    setTiles(p, cur, false); P.push_back(p); }
  c.dwCount = (int)P.size() - c.dwIdx; c.dwBlocks = cur;
}

int dpgGemm(hl_learner* h, const char* name, int role, int flavor, int K, int idx, int blocks, const AdamHyper& hyp, hipStream_t s) {
  const GemmProblem* p = h->dProbs + idx;
  HIPCK(timed(h, name, s, [&] {
    return gemm_oneshot_ok(flavor, K) ? launch_gemm_oneshot(role, p, K, blocks, h->sc, hyp, nullptr, s) : launch_gemm(role, p, 1, blocks, h->sc, hyp, nullptr, s); }));
  return HL_OK;
}
// behind the actor's forward launches: the critic's input rows and forward chain, the target launch, the head, the critic's backward
// (the actor's follows in launchBackward).  Eager steps, no riders
int dpgHead(hl_learner* h, const HeadArgs& ha, int parity, const AdamHyper& hyp, hipStream_t s) {
  hl_learner::DpgCritic& c = h->critic; const int nH = c.nHidden;
  if ((int)c.fwdIdx.size() != nH) return fail(h, HL_ERR_STATE, "DPG: the critic has no problem records");
  const long long* slot = h->buf[parity].bt.slot;
  HIPCK(timed(h, "dpg_critic_gather", s, [&] { return launch_dpg_critic_gather(h->rp, slot, h->buf[parity].X0, h->ldX0, c.X0, c.ldX0, h->dS, h->dA, h->B, s); }));
  for (int j = 0; j < nH; ++j) { const int rc = dpgGemm(h, "dpg_critic_fwd", j == 0 ? GEMM_ROLE_FWD0 : GEMM_ROLE_FWD, GEMM_F, c.hid[j].nIn, c.fwdIdx[j], c.fwdBlocks[j], hyp, s); if (rc) return rc; }
  DpgTargetArgs ta = c.tgt; ta.rp = h->rp; ta.slot = slot; ta.B = h->B; ta.Wa = h->Wtgt; ta.Wc = c.Wtgt; ta.qT = c.qT; ta.qN = c.qN; ta.dQda = c.dQda;
  HIPCK(timed(h, "dpg_target", s, [&] { return launch_dpg_target(ta, s); }));
  const DevHidden& q = c.hid[nH - 1];
  DpgHeadArgs da{}; da.h = ha; da.cYin = q.hasRes ? q.Rr : q.Y; da.cX = q.X; da.cY = q.Y; da.cH = q.size; da.cLd = q.ldA; da.cFunc = q.func;
  da.cW = c.W; da.cIndWo = c.indWo; da.cIndBo = c.indBo; da.cLdWo = c.ldWo; da.cDOut = c.dOut; da.cLdDo = c.ldDo; da.cDres = q.Dres; da.cD = q.D;
  da.qT = c.qT; da.qN = c.qN; da.dQda = c.dQda; da.cQ = c.q; da.cG = c.gOut; da.gamma = h->cfg.gamma; da.explNoise = h->cfg.explNoise;
  HIPCK(timed(h, "head_dpg", s, [&] { return launch_head_dpg(da, s); }));
  for (size_t i = 0; i < c.dxIdx.size(); ++i) { const int rc = dpgGemm(h, "dpg_critic_dx", GEMM_ROLE_DX, GEMM_X, c.hid[nH - 1 - (int)i].size, c.dxIdx[i], c.dxBlocks[i], hyp, s); if (rc) return rc; }
  HIPCK(timed(h, "dpg_critic_dw", s, [&] { return launch_gemm(GEMM_ROLE_DW, h->dProbs + c.dwIdx, c.dwCount, c.dwBlocks, h->sc, hyp, nullptr, s); }));
  return HL_OK;
}
// Adam and the target weights of both nets in one launch (Optimizer.cpp:162-177), NAF's counter rule
int dpgAdam(hl_learner* h, const AdamArgs& aa) {
  int mode = NAF_TGT_KEEP;
  if (h->tgtDelay > 0) {
    if (h->tgtCnt == 0) { h->tgtCnt = (long long)h->tgtDelay; mode = h->tgtDelay >= 1 ? NAF_TGT_COPY : NAF_TGT_POLYAK; }
    if (h->tgtCnt > 0) h->tgtCnt -= 1;
  }
  hl_learner::DpgCritic& c = h->critic;
  DpgAdamArgs da{}; da.a[0] = aa; da.a[1] = aa; da.a[1].W = c.W; da.a[1].M1 = c.M1; da.a[1].M2 = c.M2; da.a[1].G = c.G; da.a[1].n = c.nParams;
  da.a[1].lambda = DPG_CRITIC_LAMBDA; da.T[0] = h->Wtgt; da.T[1] = c.Wtgt; da.etaMul[0] = 1.f; da.etaMul[1] = DPG_CRITIC_ETA; da.mode = mode; da.alpha = h->tgtDelay;
  HIPCK(timed(h, "dpg_adam_target", h->stream, [&] { return launch_dpg_adam_target(da, h->stream); }));
  return HL_OK;
}

}  // namespace
