// smarties_amd/csrc/naf_exec.h -- the launches of a NAF learner (hl_create_naf; headq.hip) inside the step's launch sequence (included by
// learner.cpp in front of step_exec.h, whose launchHead / launchAdam hand NAF learners over).  Counters of their own: no launch-count
// table of the nets hl_create serves (tests/blocks.py) lists them, and none of them fires on such a net.  tools/naf_timing.py reads them.
#pragma once

namespace {

// returnsEstimator "none": the next states' rows, the dense chain on the target weights (a launch per layer), V_tgt of each row
int nafTarget(hl_learner* h, int parity, const AdamHyper& hyp, hipStream_t s) {
  HIPCK(timed(h, "naf_next_gather", s, [&] { return launch_naf_next_gather(h->rp, h->buf[parity].bt.slot, h->nafX1, h->ldX0, h->dS, h->B, s); }));
  for (int j = 0; j < h->nHidden; ++j) {
    const int role = j == 0 ? GEMM_ROLE_FWD0 : GEMM_ROLE_FWD, nIn = h->hid[j].nIn;
    const GemmProblem* p = h->dProbs + h->tgtFwdIdx[j];
    HIPCK(timed(h, "naf_tgt_fwd", s, [&] {
      return gemm_oneshot_ok(GEMM_F, nIn) ? launch_gemm_oneshot(role, p, nIn, h->tgtFwdBlocks[j], h->sc, hyp, nullptr, s)
                                          : launch_gemm(role, p, 1, h->tgtFwdBlocks[j], h->sc, hyp, nullptr, s); }));
  }
  const int jl = h->nHidden - 1; const DevHidden& q = h->hid[jl];
  HIPCK(timed(h, "naf_vtgt", s, [&] { return launch_naf_vtgt(q.hasRes ? h->tgtR[jl] : h->tgtY[jl], q.ldA, q.size, h->Wtgt + h->indWo, h->ldWo, h->Wtgt + h->indBo, h->cfg.nnOutputFunc, h->nafVtgt, h->B, s); }));
  return HL_OK;
}
// the head launch (and the target path in front of it): eager steps, no riders
int nafHead(hl_learner* h, const HeadArgs& ha, int parity, const AdamHyper& hyp, hipStream_t s) {
  if (h->nafX1) { const int rc = nafTarget(h, parity, hyp, s); if (rc) return rc; }
  NafHeadArgs na{}; na.h = ha; na.nL = h->nAdv; na.retNone = h->nafX1 ? 1 : 0; na.gamma = h->cfg.gamma; na.explNoise = h->cfg.explNoise; na.vTgt = h->nafVtgt;
  HIPCK(timed(h, "head_naf", s, [&] { return launch_head_naf(na, h->Mmax, s); }));
  return HL_OK;
}
// Adam and the target weights in one launch (Optimizer.cpp:162-177; cntUpdateDelay is an unsigned integer there)
int nafAdam(hl_learner* h, const AdamArgs& aa) {
  int mode = NAF_TGT_KEEP;
  if (h->tgtDelay > 0) {
    if (h->tgtCnt == 0) { h->tgtCnt = (long long)h->tgtDelay; mode = h->tgtDelay >= 1 ? NAF_TGT_COPY : NAF_TGT_POLYAK; }
    if (h->tgtCnt > 0) h->tgtCnt -= 1;
  }
  HIPCK(timed(h, "naf_adam_target", h->stream, [&] { return launch_naf_adam_target(aa, h->Wtgt, mode, h->tgtDelay, h->stream); }));
  return HL_OK;
}

}  // namespace
