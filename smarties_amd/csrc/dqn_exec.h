// smarties_amd/csrc/dqn_exec.h -- the launches of a DQN learner (hl_create_dqn; headdq.hip) inside the step's launch sequence (included by
// learner.cpp beside naf_exec.h, in front of step_exec.h, whose launchHead / launchAdam hand DQN learners over).  The gather of the next
// states and the optimiser launch are NAF's kernels as they are; counters of their own, as NAF's launches have: no launch-count table of
// the nets hl_create serves (tests/blocks.py) lists them, and none of them fires on such a net.  tools/dqn_timing.py reads them.
#pragma once

namespace {

// one dense chain over the B next-state rows: a launch per layer on the records buildProblems made for it
int dqnNextChain(hl_learner* h, const char* name, const std::vector<int>& idx, const std::vector<int>& blocks, const AdamHyper& hyp, hipStream_t s) {
  for (int j = 0; j < h->nHidden; ++j) {
    const int role = j == 0 ? GEMM_ROLE_FWD0 : GEMM_ROLE_FWD, nIn = h->hid[j].nIn;
    const GemmProblem* p = h->dProbs + idx[j];
    HIPCK(timed(h, name, s, [&] {
      return gemm_oneshot_ok(GEMM_F, nIn) ? launch_gemm_oneshot(role, p, nIn, blocks[j], h->sc, hyp, nullptr, s)
                                          : launch_gemm(role, p, 1, blocks[j], h->sc, hyp, nullptr, s); }));
  }
  return HL_OK;
}
// the head launch; with returnsEstimator "none" the next states' rows and the dense chain on the live and -- targetDelay > 0 -- on the
// target weights in front of it.  Eager steps, no riders
int dqnHead(hl_learner* h, const HeadArgs& ha, int parity, const AdamHyper& hyp, hipStream_t s) {
  const bool none = h->nafX1 != nullptr, tgt = none && h->tgtY[0] != nullptr;
  if (none) {
    if ((int)h->nxtFwdIdx.size() != h->nHidden || (tgt && (int)h->tgtFwdIdx.size() != h->nHidden)) return fail(h, HL_ERR_STATE, "DQN: the next-state chains have no problem records");
    HIPCK(timed(h, "dqn_next_gather", s, [&] { return launch_naf_next_gather(h->rp, h->buf[parity].bt.slot, h->nafX1, h->ldX0, h->dS, h->B, s); }));
    int rc = dqnNextChain(h, "dqn_nxt_fwd", h->nxtFwdIdx, h->nxtFwdBlocks, hyp, s); if (rc) return rc;
    if (tgt) { rc = dqnNextChain(h, "dqn_tgt_fwd", h->tgtFwdIdx, h->tgtFwdBlocks, hyp, s); if (rc) return rc; }
  }
  const int jl = h->nHidden - 1; const bool res = h->hid[jl].hasRes;
  DqnHeadArgs da{}; da.h = ha; da.retNone = none ? 1 : 0; da.hasTgt = tgt ? 1 : 0; da.gamma = h->cfg.gamma;
  da.Ynxt = none ? (res ? h->nxtR[jl] : h->nxtY[jl]) : nullptr;
  da.Ytgt = tgt ? (res ? h->tgtR[jl] : h->tgtY[jl]) : nullptr;
  da.tgtParams = tgt ? h->Wtgt : nullptr;
  HIPCK(timed(h, "head_dqn", s, [&] { return launch_head_dqn(da, h->Mmax, s); }));
  return HL_OK;
}
// Adam and the target weights in one launch (Optimizer.cpp:162-177), NAF's kernel and NAF's counter rule; targetDelay <= 0: the
// target weights stay as they are
int dqnAdam(hl_learner* h, const AdamArgs& aa) {
  int mode = NAF_TGT_KEEP;
  if (h->tgtDelay > 0) {
    if (h->tgtCnt == 0) { h->tgtCnt = (long long)h->tgtDelay; mode = h->tgtDelay >= 1 ? NAF_TGT_COPY : NAF_TGT_POLYAK; }
    if (h->tgtCnt > 0) h->tgtCnt -= 1;
  }
  HIPCK(timed(h, "dqn_adam_target", h->stream, [&] { return launch_naf_adam_target(aa, h->Wtgt, mode, h->tgtDelay, h->stream); }));
  return HL_OK;
}

}  // namespace
