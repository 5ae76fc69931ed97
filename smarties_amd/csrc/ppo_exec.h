// smarties_amd/csrc/ppo_exec.h -- the second network, the launches and the on-policy life cycle of a PPO learner (hl_create_ppo;
// headppo.hip) inside the step's launch sequence (included by learner.cpp beside dpg_exec.h, in front of step_exec.h, whose
// buildProblems / launchHead / launchAdam hand PPO learners over).  The actor is the handle's network and keeps the generic launches; the
// critic is dpg_exec.h's second net (buildCritic, dpgProblems, dpgGemm) on the state rows, without target weights.  Counters of their own,
// as NAF's, DQN's and DPG's launches have: no launch-count table of the nets hl_create serves lists them, and none of them fires on such
// a net.  tools/ppo_timing.py reads them.
#pragma once

namespace {

constexpr float PPO_CRITIC_ETA = 3.f;      // PPO_common.cpp:71: settings.learnrate *= 3 in front of the critic's construction

// behind the actor's forward launches: the critic's rows and forward chain, the head, the critic's backward (the actor's follows in
// launchBackward).  Eager steps, no riders
int ppoHead(hl_learner* h, const HeadArgs& ha, int parity, const AdamHyper& hyp, hipStream_t s) {
  hl_learner::DpgCritic& c = h->critic; const int nH = c.nHidden;
  if ((int)c.fwdIdx.size() != nH) return fail(h, HL_ERR_STATE, "PPO: the critic has no problem records");
  // (one set of records for both minibatch buffers: the standardised state rows of the buffer in use, copied)
  HIPCK(hipMemcpyAsync(c.X0, h->buf[parity].X0, (size_t)h->B * h->ldX0 * sizeof(float), hipMemcpyDeviceToDevice, s));
  for (int j = 0; j < nH; ++j) { const int rc = dpgGemm(h, "ppo_critic_fwd", j == 0 ? GEMM_ROLE_FWD0 : GEMM_ROLE_FWD, GEMM_F, c.hid[j].nIn, c.fwdIdx[j], c.fwdBlocks[j], hyp, s); if (rc) return rc; }
  const DevHidden& q = c.hid[nH - 1];
  PpoHeadArgs pa{}; pa.h = ha; pa.cYin = q.hasRes ? q.Rr : q.Y; pa.cX = q.X; pa.cY = q.Y; pa.cH = q.size; pa.cLd = q.ldA; pa.cFunc = q.func;
  pa.cW = c.W; pa.cIndWo = c.indWo; pa.cIndBo = c.indBo; pa.cLdWo = c.ldWo; pa.cDOut = c.dOut; pa.cLdDo = c.ldDo; pa.cDres = q.Dres; pa.cD = q.D;
  pa.cV = c.q; pa.cG = c.gOut; pa.gain = h->ppoSt.gain; pa.rowStat = h->ppoSt.rowStat; pa.pen = h->ppoSt.pen; pa.Cpol = h->cfg.clipImpWeight;
  HIPCK(timed(h, "head_ppo", s, [&] { return launch_head_ppo(pa, s); }));
  for (size_t i = 0; i < c.dxIdx.size(); ++i) { const int rc = dpgGemm(h, "ppo_critic_dx", GEMM_ROLE_DX, GEMM_X, c.hid[nH - 1 - (int)i].size, c.dxIdx[i], c.dxBlocks[i], hyp, s); if (rc) return rc; }
  HIPCK(timed(h, "ppo_critic_dw", s, [&] { return launch_gemm(GEMM_ROLE_DW, h->dProbs + c.dwIdx, c.dwCount, c.dwBlocks, h->sc, hyp, nullptr, s); }));
  return HL_OK;
}
// Adam of both nets and the serial penalty / DKL_target chain in one launch
int ppoAdam(hl_learner* h, const AdamArgs& aa) {
  hl_learner::DpgCritic& c = h->critic;
  DpgAdamArgs da{}; da.a[0] = aa; da.a[1] = aa; da.a[1].W = c.W; da.a[1].M1 = c.M1; da.a[1].M2 = c.M2; da.a[1].G = c.G; da.a[1].n = c.nParams;
  da.etaMul[0] = 1.f; da.etaMul[1] = PPO_CRITIC_ETA; da.mode = NAF_TGT_KEEP;      // (the critic's nnLambda is the settings': PPO changes learnrate and nnOutputFunc alone)
  PpoAdamArgs pp{}; pp.rowStat = h->ppoSt.rowStat; pp.pen = h->ppoSt.pen; pp.B = h->B;
  HIPCK(timed(h, "ppo_adam", h->stream, [&] { return launch_ppo_adam(da, pp, h->stream); }));
  return HL_OK;
}

// hl_ppo_values: the row-block acting launch on the critic's record
int ppoValuesLaunch(hl_learner* h, const ActRowsArgs& a) {
  HIPCK(timed(h, "ppo_values", h->stream, [&] { return launch_act_rows(a, h->stream); }));
  return HL_OK;
}

}  // namespace
