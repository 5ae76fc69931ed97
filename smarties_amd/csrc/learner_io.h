// smarties_amd/csrc/learner_io.h -- part of learner.cpp's ONE translation unit (included there, like step_exec.h): the reference's file and wire formats -- packed episodes (Episode::packEpisode), the statistics line (Learner::getMetrics), the importance-weight histogram, replay-memory and network checkpoints (MemoryBuffer::save / restart, Network::save)
#pragma once

// ---- episodes in the reference's wire format (Episode::packEpisode / unpackEpisode, Episode.cpp:24-130) ----
int64_t hl_packed_episode_size(const hl_learner* h, int32_t N) {
  if (!h || N < 0) return -1;
  HL_LOCK(h);
  return (int64_t)(h->dS + h->dA + h->polDim + 1 + 6) * N + 10;      // Episode::computeTotalEpisodeSize (Episode.h:211-219)
}
int hl_append_packed_episode(hl_learner* h, const float* data, int64_t n) {
  if (!h || !data) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  const int dS = h->dS, dA = h->dA, pD = h->polDim, tup = dS + 1 + dA + pD;
  const int64_t N = (n - 10) / (tup + 6);
  if (N < 2 || hl_packed_episode_size(h, (int32_t)N) != n) return fail(h, HL_ERR_BAD_ARG, "packed episode has the wrong size");
  std::vector<float> S((size_t)N * dS), V(N), ADV(N);
  std::vector<double> A((size_t)N * dA), MU((size_t)N * pD), R(N);
  const float* buf = data;
  for (int64_t i = 0; i < N; ++i) {      // Episode::unpackEpisode: fp32 -> Fvec states, Real reward, Rvec action / policy
    std::copy(buf, buf + dS, S.begin() + i * dS); R[i] = buf[dS]; buf += dS + 1;
    for (int j = 0; j < dA; ++j) A[i * dA + j] = buf[j];
    buf += dA;
    for (int j = 0; j < pD; ++j) MU[i * pD + j] = buf[j];
    buf += pD;
  }
  buf += N;                                            // returnEstimator: recomputed on insertion
  std::copy(buf, buf + N, ADV.begin()); buf += N;      // actionAdvantage
  std::copy(buf, buf + N, V.begin()); buf += N;        // stateValue
  buf += 3 * N;                                        // deltaValue, offPolicImpW, KullbLeibDiv: reset on insertion
  const char* cp = reinterpret_cast<const char*>(buf);
  bool term; int64_t ID; std::memcpy(&term, cp, sizeof(bool)); std::memcpy(&ID, cp + sizeof(bool), sizeof(int64_t));
  return hl_append_episode(h, (int32_t)N, S.data(), A.data(), MU.data(), R.data(), V.data(), ADV.data(), term ? 1 : 0, ID);
}
int hl_pack_episode(hl_learner* h, int64_t pos, float* dst, int64_t cap) {
  if (!h || !dst || pos < 0 || pos >= (int64_t)h->order.size()) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  const EpMeta e = h->order[(size_t)pos];
  const int dS = h->dS, dA = h->dA, pD = h->polDim; const int64_t N = e.N, total = hl_packed_episode_size(h, e.N);
  if (cap < total) return fail(h, HL_ERR_BAD_ARG, "hl_pack_episode: destination too small");
  int rc = flushPending(h); if (rc) return rc;
  std::vector<float> S((size_t)N * dS), F((size_t)6 * N);
  std::vector<double> A((size_t)N * dA), MU((size_t)N * pD), R(N);
  HIPCK(hipMemcpyAsync(S.data(), h->rp.S + (size_t)e.off * dS, S.size() * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipMemcpyAsync(A.data(), h->rp.A + (size_t)e.off * dA, A.size() * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipMemcpyAsync(MU.data(), h->rp.MU + (size_t)e.off * pD, MU.size() * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipMemcpyAsync(R.data(), h->rp.R + e.off, R.size() * 8, hipMemcpyDeviceToHost, h->stream));
  const float* src[6] = {h->rp.RET, h->rp.ADV, h->rp.V, h->rp.DQ, h->rp.IMPW, h->rp.DKL};   // order of Episode.cpp:48-72
  for (int k = 0; k < 6; ++k) HIPCK(hipMemcpyAsync(F.data() + (size_t)k * N, src[k] + e.off, (size_t)N * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  std::fill(dst, dst + total, 0.f);
  float* buf = dst;
  for (int64_t i = 0; i < N; ++i) {
    std::copy(S.begin() + i * dS, S.begin() + (i + 1) * dS, buf); buf[dS] = (float)R[i]; buf += dS + 1;
    for (int j = 0; j < dA; ++j) buf[j] = (float)A[i * dA + j];
    buf += dA;
    for (int j = 0; j < pD; ++j) buf[j] = (float)MU[i * pD + j];
    buf += pD;
  }
  std::copy(F.begin(), F.end(), buf); buf += 6 * N;
  char* cp = reinterpret_cast<char*>(buf);
  const bool term = e.term; const int64_t ID = e.tag, sampled = e.sampled, agentID = e.agentID;
  std::memcpy(cp, &term, sizeof(bool)); cp += sizeof(bool);
  std::memcpy(cp, &ID, 8); cp += 8; std::memcpy(cp, &sampled, 8); cp += 8; std::memcpy(cp, &agentID, 8);
  return HL_OK;
}

// ---- statistics line (Learner::logStats: MemoryBuffer::getMetrics + AdamOptimizer::getMetrics) ----
static void real2SS(std::ostringstream& B, const double V, const int W, const bool bPos) {   // SstreamUtilities.h:51-63
  B << " " << std::setw(W);
  if (std::fabs(V) >= 1e4) B << std::setprecision(std::max(W - 7 + bPos, 0));
  else if (std::fabs(V) >= 1e3) B << std::setprecision(std::max(W - 6 + bPos, 0));
  else if (std::fabs(V) >= 1e2) B << std::setprecision(std::max(W - 5 + bPos, 0));
  else if (std::fabs(V) >= 1e1) B << std::setprecision(std::max(W - 4 + bPos, 0));
  else B << std::setprecision(std::max(W - 3 + bPos, 0));
  B << std::fixed << V;
}
int hl_metrics(hl_learner* h, char* header, int32_t headerCap, char* line, int32_t lineCap) {
  if (!h) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  hl_stats st; int rc = hl_get_stats(h, &st); if (rc) return rc;
  DevScalars sc; rc = syncScalarsToHost(h, &sc); if (rc) return rc;
  const bool qStats = st.minQ < st.maxQ;
  if (line) {
    std::ostringstream buff;
    real2SS(buff, st.avgReturn, 9, 0); real2SS(buff, (double)sc.rewMean, 6, 0); real2SS(buff, (double)sc.rewStd, 6, 1);
    real2SS(buff, st.avgKLdivergence, 5, 1);
    if (qStats) {
      const double EPS = std::numeric_limits<float>::epsilon();
      real2SS(buff, std::sqrt(std::max(EPS, st.avgSquaredErr)), 6, 1); real2SS(buff, st.maxAbsError, 6, 1);
      // the "dRet" column (MemoryBuffer.cpp:534-544): root-mean-square change of the return estimates in the sweeps since
      // the last line; printing consumes the counters
      long long newCnt = -1;
      if (st.countReturnsEstimateUpdates > 0) {
        const double nRet = (double)std::max<int64_t>(1, st.countReturnsEstimateUpdates), eRet = std::max(EPS, st.sumReturnsEstimateErrors);
        real2SS(buff, std::sqrt(eRet / nRet), 6, 1);
        newCnt = 0;
      }
      st.countReturnsEstimateUpdates = newCnt;
      HIPCK(launch_set_ret_counters(h->sc, newCnt, h->stream));
      real2SS(buff, st.stdevQ, 6, 1); real2SS(buff, st.avgQ, 6, 0); real2SS(buff, st.minQ, 6, 0); real2SS(buff, st.maxQ, 6, 0);
    }
    buff << " " << std::setw(5) << (long)h->order.size();
    buff << " " << std::setw(7) << (long)h->nTransitions;
    buff << " " << std::setw(7) << (long)sc.seenUpd[0];       // nSeenEps() / nSeenSteps(): as of the last updateCounters
    buff << " " << std::setw(8) << (long)sc.seenUpd[1];
    buff << " " << std::setw(7) << (long)st.nFarPolicySteps;
    if (sc.Cmax > 1) real2SS(buff, sc.beta, 6, 1);
    // AdamOptimizer::getMetrics: L2 norm of the whole (padded) weight blob in long double
    std::vector<float> w((size_t)h->nParams);
    rc = hl_get_params(h, w.data(), nullptr, nullptr); if (rc) return rc;
    long double sum = 0; for (float x : w) sum += (long double)x * (long double)x;
    real2SS(buff, (double)std::sqrt(sum), 7, 1);
    const std::string sLine = buff.str();
    if ((int)sLine.size() + 1 > lineCap) return fail(h, HL_ERR_BAD_ARG, "hl_metrics: line buffer too small");
    std::memcpy(line, sLine.c_str(), sLine.size() + 1);
  }
  if (header) {
    std::ostringstream buff;
    buff << "|  avgR  | avgr | stdr | DKL ";
    if (qStats) buff << (st.countReturnsEstimateUpdates >= 0 ? "| RMSE |maxErr| dRet | stdQ | avgQ | minQ | maxQ " : "| RMSE |maxErr| stdQ | avgQ | minQ | maxQ ");
    buff << "| nEp |  nObs | totEp | totObs | nFarP ";
    if (sc.Cmax > 1) buff << "| beta ";
    buff << std::left << std::setfill(' ') << "| " << std::setw(6) << "net";
    const std::string sHead = buff.str();
    if ((int)sHead.size() + 1 > headerCap) return fail(h, HL_ERR_BAD_ARG, "hl_metrics: header buffer too small");
    std::memcpy(header, sHead.c_str(), sHead.size() + 1);
  }
  return HL_OK;
}


// the bounds and the text block of MemoryProcessing::histogramImportanceWeights (MemoryProcessing.cpp:353-389)
static void impwBounds(float bounds[82]) {
  const int nBins = 81;
  const double beg = std::log(1e-3), end = std::log(50.0);
  bounds[0] = 0;
  for (int i = 1; i < nBins; ++i) bounds[i] = (float)std::exp(beg + (end - beg) * (i - 1.0) / (nBins - 2.0));
  bounds[nBins] = std::numeric_limits<float>::max() - 1e2;
}
static std::string impwText(const float bounds[82], const int64_t counts[81], double dataSize) {
  std::ostringstream buff;
  buff << "_____________________________________________________________________";
  buff << "\nOFF-POLICY IMP WEIGHTS HISTOGRAMS\n";
  buff << "weight pi/mu (harmonic mean of histogram's bounds):\n";
  for (int b = 0; b < 81; ++b) { const float x = bounds[b], y = bounds[b + 1]; real2SS(buff, 2 * x * (y / (x + y)), 6, 1); }
  buff << "\nfraction of dataset:\n";
  for (int b = 0; b < 81; ++b) real2SS(buff, counts[b] / dataSize, 6, 1);
  buff << "\n";
  buff << "_____________________________________________________________________";
  return buff.str();
}
int hl_impweight_histogram(hl_learner* h, char* text, int32_t cap, int64_t counts[HL_IMPW_BINS]) {
  if (!h) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  int rc = flushPending(h); if (rc) return rc;
  HistArgs ha{}; ha.rp = h->rp; ha.nEpisodes = (int)h->order.size(); impwBounds(ha.bounds);
  unsigned long long* dCnt = nullptr;
  HIPCK(devAlloc(&dCnt, 81));
  ha.counts = dCnt;
  HIPCK(launch_impw_hist(ha, h->stream));
  unsigned long long hc[81];
  HIPCK(hipMemcpyAsync(hc, dCnt, sizeof(hc), hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  hipFree(dCnt);
  int64_t c64[81]; for (int b = 0; b < 81; ++b) c64[b] = (int64_t)hc[b];
  if (counts) std::memcpy(counts, c64, sizeof(c64));
  if (text) {
    const std::string t = impwText(ha.bounds, c64, (double)h->nTransitions);
    if ((int)t.size() + 1 > cap) return fail(h, HL_ERR_BAD_ARG, "hl_impweight_histogram: text buffer too small");
    std::memcpy(text, t.c_str(), t.size() + 1);
  }
  return HL_OK;
}

// ---- replay memory + ReF-ER state (MemoryBuffer::save / restart, MemoryBuffer.cpp:172-324) ----
static bool copyFile(const std::string& from, const std::string& to) {
  FILE* a = fopen(from.c_str(), "rb"); if (!a) return false;
  FILE* b = fopen(to.c_str(), "wb"); if (!b) { fclose(a); return false; }
  char buf[1 << 16]; size_t n;
  while ((n = fread(buf, 1, sizeof(buf), a)) > 0) fwrite(buf, 1, n, b);
  fclose(a); fclose(b); return true;
}
int hl_save_memory(hl_learner* h, const char* base, int32_t rank) {
  if (!h || !base) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  int rc = flushPending(h); if (rc) return rc;
  DevScalars sc; rc = syncScalarsToHost(h, &sc); if (rc) return rc;
  const int dS = h->dS;
  std::vector<float> mean(dS), scale(dS), stdv(dS);
  HIPCK(hipMemcpy(mean.data(), h->rp.stMean, dS * 4, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(scale.data(), h->rp.stScale, dS * 4, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(stdv.data(), h->rp.stStd, dS * 4, hipMemcpyDeviceToHost));
  const std::string B(base);
  {
    const std::string back = B + "_scaling_backup.raw";
    FILE* f = fopen(back.c_str(), "wb"); if (!f) return fail(h, HL_ERR_IO, "Unable to save into file " + back);
    std::vector<double> V(mean.begin(), mean.end()); fwrite(V.data(), 8, V.size(), f);
    V.assign(scale.begin(), scale.end()); fwrite(V.data(), 8, V.size(), f);
    V.assign(stdv.begin(), stdv.end()); fwrite(V.data(), 8, V.size(), f);
    const double r3[3] = {(double)sc.rewStd, (double)sc.rewScale, (double)sc.rewMean};
    fwrite(r3, 8, 3, f); fclose(f);
    copyFile(back, B + "_scaling.raw");
  }
  char rk[64]; snprintf(rk, sizeof(rk), "_rank_%03u_learner_", (unsigned)rank);
  const std::string fName = B + rk;
  {
    FILE* f = fopen((fName + "status_backup.raw").c_str(), "w"); if (!f) return fail(h, HL_ERR_IO, "Unable to save into file " + fName);
    fprintf(f, "nStoredEps: %lu\n", (unsigned long)h->order.size());
    fprintf(f, "nStoredObs: %lu\n", (unsigned long)h->nTransitions);
    fprintf(f, "nLocalSeenEps: %lu\n", (unsigned long)h->nSeenEps);
    fprintf(f, "nLocalSeenObs: %lu\n", (unsigned long)h->nSeenSteps);
    fprintf(f, "nInitialData: %ld\n", (long)h->nGatheredB4Startup);
    fprintf(f, "nGradSteps: %ld\n", (long)(h->nGradSteps + 1));           // the reference writes counters.nGradSteps + 1
    fprintf(f, "CmaxReFER: %le\n", sc.Cmax);
    fprintf(f, "beta: %le\n", sc.beta);
    fclose(f);
  }
  {
    FILE* f = fopen((fName + "data_backup.raw").c_str(), "wb"); if (!f) return fail(h, HL_ERR_IO, "Unable to save into file " + fName);
    std::vector<float> buf;
    for (long long p = (long long)h->order.size() - 1; p >= 0; --p) {      // oldest first: re-appending restores the order
      const unsigned long N = (unsigned long)h->order[(size_t)p].N;
      buf.resize((size_t)hl_packed_episode_size(h, (int32_t)N));
      rc = hl_pack_episode(h, p, buf.data(), (int64_t)buf.size()); if (rc) { fclose(f); return rc; }
      fwrite(&N, sizeof(unsigned long), 1, f); fwrite(buf.data(), 4, buf.size(), f);
    }
    fclose(f);
  }
  copyFile(fName + "status_backup.raw", fName + "status.raw");
  copyFile(fName + "data_backup.raw", fName + "data.raw");
  return HL_OK;
}
int hl_restart_memory(hl_learner* h, const char* base, int32_t rank) {
  if (!h || !base) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  if (!h->order.empty()) return fail(h, HL_ERR_STATE, "hl_restart_memory needs an empty replay");
  const int dS = h->dS, dA = h->dA;
  const std::string B(base);
  {
    FILE* f = fopen((B + "_scaling.raw").c_str(), "rb");
    if (!f) return fail(h, HL_ERR_IO, "Parameters restart file " + B + "_scaling.raw not found.");
    std::vector<double> V((size_t)3 * dS + 3);
    const size_t got = fread(V.data(), 8, V.size(), f); fclose(f);
    if (got != V.size()) return fail(h, HL_ERR_IO, "Mismatch in restarted file " + B + "_scaling.raw");
    std::vector<float> m(dS), s(dS), d(dS);
    for (int i = 0; i < dS; ++i) { m[i] = (float)V[i]; s[i] = (float)V[dS + i]; d[i] = (float)V[2 * dS + i]; }
    HIPCK(hipMemcpy(h->rp.stMean, m.data(), dS * 4, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(h->rp.stScale, s.data(), dS * 4, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(h->rp.stStd, d.data(), dS * 4, hipMemcpyHostToDevice));
    const float r3[3] = {(float)V[3 * dS + 2], (float)V[3 * dS + 1], (float)V[3 * dS]};   // mean, scale, std
    HIPCK(hipMemcpy(&h->sc->rewMean, &r3[0], 4, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(&h->sc->rewScale, &r3[1], 4, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(&h->sc->rewStd, &r3[2], 4, hipMemcpyHostToDevice));
  }
  char rk[64]; snprintf(rk, sizeof(rk), "_rank_%03u_learner_", (unsigned)rank);
  const std::string fName = B + rk;
  FILE* fs = fopen((fName + "status.raw").c_str(), "r");
  FILE* fd = fopen((fName + "data.raw").c_str(), "rb");
  if (!fs || !fd) { if (fs) fclose(fs); if (fd) fclose(fd); return fail(h, HL_ERR_IO, "Learner status / data restart file " + fName + "*.raw not found"); }
  unsigned long nEps = 0, nObs = 0, seenE = 0, seenO = 0; long nInit = 0, doneGrad = 0; double Cmax = 0, beta = 0;
  int pass = 1;
  pass = pass && 1 == fscanf(fs, "nStoredEps: %lu\n", &nEps);
  pass = pass && 1 == fscanf(fs, "nStoredObs: %lu\n", &nObs);
  pass = pass && 1 == fscanf(fs, "nLocalSeenEps: %lu\n", &seenE);
  pass = pass && 1 == fscanf(fs, "nLocalSeenObs: %lu\n", &seenO);
  pass = pass && 1 == fscanf(fs, "nInitialData: %ld\n", &nInit);
  pass = pass && 1 == fscanf(fs, "nGradSteps: %ld\n", &doneGrad);
  pass = pass && 1 == fscanf(fs, "CmaxReFER: %le\n", &Cmax);
  pass = pass && 1 == fscanf(fs, "beta: %le\n", &beta);
  fclose(fs);
  if (!pass || doneGrad < 0) { fclose(fd); return fail(h, HL_ERR_IO, "Mismatch in restarted file " + fName + "status.raw"); }
  // episodes: unpack, append (same path as fresh ones), then put the stored per-step fields back
  struct Stored { std::vector<float> f6; int N; };
  std::vector<Stored> stored; stored.reserve(nEps);
  const int tup = dS + 1 + dA + h->polDim;
  for (unsigned long i = 0; i < nEps; ++i) {
    unsigned long N = 0;
    if (fread(&N, sizeof(unsigned long), 1, fd) != 1 || N < 2) { fclose(fd); return fail(h, HL_ERR_IO, "Unable to find sequence in " + fName + "data.raw"); }
    std::vector<float> buf((size_t)hl_packed_episode_size(h, (int32_t)N));
    if (fread(buf.data(), 4, buf.size(), fd) != buf.size()) { fclose(fd); return fail(h, HL_ERR_IO, "Truncated " + fName + "data.raw"); }
    int rc = hl_append_packed_episode(h, buf.data(), (int64_t)buf.size()); if (rc) { fclose(fd); return rc; }
    Stored st; st.N = (int)N; st.f6.assign(buf.begin() + (size_t)N * tup, buf.begin() + (size_t)N * (tup + 6));
    stored.push_back(std::move(st));
    const char* cp = reinterpret_cast<const char*>(buf.data() + (size_t)N * (tup + 6)) + sizeof(bool) + 8;
    std::memcpy(&h->order.front().sampled, cp, 8); std::memcpy(&h->order.front().agentID, cp + 8, 8);
  }
  fclose(fd);
  int rc = flushPending(h); if (rc) return rc;            // tables, counters, insertion-time Retrace
  float* dst[6] = {h->rp.RET, h->rp.ADV, h->rp.V, h->rp.DQ, h->rp.IMPW, h->rp.DKL};
  for (size_t i = 0; i < stored.size(); ++i) {           // episode i of the file sits at position nEps-1-i
    const EpMeta& e = h->order[stored.size() - 1 - i];
    for (int k = 0; k < 6; ++k)
      HIPCK(hipMemcpyAsync(dst[k] + e.off, stored[i].f6.data() + (size_t)k * e.N, (size_t)e.N * 4, hipMemcpyHostToDevice, h->stream));
  }
  HIPCK(hipStreamSynchronize(h->stream));
  // counters and ReF-ER state, then Episode::updateCumulative for every episode (MemoryBuffer.cpp:266)
  h->nSeenEps = (long long)seenE; h->nSeenSteps = (long long)seenO; h->nGatheredB4Startup = nInit; h->nGradSteps = doneGrad;
  h->countsDirty = true;
  rc = flushPending(h); if (rc) return rc;
  DevScalars sc; rc = syncScalarsToHost(h, &sc); if (rc) return rc;
  sc.Cmax = Cmax; sc.Cinv = 1 / Cmax; sc.beta = beta; sc.nGradSteps = doneGrad;
  HIPCK(hipMemcpy(h->sc, &sc, sizeof(DevScalars), hipMemcpyHostToDevice));
  rc = runSweep(h, nullptr, (int)h->order.size(), 1, /*skipRetrace*/1); if (rc) return rc;
  // (one-behind replicas: the first step's message carries the counters as restored; no completed moments sum is held)
  HIPCK(hipMemcpyAsync(h->sc->cntPrev, h->sc->cnt, sizeof(h->sc->cnt), hipMemcpyDeviceToDevice, h->stream));
  h->momPrevValid = false;
  HIPCK(hipStreamSynchronize(h->stream));
  if ((unsigned long)h->nTransitions != nObs) return fail(h, HL_ERR_IO, "nStoredObs of the status file does not match the data file");
  h->initialized = true;      // Learner::initializeLearner is skipped for a restarted learner (Learner.cpp:51-54)
  return HL_OK;
}

// ---- checkpoint in the reference's format (Network::save / restart, Network/Network.cpp:22-68) ----
static void packBlob(const hl_learner* h, const std::vector<float>& P, std::vector<float>& out) {
  out.clear();
  for (const auto& l : h->lay) {
    const float* W = P.data() + l.indW; const float* Bv = P.data() + l.indB;
    if (l.type == 1) {
      for (int i = 0; i < l.nIn; ++i) for (int o = 0; o < l.size; ++o) out.push_back(W[o + (long long)l.ld * i]);
      for (int o = 0; o < l.size; ++o) out.push_back(Bv[o]);
    } else if (l.type == 2) {
      for (int o = 0; o < l.size; ++o) out.push_back(W[o]);
      for (int o = 0; o < l.size; ++o) out.push_back(Bv[o]);
    } else if (l.type == 4 || l.type == 5) {     // LSTMLayer::save / MGULayer::save (Layer_LSTM.h:186-197, Layer_GRU.h:248-258): weights, then biases, as they lie
      for (long long w = 0; w < (long long)l.ld * (l.nIn + l.size); ++w) out.push_back(W[w]);
      for (int o = 0; o < l.ld; ++o) out.push_back(Bv[o]);
    } else if (l.type == 6) {                    // Conv2DLayer::save (Layer_Conv2D.h:215-231): filters, then biases, as they lie
      for (int w = 0; w < l.nIn; ++w) out.push_back(W[w]);
      for (int o = 0; o < l.size; ++o) out.push_back(Bv[o]);
    } else for (int o = 0; o < l.size; ++o) out.push_back(Bv[o]);
  }
}
static void unpackBlob(const hl_learner* h, const std::vector<float>& in, std::vector<float>& P) {
  size_t k = 0;
  for (const auto& l : h->lay) {
    float* W = P.data() + l.indW; float* Bv = P.data() + l.indB;
    if (l.type == 1) {
      for (int i = 0; i < l.nIn; ++i) for (int o = 0; o < l.size; ++o) W[o + (long long)l.ld * i] = in[k++];
      for (int o = 0; o < l.size; ++o) Bv[o] = in[k++];
    } else if (l.type == 2) {
      for (int o = 0; o < l.size; ++o) W[o] = in[k++];
      for (int o = 0; o < l.size; ++o) Bv[o] = in[k++];
    } else if (l.type == 4 || l.type == 5) {
      for (long long w = 0; w < (long long)l.ld * (l.nIn + l.size); ++w) W[w] = in[k++];
      for (int o = 0; o < l.ld; ++o) Bv[o] = in[k++];
    } else if (l.type == 6) {
      for (int w = 0; w < l.nIn; ++w) W[w] = in[k++];
      for (int o = 0; o < l.size; ++o) Bv[o] = in[k++];
    } else for (int o = 0; o < l.size; ++o) Bv[o] = in[k++];
  }
}
int hl_save(hl_learner* h, const char* base) {
  if (!h || !base) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  std::vector<float> P[3]; for (auto& v : P) v.resize((size_t)h->nParams);
  int rc = hl_get_params(h, P[0].data(), P[1].data(), P[2].data()); if (rc) return rc;
  const char* suf[3] = {"_weights", "_1stMom", "_2ndMom"};
  std::vector<float> buf;
  for (int b = 0; b < 3; ++b) {
    packBlob(h, P[b], buf);
    // like Network::save: write <name>_backup.raw first, then copy it over <name>.raw
    const std::string name = std::string(base) + suf[b] + ".raw", back = std::string(base) + suf[b] + "_backup.raw";
    for (const std::string& fn : {back, name}) {
      FILE* f = fopen(fn.c_str(), "wb");
      if (!f) return fail(h, HL_ERR_IO, "Unable to save into file " + fn);
      const size_t w = fwrite(buf.data(), sizeof(float), buf.size(), f);
      fclose(f);
      if (w != buf.size()) return fail(h, HL_ERR_IO, "short write to " + fn);
    }
  }
  return HL_OK;
}
int hl_restart(hl_learner* h, const char* base) {
  if (!h || !base) return HL_ERR_BAD_ARG;
  HL_LOCK(h);
  std::vector<float> P[3]; for (auto& v : P) v.resize((size_t)h->nParams);
  int rc = hl_get_params(h, P[0].data(), P[1].data(), P[2].data()); if (rc) return rc;
  size_t n = 0;
  for (const auto& l : h->lay) n += l.type == 1 ? (size_t)l.size * (l.nIn + 1) : (l.type == 2 ? 2 * (size_t)l.size :
                                  (l.type == 4 || l.type == 5 ? (size_t)l.ld * (l.nIn + l.size + 1) :
                                   (l.type == 6 ? (size_t)l.nIn + l.size : (size_t)l.size)));
  const char* suf[3] = {"_weights", "_1stMom", "_2ndMom"};
  for (int b = 0; b < 3; ++b) {
    const std::string name = std::string(base) + suf[b] + ".raw";
    FILE* f = fopen(name.c_str(), "rb");
    if (!f) { if (b == 0) return fail(h, HL_ERR_IO, "Parameters restart file " + name + " not found."); continue; }
    std::vector<float> buf(n + 1);
    const size_t got = fread(buf.data(), sizeof(float), n + 1, f); fclose(f);
    if (got != n) return fail(h, HL_ERR_IO, "Mismatch in restarted file " + name);
    buf.resize(n); unpackBlob(h, buf, P[b]);
  }
  return hl_set_params(h, P[0].data(), P[1].data(), P[2].data());
}

// rollout inference: Approximator::forward(agent) for n states (RACER.cpp:30-59)
// pinned, device-mapped staging of rollout inference: outputs [ACT_MAXROWS][nOut] f64 | states f32 | completion stamps
