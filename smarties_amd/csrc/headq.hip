// smarties_amd/csrc/headq.hip -- NAF learners (include/smarties_hip_naf.h): output layer + head with the triangular-matrix advantage, and
// the launches of the target path.
//
//   output InnerProduct layer (Linear, Layer_Base.h:64-95) + ParamLayer (Layers.h:510-520), NAF::Train (Learners/NAF.cpp:133-178) in
//   fp64 with Continuous_policy (Math/Continuous_policy.h) and Quadratic_advantage (Math/Quadratic_term.h, Math/Quadratic_advantage.h):
//   outputs [V | l x nL | m x dA | sigma parameter x dA], write-backs MiniBatch::setMseDklImpw / setValues (MiniBatch.h:161-175) and the
//   backward of the output layer into the last hidden block.
//
// How the work is split.  ONE WORKGROUP of four wavefronts per minibatch row:
//   forward   the row's hidden activations go to LDS once; the OUTPUT COLUMNS sit on the lanes -- column o = lane + 64 s in register slot
//             s of lane `lane`, three slots hold the 1 + 153 + 17 = 171 dense outputs of dimA = 17 -- and each wavefront walks a quarter of
//             the hidden units, reading one weight row per unit as 64-lane coalesced loads.  The four partial sums of a column meet in LDS
//             and are added in wavefront order.
//   head      wavefront 0, fp64.  The dA x dA triangle L, P = L L^T and d = a - mu live in LDS; an entry (j, i) of the triangle -- an output
//             column -- or of P is one lane's work (entries lane + 64 s), P d and the triangular product of the gradient are row sums whose
//             terms are added in ascending index order by the lane that owns the entry.
//   backward  every thread owns hidden units tid + 256 q and adds W[k][o] delta[o] over the columns in ascending order (16-byte loads
//             along its weight row; the deltas are LDS broadcasts).
// No atomics and no order that depends on timing: results are bit-deterministic.
//
// stateValue[t+1] with returnsEstimator "none" is written by the step that samples t.  Where the same minibatch also samples t+1 of that
// episode (the sorted unique indices put it in the next row) that step's own setValues(t+1, V, Q) wins: the writer of t leaves
// stateValue[t+1] alone and only uses V_tgt in its target.  (The reference races there.)
#include <algorithm>
#include "dev_common.h"

namespace hl {

constexpr int NQ_MAXOUT = 192;                       // 171 dense outputs + 17 sigma parameters, rounded up to whole 64-lane slots
constexpr int NQ_LD = NAF_MAX_DIMA;                  // row pitch of the triangle and of P in LDS
constexpr int NQ_MAXH = 2048;                        // hidden width hl_create serves

__device__ __forceinline__ double nqSoftPlus(double x) { return (x + sqrt(1 + x * x)) / 2; }                 // SoftPlus::_eval (Functions.h:541-584)
__device__ __forceinline__ double nqSoftPlusD(double x) { return (1 + x / sqrt(1 + x * x)) / 2; }
__device__ __forceinline__ double nqHardSigm(double x) { return 0.5 * (1 + x / sqrt(1 + x * x)); }           // HardSigmoid::_eval (Functions.h:268-283)
__device__ __forceinline__ double nqHardSigmD(double x) { const double d = sqrt(1 + x * x); return 0.5 / (d * d * d); }
// entry e of the triangle in the outputs' order (row j outer, column i <= j inner)
__device__ __forceinline__ void nqEntry(int e, int& j, int& i) { j = 0; while ((j + 1) * (j + 2) / 2 <= e) ++j; i = e - j * (j + 1) / 2; }

template <int HQ>
__global__ __launch_bounds__(256) void headq_kernel(NafHeadArgs q) {
  const HeadArgs& a = q.h;
  __shared__ float sY[NQ_MAXH];
  __shared__ float sPart[4][NQ_MAXOUT];
  __shared__ float sXo[NQ_MAXOUT], sDelta[NQ_MAXOUT];
  __shared__ double sO[NQ_MAXOUT];
  __shared__ double sL[NQ_LD * NQ_LD], sP[NQ_LD * NQ_LD], sd[NQ_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = blockIdx.x;
  const DevScalars* sc = a.sc;
  if (row >= sc->nRows[a.parity]) return;
  const int B = a.B, dA = a.dA, nDense = a.nDense, H = a.H, nL = q.nL, pM = 1 + nL;
  const bool isNext = row >= B;
  if (isNext && q.retNone) return;            // (the next states of this estimator go through the target net: launch_naf_vtgt)
  const int b = isNext ? a.bt.nextSrc[row - B] : row;
  const long long slot = a.bt.slot[b];
  const float* Wo = a.params + a.indWo;

  // ---- every load a sample needs, in one round ----------------------------------------------------------------
  for (int k = tid; k < H; k += 256) sY[k] = a.Yin[(size_t)row * a.ldY + k];
  float xl[HQ], yl[HQ];
#pragma unroll
  for (int u = 0; u < HQ; ++u) {
    const int k = tid + 256 * u; const bool ok = k < H && !isNext;
    xl[u] = ok ? a.Xlast[(size_t)row * a.ldD + k] : 0.f;
    yl[u] = ok ? a.Ylast[(size_t)row * a.ldD + k] : 0.f;
  }
  if (tid < NQ_MAXOUT) sDelta[tid] = 0.f;
  double act = 0, bMean = 0, bStd = 1, rew = 0;
  float misc = 0.f, bp = 0.f;
  int eidv = 0, nxtv = -1, tv = 0, eidNext = -1, tNext = -1, epN = 0, epTerm = 0;
  double beta = 1, Cmax = 1, Cinv = 1; float rM = 0.f, rS = 1.f;
  if (wave == 0) {
    beta = sc->beta; Cmax = sc->Cmax; Cinv = sc->Cinv; rM = sc->rewMean; rS = sc->rewScale;
    if (lane < a.nSig) bp = a.params[a.indBp + lane];
    if (!isNext && lane < dA) {
      act = a.rp.A[(size_t)slot * dA + lane];
      bMean = a.rp.MU[(size_t)slot * 2 * dA + lane]; bStd = a.rp.MU[(size_t)slot * 2 * dA + dA + lane];
    }
    // lanes 0..5: RET, DQ, DKL, IMPW, V, ADV of the sampled step; lanes 6, 7: V, ADV of t+1
    const float* arr = lane == 6 ? a.rp.V : lane == 7 ? a.rp.ADV : nullptr; long long sl = slot + 1;
    if (!isNext && lane < 6) { arr = lane == 0 ? a.rp.RET : lane == 1 ? a.rp.DQ : lane == 2 ? a.rp.DKL : lane == 3 ? a.rp.IMPW : lane == 4 ? a.rp.V : a.rp.ADV; sl = slot; }
    if (arr) misc = arr[sl];
    if (!isNext && lane == 0) {
      eidv = a.bt.eid[b]; nxtv = a.bt.nextOf[b]; tv = a.bt.t[b]; rew = a.rp.R[slot];
      if (b + 1 < B) { eidNext = a.bt.eid[b + 1]; tNext = a.bt.t[b + 1]; }
      epN = a.rp.epN[eidv]; epTerm = a.rp.epTerm[eidv];
    }
  }
  __syncthreads();

  // ---- output dense layer: columns on the lanes, a quarter of the hidden units per wavefront -----------------
  const int cols = isNext ? 1 : nDense;
  {
    const int kq = (H + 3) / 4, k0 = wave * kq, k1 = min(H, k0 + kq);
    float p0 = 0.f, p1 = 0.f, p2 = 0.f;
    const bool c0 = lane < cols, c1 = lane + 64 < cols, c2 = lane + 128 < cols;
#pragma unroll 4
    for (int k = k0; k < k1; ++k) {
      const float y = sY[k]; const float* wr = Wo + (size_t)k * a.ldWo;
      if (c0) p0 = fmaf(y, wr[lane], p0);
      if (c1) p1 = fmaf(y, wr[lane + 64], p1);
      if (c2) p2 = fmaf(y, wr[lane + 128], p2);
    }
    sPart[wave][lane] = p0; sPart[wave][lane + 64] = p1; sPart[wave][lane + 128] = p2;
  }
  __syncthreads();
  if (wave == 0) {
    for (int o = lane; o < cols; o += 64) {      // the four quarter sums in wavefront order, then the bias
      const float x = ((sPart[0][o] + sPart[1][o]) + (sPart[2][o] + sPart[3][o])) + a.params[a.indBo + o];
      sXo[o] = x; sO[o] = (double)(a.outFunc == HL_FUNC_LINEAR ? x : actEval(a.outFunc, x));
    }
    if (lane < a.nSig) sO[nDense + lane] = (double)bp;      // ParamLayer, Linear
  }
  __syncthreads();
  if (isNext) {      // NAF.cpp:150-152: V_live(s_{t+1}) of a truncated episode end (estimators other than "none")
    if (wave != 0) return;
    const float oV = __shfl(misc, 6, 64), oA = __shfl(misc, 7, 64);
    if (lane == 0) {
      const float Vn = (float)sO[0];
      a.bt.oldNextV[b] = oV; a.bt.oldNextADV[b] = oA;
      a.rp.V[slot + 1] = Vn; a.rp.ADV[slot + 1] = 0.f; a.bt.nextV[b] = Vn;
      a.bt.O[(size_t)row * a.nOut] = sO[0];
    }
    return;
  }

  if (wave == 0) {
    // ---- policy: rho, D_KL, the far-policy rule (as head_body.h) ---------------------------------------------
    const double MAXM = 8.31776613503286;
    double lw = 0, kl = 0, mean = 0, stdev = 1, dPos = 0, dk = 0;
    bool bnd = false;
    if (lane < dA) {
      bnd = a.bounded[lane] != 0;
      mean = sO[pM + lane];
      const double pp = sO[nDense + lane], rt = sqrt(1 + pp * pp);
      stdev = (pp + rt) / 2; dPos = (1 + pp / rt) / 2;
      const double invStd = 1 / stdev, bInv = 1 / bStd;
      const double m = bnd ? (mean > MAXM ? MAXM : (mean < -MAXM ? -MAXM : mean)) : mean;
      const double u1 = (act - m) * invStd, u2 = (act - bMean) * bInv;
      const double qq = stdev * bInv, lq = log(qq);
      lw = (u2 * u2 - u1 * u1) / 2 - lq;
      const double dm = (mean - bMean) * bInv;
      kl = (qq * qq - 1 + dm * dm - 2 * lq) / 2;
      // the quadratic term's own mean (Quadratic_term.h:83-96) and d = a - mu
      dk = act - (bnd ? nqHardSigm(mean) : mean);
      sd[lane] = dk;
    }
    const double logW = waveSum(lw), DKL = waveSum(kl);
    const double RHO = exp(logW > 7 ? 7 : (logW < -7 ? -7 : logW));
    const float Wf = (float)RHO, Cf = (float)Cmax, iCf = (float)Cinv;
    const bool far = (Cf > 1.f) && (Wf > Cf || Wf < iCf);
    // ---- the triangle: entry e = lane + 64 s is output column 1 + e --------------------------------------------
    for (int x = lane; x < dA * NQ_LD; x += 64) sL[x] = 0;
    __builtin_amdgcn_wave_barrier(); __threadfence_block();
    for (int e = lane; e < nL; e += 64) { int j, i; nqEntry(e, j, i); const double l = sO[1 + e]; sL[j * NQ_LD + i] = i == j ? nqSoftPlus(l) : l; }
    __builtin_amdgcn_wave_barrier(); __threadfence_block();
    for (int x = lane; x < dA * dA; x += 64) {      // P = L L^T (Quadratic_term.h:98-110), k ascending
      const int j = x / dA, i = x - j * dA;
      double s = 0;
      for (int k = 0; k < dA; ++k) s += sL[j * NQ_LD + k] * sL[i * NQ_LD + k];
      sP[j * NQ_LD + i] = s;
    }
    __builtin_amdgcn_wave_barrier(); __threadfence_block();
    double rowQ = 0, Pd = 0;      // lane j: sum_i d_i P_ji d_j (quadMatMul's inner loop) and (P d)_j with the error's factor below
    if (lane < dA) for (int i = 0; i < dA; ++i) rowQ += sd[i] * sP[lane * NQ_LD + i] * dk;
    double quad = 0;
    for (int j = 0; j < dA; ++j) quad += __shfl(rowQ, j, 64);
    const double V = sO[0], Aval = -0.5 * quad, Qs = V + Aval;
    // ---- target -------------------------------------------------------------------------------------------------
    const int t0 = __shfl(tv, 0, 64), N0 = __shfl(epN, 0, 64), term0 = __shfl(epTerm, 0, 64);
    const bool nextTerminal = (t0 + 2 == N0) && term0 != 0;
    const bool nextSampled = __shfl(eidNext, 0, 64) == __shfl(eidv, 0, 64) && __shfl(tNext, 0, 64) == t0 + 1;
    double target; bool wroteNext = false; float Vnext = 0.f;
    if (q.retNone) {
      const double r = __shfl(rew, 0, 64);
      target = (double)(float)((r - (double)rM) * (double)rS);      // Episode::scaledReward, as the sweeps evaluate it (misc.hip)
      if (!nextTerminal && !far) {
        const double Vt = (double)q.vTgt[b];
        target += q.gamma * Vt; Vnext = (float)Vt; wroteNext = !nextSampled;
      }
    } else target = (double)__shfl(misc, 0, 64);
    const double err = far ? 0.0 : target - Qs;
    // ---- gradient (Quadratic_advantage.h:30-71) ---------------------------------------------------------------------
    for (int e = lane; e < nL; e += 64) {
      int j, i; nqEntry(e, j, i);
      double g = 0;
      for (int k = i; k < dA; ++k) g += (err * (-sd[k] * sd[j])) * sL[k * NQ_LD + i];
      if (i == j) g *= nqSoftPlusD(sO[1 + e]);
      sDelta[1 + e] = (float)g; a.bt.G[(size_t)b * a.nOut + 1 + e] = (double)(float)g;
    }
    if (lane < dA) {
      for (int i = 0; i < dA; ++i) Pd += err * sP[lane * NQ_LD + i] * sd[i];
      double gM = bnd ? Pd * nqHardSigmD(mean) : Pd;
      if (Cmax > 1 && beta < 1) gM = beta * gM + (1 - beta) * (-1 * ((mean - bMean) * (1 / (bStd * bStd))));      // KLDivGradient(mu, -1), mean part
      const double gS = dPos * (q.explNoise - stdev) / 2;      // fixExplorationGrad
      sDelta[pM + lane] = (float)gM;
      a.bt.gParam[(size_t)b * dA + lane] = (float)gS;
      a.bt.G[(size_t)b * a.nOut + pM + lane] = (double)(float)gM;
      a.bt.G[(size_t)b * a.nOut + nDense + lane] = (double)(float)gS;
    }
    {
      const float oDQ = __shfl(misc, 1, 64), oDKL = __shfl(misc, 2, 64), oW = __shfl(misc, 3, 64);
      const float oV = __shfl(misc, 4, 64), oADV = __shfl(misc, 5, 64), oNV = __shfl(misc, 6, 64), oNA = __shfl(misc, 7, 64);
      if (lane == 0) {
        sDelta[0] = (float)err; a.bt.G[(size_t)b * a.nOut] = (double)(float)err;
        a.bt.rho[b] = RHO; a.bt.dkl[b] = DKL; a.bt.far[b] = far ? 1 : 0;
        const float E = (float)err, D = (float)DKL, Wn = (float)RHO, Vf = (float)V, Qf = (float)Qs;
        a.bt.oldDQ[b] = oDQ; a.bt.oldDKL[b] = oDKL; a.bt.oldW[b] = oW; a.bt.oldV[b] = oV; a.bt.oldADV[b] = oADV;
        a.bt.newDQ[b] = E; a.bt.newDKL[b] = D; a.bt.newW[b] = Wn; a.bt.newV[b] = Vf; a.bt.newQ[b] = Qf;
        a.rp.DQ[slot] = E; a.rp.DKL[slot] = D; a.rp.IMPW[slot] = Wn; a.rp.V[slot] = Vf; a.rp.ADV[slot] = Qf - Vf;
        a.bt.dq[b] = (double)E;
        a.bt.pEid[b] = eidv;
        if (q.retNone) {      // setValues(t+1, V_tgt): the bookkeeping pass takes it as it takes a truncated next state's value
          a.bt.pNextOf[b] = wroteNext ? B : -1;
          if (wroteNext) { a.bt.oldNextV[b] = oNV; a.bt.oldNextADV[b] = oNA; a.bt.nextV[b] = Vnext; a.rp.V[slot + 1] = Vnext; a.rp.ADV[slot + 1] = 0.f; }
        } else a.bt.pNextOf[b] = nxtv;
      }
    }
    for (int o = lane; o < a.nOut; o += 64) a.bt.O[(size_t)row * a.nOut + o] = sO[o];
    __builtin_amdgcn_wave_barrier(); __threadfence_block();
    for (int o = lane; o < nDense; o += 64) {      // BaseLayer::backward: deltas *= f'(x, y)
      float dl = sDelta[o];
      if (a.outFunc != HL_FUNC_LINEAR) { dl *= actDiff(a.outFunc, sXo[o], (float)sO[o]); sDelta[o] = dl; }
      a.dOut[(size_t)b * a.ldDo + o] = dl;
    }
  }
  __syncthreads();
  // ---- back-propagation into the last hidden block: a thread per hidden unit, columns in ascending order -----------
#pragma unroll
  for (int u = 0; u < HQ; ++u) {
    const int k = tid + 256 * u;
    if (k >= H) continue;
    const float4* wr = reinterpret_cast<const float4*>(Wo + (size_t)k * a.ldWo);
    float acc = 0.f;
    for (int c = 0; 4 * c < nDense; ++c) {
      const float4 w = wr[c];
      acc += (w.x * sDelta[4 * c] + w.y * sDelta[4 * c + 1]) + (w.z * sDelta[4 * c + 2] + w.w * sDelta[4 * c + 3]);
    }
    a.Dres[(size_t)b * a.ldD + k] = acc;
    a.D[(size_t)b * a.ldD + k] = acc * actDiff(a.func, xl[u], yl[u]);
  }
}

hipError_t launch_head_naf(const NafHeadArgs& a, int maxRows, hipStream_t s) {
  if (a.h.dA > NAF_MAX_DIMA || a.h.nOut > NQ_MAXOUT || a.h.H > NQ_MAXH || (a.h.ldWo & 3)) return hipErrorInvalidValue;
  const dim3 grid(maxRows), block(256);
  const int HQ = (a.h.H + 255) / 256;
  if (HQ <= 1) hipLaunchKernelGGL((headq_kernel<1>), grid, block, 0, s, a);
  else if (HQ <= 2) hipLaunchKernelGGL((headq_kernel<2>), grid, block, 0, s, a);
  else if (HQ <= 4) hipLaunchKernelGGL((headq_kernel<4>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((headq_kernel<8>), grid, block, 0, s, a);
  return hipGetLastError();
}

// ---- the target path ------------------------------------------------------------------------------------------------
// rows 0 .. B-1 of X1: the standardised state t+1 of each sampled step (Episode::standardizedState), as the sampler's gather writes s_t
__global__ __launch_bounds__(256) void naf_next_gather_kernel(DevReplay rp, const long long* slot, float* X1, int ldX, int dS, int B) {
  const long long n = (long long)B * dS;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int b = (int)(e / dS), i = (int)(e - (long long)b * dS);
    X1[(size_t)b * ldX + i] = (rp.S[(size_t)(slot[b] + 1) * dS + i] - rp.stMean[i]) * rp.stScale[i];
  }
}
hipError_t launch_naf_next_gather(const DevReplay& rp, const long long* slot, float* X1, int ldX, int dS, int B, hipStream_t s) {
  const long long n = (long long)B * dS;
  hipLaunchKernelGGL(naf_next_gather_kernel, dim3((unsigned)std::min<long long>(1024, (n + 255) / 256)), dim3(256), 0, s, rp, slot, X1, ldX, dS, B);
  return hipGetLastError();
}
// output column 0 of the target net: a wavefront per row, hidden units strided over the lanes, the butterfly sum's fixed order
__global__ __launch_bounds__(256) void naf_vtgt_kernel(const float* Y, int ldY, int H, const float* Wo, int ldWo, const float* bo, int outFunc, float* vTgt, int B) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  float p = 0.f;
  for (int k = lane; k < H; k += 64) p = fmaf(Y[(size_t)row * ldY + k], Wo[(size_t)k * ldWo], p);
  p = waveSumF(p);
  if (lane == 0) { const float x = p + bo[0]; vTgt[row] = outFunc == HL_FUNC_LINEAR ? x : actEval(outFunc, x); }
}
hipError_t launch_naf_vtgt(const float* Y, int ldY, int H, const float* Wo, int ldWo, const float* bo, int outFunc, float* vTgt, int B, hipStream_t s) {
  hipLaunchKernelGGL(naf_vtgt_kernel, dim3((B + 3) / 4), dim3(256), 0, s, Y, ldY, H, Wo, ldWo, bo, outFunc, vTgt, B);
  return hipGetLastError();
}
// Adam (misc.hip: adam_kernel) and, behind it on the same element, the target weights' update (Network/Optimizer.cpp:162-177)
__global__ __launch_bounds__(256) void naf_adam_target_kernel(AdamArgs a, float* T, int mode, double alpha) {
  AdamCoef c; c.eta = a.sc->etaEff[a.parity]; c.lambda = a.lambda; c.fac = a.fac;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long long)gridDim.x * blockDim.x) {
    float w = a.W[i], m1 = a.M1[i], m2 = a.M2[i];
    adamStep(c, a.G[i], w, m1, m2);
    a.W[i] = w; a.M1[i] = m1; a.M2[i] = m2;
    if (mode == NAF_TGT_COPY) T[i] = w;
    else if (mode == NAF_TGT_POLYAK) { const float t = T[i]; T[i] = (float)((double)t + alpha * (double)(w - t)); }
  }
}
hipError_t launch_naf_adam_target(const AdamArgs& a, float* T, int mode, double alpha, hipStream_t s) {
  hipLaunchKernelGGL(naf_adam_target_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a, T, mode, alpha);
  return hipGetLastError();
}

}  // namespace hl
