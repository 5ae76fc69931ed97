// smarties_amd/csrc/dpgt.hip -- DPG learners (include/smarties_hip_dpg.h): the target chain of DPG::Train (Learners/DPG.cpp:21-83) as ONE
// launch, the DPG head, the gather of the critic's input rows and the optimiser launch over both nets.
//
//   mu~(s) from the target actor, Q~(s, mu~(s)) from the target critic -- Approximator::forward with sample id -1 selects the target
//   weights of the critic AND of the actor that feeds it (Approximator.h:143-159) -- on s_t and on s_{t+1}, and for s_t the gradient of
//   Q~ with respect to the critic's action inputs (oneStepBackProp({1}, bID, t, -1), Approximator.h:207-230): the deterministic policy
//   gradient.  No weight gradient is taken along this chain and none of its activations is needed afterwards, so none is written.
//
// dpg_target_kernel.  ONE WORKGROUP of four wavefronts owns 16 minibatch rows of one row set (blockIdx.y: 0 = s_t, 1 = s_{t+1}; the
// rows are gathered from the replay through the minibatch's slot table and standardised as naf_next_gather_kernel does):
//   forward   a layer's input tile [16][K] sits in LDS (two tiles of pitch ld = 4 mod 16 take turns as input and output).  Wavefront w
//             owns the 16-column tiles w, w + 4, .. of the layer, four of them at a time with their accumulators in registers, on
//             v_mfma_f32_16x16x4_f32; k ascends; the weights come by DIRECT LOADS (a column tile belongs to one wavefront: a trip
//             through LDS would buy no reuse), the B operand's (k, column) elements being four 64-byte runs of weight rows.  The
//             epilogue adds the bias, applies the activation and the parametric residual (Layers.h:340-362) and writes the tile for the
//             next layer; columns up to the next multiple of 16 are written as zeros, so every k loop may read whole groups of four.
//   actor     its output layer is one column tile; the mean under nnOutputFunc lands BEHIND THE STATE in the critic's input tile.
//   critic    the same layers on [s | mu~]; the single output column is a fixed-order reduction: lane (row, quarter) of wavefront 0 adds
//             the units k = quarter mod 4 in ascending order, the four quarters meet as (q0 + q1) + (q2 + q3).
//   backward  (s_t only) each critic layer's activation derivative f'(x, y) stays in LDS, [16][size + pad] per layer.  The output layer
//             is Linear, so dQ/dR_last = Wo; per layer delta = g f', g_prev = delta W^T (+ g w_res on the residual's columns) on the
//             MFMA with the weight tile [16 inputs][64 units] loaded along the weight rows (16 bytes per lane) and transposed on its
//             way through the wavefront's own LDS region, as phase C of dqn_head_kernel does.  The first layer is taken for its dimA
//             action rows alone.
// Partial tiles (rows beyond B, inputs, units) are zero-filled on the way in and predicated on the way out.  No atomics; every sum has a
// fixed order: the same inputs give the same bits.
//
// dpg_head_kernel.  A workgroup per sample, as headq.hip: the actor's dimA output columns and the critic's one from the live nets' last
// hidden blocks (partial sums of strided units, joined in ascending order), the head in fp64 on the lanes of wavefront 0 (rho, D_KL and
// the far-policy rule as head_body.h evaluates them), then both output layers' backward into the last hidden blocks.
#include <algorithm>
#include "dev_common.h"

namespace hl {

constexpr int DT_LDW = 68;      // pitch of a wavefront's transposing region [16][64 + 4]
typedef float dtF4 __attribute__((ext_vector_type(4)));

static inline int dtUp16(int n) { return (n + 15) / 16 * 16; }
__device__ __forceinline__ int dtUp16d(int n) { return (n + 15) & ~15; }

size_t dpg_target_lds(const DpgTargetArgs& a) {
  size_t fl = (size_t)2 * 16 * a.ld + (size_t)4 * 16 * DT_LDW;
  for (int j = 0; j < a.critic.nHidden; ++j) fl += (size_t)16 * (dtUp16(a.critic.L[j].size) + 4);
  return fl * sizeof(float);
}

// one dense layer for the 16 rows of the tile: sOut[r][cOff + c] = f(sum_k sIn[r][k] W[k][c] + b[c]) (+ residual); sDer: f'(x, y) or nullptr
__device__ __forceinline__ void dtForward(const float* __restrict__ W, const DpgLayer& L, int func, const float* sIn, float* sOut, int ld,
                                          float* sDer, int ldDer, int cOff, int wave, int li, int lg) {
  const int K = L.nIn, N = L.size, nT = (N + 15) >> 4, ldW = L.ldW;
  const float* __restrict__ Wl = W + L.indW;
  for (int t0 = wave; t0 < nT; t0 += 16) {
    dtF4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = dtF4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int k4 = 0; k4 < K; k4 += 4) {
      const int k = k4 + lg; const bool kin = k < K;
      const float av = sIn[(size_t)li * ld + k];      // (k < roundUp(K, 4) <= roundUp(K, 16): written, zeros beyond K)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c0 = 16 * (t0 + 4 * u);
        if (c0 < N) {      // (wavefront-uniform)
          const bool on = kin && c0 + li < N;
          const float bv = on ? Wl[(size_t)k * ldW + c0 + li] : 0.f;
          acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[u], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = 16 * (t0 + 4 * u) + li;
      if (16 * (t0 + 4 * u) >= N) continue;
      const bool on = c < N;
      const float b = on ? W[L.indB + c] : 0.f;
      const bool res = on && L.hasRes && c < L.resW;
      const float wr = res ? W[L.indWr + c] : 0.f, br = res ? W[L.indBr + c] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {      // result element i of a lane: (row 4 lg + i, column li) of its tile
        const int r = 4 * lg + i;
        const float x = acc[u][i] + b;
        float y = func == HL_FUNC_LINEAR ? x : actEval(func, x);
        if (sDer) sDer[(size_t)r * ldDer + c] = on ? (func == HL_FUNC_LINEAR ? 1.f : actDiff(func, x, y)) : 0.f;
        if (res) y += sIn[(size_t)r * ld + c] * wr + br;
        sOut[(size_t)r * ld + cOff + c] = on ? y : 0.f;
      }
    }
  }
}

// g_prev[r][m] = sum_n sDelta[r][n] W[rowOff + m][n] (+ sG[r][m] w_res[m], m < resW) for m < M; zeros up to the next multiple of 16
__device__ __forceinline__ void dtBackward(const float* __restrict__ Wl, int ldW, int rowOff, int M, int Nred, const float* sDelta, int ldDer,
                                           const float* sG, const float* __restrict__ wRes, int resW, float* sOut, int ld, float* sWave,
                                           int wave, int li, int lg) {
  const int mEnd = dtUp16d(M), nK = (Nred + 3) >> 2;
  for (int m0 = 16 * wave; m0 < mEnd; m0 += 64) {
    dtF4 d4{0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < Nred; n0 += 64) {
      // sWave belongs to this wavefront alone, so no __syncthreads: a wavefront's LDS operations complete in issue order on gfx950, the
      // wave barrier keeps the compiler from moving the stores across the reads, the fence makes it wait for them (as dqn_head_kernel, phase C)
      __builtin_amdgcn_wave_barrier(); __threadfence_block();      // (the chunk before this one has been read)
#pragma unroll
      for (int u = 0; u < 4; ++u) {      // lane -> (input lg + 4 u, units n0 + 4 li ..+3): 16-byte loads along the weight row
        const int m = m0 + lg + 4 * u, n = n0 + 4 * li;
        dtF4 w{0.f, 0.f, 0.f, 0.f};
        if (m < M && n < ldW) w = *reinterpret_cast<const dtF4*>(Wl + (size_t)(rowOff + m) * ldW + n);      // (ldW and the block's offset are multiples of 8)
        if (n + 0 >= Nred) w.x = 0.f;
        if (n + 1 >= Nred) w.y = 0.f;
        if (n + 2 >= Nred) w.z = 0.f;
        if (n + 3 >= Nred) w.w = 0.f;
        *reinterpret_cast<dtF4*>(sWave + (size_t)(lg + 4 * u) * DT_LDW + 4 * li) = w;
      }
      __builtin_amdgcn_wave_barrier(); __threadfence_block();
      const int ks = min(16, nK - n0 / 4);
      for (int s = 0; s < ks; ++s) {      // A = delta (row li, unit n0 + 4 s + lg); B = W^T (unit, input m0 + li)
        const float av = sDelta[(size_t)li * ldDer + n0 + 4 * s + lg];
        const float bv = sWave[(size_t)li * DT_LDW + 4 * s + lg];
        d4 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, d4, 0, 0, 0);
      }
    }
    const int m = m0 + li;
    const bool res = m < M && m < resW;
    const float wr = res ? wRes[m] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * lg + i;
      float v = d4[i];
      if (res) v += sG[(size_t)r * ld + m] * wr;
      sOut[(size_t)r * ld + m] = m < M ? v : 0.f;
    }
  }
}

__global__ __launch_bounds__(256) void dpg_target_kernel(DpgTargetArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smemDt[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int set = (int)blockIdx.y, row0 = (int)blockIdx.x * 16, B = a.B, dS = a.dS, dA = a.dA, ld = a.ld;
  if (row0 >= B) return;
  float* cur = reinterpret_cast<float*>(smemDt);
  float* nxt = cur + (size_t)16 * ld;
  float* sDer0 = nxt + (size_t)16 * ld;
  float* sW = sDer0;
  for (int j = 0; j < a.critic.nHidden; ++j) sW += (size_t)16 * (dtUp16d(a.critic.L[j].size) + 4);
  float* sWave = sW + (size_t)wave * 16 * DT_LDW;
  const int in16 = dtUp16d(dS), inC16 = dtUp16d(dS + dA);

  // the state rows of the tile, standardised (Episode::standardizedState); rows beyond B and columns beyond dS: zeros
  auto gather = [&](float* dst, int lo, int hi, int width) {      // columns [0, dS): the state; [lo, hi): left as they are; up to width: zeros
    for (int e = tid; e < 16 * width; e += 256) {
      const int r = e / width, c = e - r * width, row = row0 + r;
      if (c >= lo && c < hi) continue;
      float v = 0.f;
      if (row < B && c < dS) v = (a.rp.S[(size_t)(a.slot[row] + set) * dS + c] - a.rp.stMean[c]) * a.rp.stScale[c];
      dst[(size_t)r * ld + c] = v;
    }
  };
  gather(cur, 0, 0, in16);
  __syncthreads();
  // ---- the target actor ----
  for (int j = 0; j < a.actor.nHidden; ++j) {
    dtForward(a.Wa, a.actor.L[j], a.actor.func, cur, nxt, ld, nullptr, 0, 0, wave, li, lg);
    __syncthreads();
    float* t = cur; cur = nxt; nxt = t;
  }
  {   // output layer: the mean under nnOutputFunc, behind the state in the critic's input tile
    const DpgLayer& q = a.actor.L[a.actor.nHidden - 1];
    DpgLayer o{}; o.nIn = q.size; o.size = dA; o.ldW = a.actor.ldWo; o.indW = a.actor.indWo; o.indB = a.actor.indBo;
    dtForward(a.Wa, o, a.outFuncA, cur, nxt, ld, nullptr, 0, dS, wave, li, lg);      // (writes columns dS .. dS + 15 <= ld - 4)
    __syncthreads();
    gather(nxt, dS, dS + dA, inC16);
    __syncthreads();
    float* t = cur; cur = nxt; nxt = t;
  }
  // ---- the target critic ----
  {
    float* sDer = sDer0;
    for (int j = 0; j < a.critic.nHidden; ++j) {
      const int ldDer = dtUp16d(a.critic.L[j].size) + 4;
      dtForward(a.Wc, a.critic.L[j], a.critic.func, cur, nxt, ld, set == 0 ? sDer : nullptr, ldDer, 0, wave, li, lg);
      __syncthreads();
      float* t = cur; cur = nxt; nxt = t;
      sDer += (size_t)16 * ldDer;
    }
  }
  const DpgLayer& last = a.critic.L[a.critic.nHidden - 1];
  const int H = last.size;
  const float* __restrict__ Wo = a.Wc + a.critic.indWo; const int ldWo = a.critic.ldWo;
  if (wave == 0) {      // the one output column: lane (row li, quarter lg)
    float s = 0.f;
    for (int k = lg; k < H; k += 4) s = fmaf(cur[(size_t)li * ld + k], Wo[(size_t)k * ldWo], s);
    const float s0 = __shfl(s, li, 64), s1 = __shfl(s, li + 16, 64), s2 = __shfl(s, li + 32, 64), s3 = __shfl(s, li + 48, 64);
    const float qv = ((s0 + s1) + (s2 + s3)) + a.Wc[a.critic.indBo];
    if (lg == 0 && row0 + li < B) (set == 0 ? a.qT : a.qN)[row0 + li] = qv;
  }
  if (set != 0) return;

  // ---- backward through the target critic to the action inputs (s_t rows) ----
  __syncthreads();
  {   // dQ/dR_last = Wo (the output layer is Linear), the same for every row
    const int w16 = dtUp16d(H);
    for (int e = tid; e < 16 * w16; e += 256) { const int r = e / w16, c = e - r * w16; nxt[(size_t)r * ld + c] = c < H ? Wo[(size_t)c * ldWo] : 0.f; }
  }
  __syncthreads();
  { float* t = cur; cur = nxt; nxt = t; }
  for (int j = a.critic.nHidden - 1; j >= 0; --j) {
    const DpgLayer& L = a.critic.L[j];
    const int ldDer = dtUp16d(L.size) + 4;
    float* sDer = sDer0;
    for (int i = 0; i < j; ++i) sDer += (size_t)16 * (dtUp16d(a.critic.L[i].size) + 4);
    {   // delta = g f'(x, y), over the derivative in place
      const int w16 = dtUp16d(L.size);
      for (int e = tid; e < 16 * w16; e += 256) { const int r = e / w16, c = e - r * w16; sDer[(size_t)r * ldDer + c] *= cur[(size_t)r * ld + c]; }
    }
    __syncthreads();
    if (j > 0) dtBackward(a.Wc + L.indW, L.ldW, 0, L.nIn, L.size, sDer, ldDer, cur, a.Wc + L.indWr, L.hasRes ? L.resW : 0, nxt, ld, sWave, wave, li, lg);
    else dtBackward(a.Wc + L.indW, L.ldW, dS, dA, L.size, sDer, ldDer, cur, nullptr, 0, nxt, ld, sWave, wave, li, lg);      // the action rows of the first layer alone
    __syncthreads();
    float* t = cur; cur = nxt; nxt = t;
  }
  for (int e = tid; e < 16 * DPG_MAX_DIMA; e += 256) {
    const int r = e / DPG_MAX_DIMA, c = e - r * DPG_MAX_DIMA;
    if (row0 + r < B && c < dA) a.dQda[(size_t)(row0 + r) * DPG_MAX_DIMA + c] = cur[(size_t)r * ld + c];
  }
}

static bool dpgNetOk(const DpgNetDesc& n, int dIn) {
  if (n.nHidden < 1 || n.nHidden > HL_MAX_HIDDEN || (n.ldWo & 3) || (n.indWo & 3)) return false;
  int prev = dIn;
  for (int j = 0; j < n.nHidden; ++j) {
    const DpgLayer& L = n.L[j];
    if (L.nIn != prev || L.size < 1 || L.size > DPG_MAX_WIDTH || L.ldW < L.size || (L.ldW & 3) || (L.indW & 3) || (L.hasRes && L.resW > std::min(L.nIn, L.size))) return false;
    prev = L.size;
  }
  return true;
}
hipError_t launch_dpg_target(const DpgTargetArgs& a, hipStream_t s) {
  // what the kernel is written for: the tiles hold every layer's input and output, the mean's tile fits behind the state
  int need = std::max(a.dS + 16, a.dS + a.dA);
  for (int j = 0; j < a.actor.nHidden; ++j) need = std::max(need, a.actor.L[j].size);
  for (int j = 0; j < a.critic.nHidden; ++j) need = std::max(need, a.critic.L[j].size);
  if (a.B < 1 || a.dS < 1 || a.dS > 512 || a.dA < 1 || a.dA > DPG_MAX_DIMA || !dpgNetOk(a.actor, a.dS) || !dpgNetOk(a.critic, a.dS + a.dA) ||
      a.ld < dtUp16(need) + 4 || (a.ld & 3) || !a.qT || !a.qN || !a.dQda) return hipErrorInvalidValue;
  const size_t lds = dpg_target_lds(a);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  hipError_t e = ensureDynLds(reinterpret_cast<const void*>(&dpg_target_kernel), lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dpg_target_kernel, dim3((a.B + 15) / 16, 2), dim3(256), lds, s, a);
  return hipGetLastError();
}

// ---- the head ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dpg_head_kernel(DpgHeadArgs q) {
  const HeadArgs& a = q.h;
  __shared__ float sPart[16][DPG_MAX_DIMA + 1];
  __shared__ float sPartC[256];
  __shared__ float sXo[DPG_MAX_DIMA], sDelta[DPG_MAX_DIMA];
  __shared__ float sQ, sDc;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, B = a.B, dA = a.dA, H = a.H;
  if (b >= B) return;
  const DevScalars* sc = a.sc;
  const long long slot = a.bt.slot[b];
  const float* Wo = a.params + a.indWo;
  const float* cWo = q.cW + q.cIndWo;
  {   // output layers: the actor's columns (column tid % 16, units tid / 16 mod 16 ascending), the critic's one (units tid mod 256)
    const int c = tid & 15, p = tid >> 4;
    float s = 0.f;
    if (c < dA) for (int k = p; k < H; k += 16) s = fmaf(a.Yin[(size_t)b * a.ldY + k], Wo[(size_t)k * a.ldWo + c], s);
    sPart[p][c] = s;
    float sc1 = 0.f;
    for (int k = tid; k < q.cH; k += 256) sc1 = fmaf(q.cYin[(size_t)b * q.cLd + k], cWo[(size_t)k * q.cLdWo], sc1);
    sPartC[tid] = sc1;
  }
  __syncthreads();
  if (wave == 0) {
    if (lane < dA) { float x = 0.f; for (int p = 0; p < 16; ++p) x += sPart[p][lane]; sXo[lane] = x + a.params[a.indBo + lane]; }
    const float c4 = (sPartC[lane] + sPartC[lane + 64]) + (sPartC[lane + 128] + sPartC[lane + 192]);
    const float qv = waveSumF(c4) + q.cW[q.cIndBo];      // (the critic's output layer is Linear)
    // ---- policy: rho, D_KL, the far-policy rule (as head_body.h) ----
    const double beta = sc->beta, Cmax = sc->Cmax, Cinv = sc->Cinv;
    const double MAXM = 8.31776613503286;
    double lw = 0, kl = 0, mean = 0, stdev = 1, dPos = 0, bMean = 0, bStd = 1, pp = 0;
    float xo = 0.f;
    if (lane < dA) {
      const bool bnd = a.bounded[lane] != 0;
      const double act = a.rp.A[(size_t)slot * dA + lane];
      bMean = a.rp.MU[(size_t)slot * 2 * dA + lane]; bStd = a.rp.MU[(size_t)slot * 2 * dA + dA + lane];
      xo = sXo[lane];
      mean = (double)(a.outFunc == HL_FUNC_LINEAR ? xo : actEval(a.outFunc, xo));
      pp = (double)a.params[a.indBp + lane];      // ParamLayer, Linear
      const double rt = sqrt(1 + pp * pp);
      stdev = (pp + rt) / 2; dPos = (1 + pp / rt) / 2;      // SoftPlus and its derivative (Functions.h:541-584)
      const double invStd = 1 / stdev, bInv = 1 / bStd;
      const double m = bnd ? (mean > MAXM ? MAXM : (mean < -MAXM ? -MAXM : mean)) : mean;
      const double u1 = (act - m) * invStd, u2 = (act - bMean) * bInv;
      const double qq = stdev * bInv, lq = log(qq);
      lw = (u2 * u2 - u1 * u1) / 2 - lq;
      const double dm = (mean - bMean) * bInv;
      kl = (qq * qq - 1 + dm * dm - 2 * lq) / 2;
    }
    const double logW = waveSum(lw), DKL = waveSum(kl);
    const double RHO = exp(logW > 7 ? 7 : (logW < -7 ? -7 : logW));
    const float Wf = (float)RHO, Cf = (float)Cmax, iCf = (float)Cinv;
    const bool far = (Cf > 1.f) && (Wf > Cf || Wf < iCf);
    // ---- target (DPG.cpp:38-55, returnsEstimator "none") ----
    const int eidv = a.bt.eid[b], tv = a.bt.t[b];
    const bool nextSampled = b + 1 < B && a.bt.eid[b + 1] == eidv && a.bt.t[b + 1] == tv + 1;
    const bool nextTerminal = (tv + 2 == a.rp.epN[eidv]) && a.rp.epTerm[eidv] != 0;
    double target = (double)(float)((a.rp.R[slot] - (double)sc->rewMean) * (double)sc->rewScale);      // Episode::scaledReward, as the NAF head reads it
    bool wroteNext = false; float Vnext = 0.f;
    if (!nextTerminal && !far) { const double Qn = (double)q.qN[b]; target += q.gamma * Qn; Vnext = (float)Qn; wroteNext = !nextSampled; }
    const double qd = (double)qv, pd = (double)q.qT[b];
    const double err = target - qd, gC = far ? 0.0 : err;
    // ---- the actor's gradient: weightSum2Grads(polGrad, KLDivGradient(mu, -1), beta) through makeNetworkGrad ----
    if (lane < dA) {
      const double pol = far ? 0.0 : (double)q.dQda[(size_t)b * DPG_MAX_DIMA + lane];
      const double iv = 1 / (bStd * bStd);
      const double penM = -((mean - bMean) * iv);
      const double penS = -(dPos * ((iv - 1 / (stdev * stdev)) * stdev));
      const double fixS = dPos * (q.explNoise - stdev) / 2;      // fixExplorationGrad
      const double gM = beta * pol + (1 - beta) * penM, gS = beta * fixS + (1 - beta) * penS;
      float dl = (float)gM;
      a.bt.G[(size_t)b * a.nOut + lane] = (double)dl;
      a.bt.G[(size_t)b * a.nOut + dA + lane] = (double)(float)gS;
      a.bt.gParam[(size_t)b * dA + lane] = (float)gS;
      a.bt.O[(size_t)b * a.nOut + lane] = mean; a.bt.O[(size_t)b * a.nOut + dA + lane] = pp;
      if (a.outFunc != HL_FUNC_LINEAR) dl *= actDiff(a.outFunc, xo, (float)mean);      // BaseLayer::backward: deltas *= f'(x, y)
      sDelta[lane] = dl; a.dOut[(size_t)b * a.ldDo + lane] = dl;
    }
    if (lane == 0) {
      const float dc = (float)gC;
      sQ = qv; sDc = dc; q.cDOut[(size_t)b * q.cLdDo] = dc; q.cQ[b] = qd; q.cG[b] = (double)dc;
      a.bt.rho[b] = RHO; a.bt.dkl[b] = DKL; a.bt.far[b] = far ? 1 : 0;
      const float E = (float)err, D = (float)DKL, Wn = (float)RHO, Vf = (float)pd, Qf = (float)qd;      // setMseDklImpw; setValues(t, p, q)
      a.bt.oldDQ[b] = a.rp.DQ[slot]; a.bt.oldDKL[b] = a.rp.DKL[slot]; a.bt.oldW[b] = a.rp.IMPW[slot]; a.bt.oldV[b] = a.rp.V[slot]; a.bt.oldADV[b] = a.rp.ADV[slot];
      a.bt.newDQ[b] = E; a.bt.newDKL[b] = D; a.bt.newW[b] = Wn; a.bt.newV[b] = Vf; a.bt.newQ[b] = Qf;
      a.rp.DQ[slot] = E; a.rp.DKL[slot] = D; a.rp.IMPW[slot] = Wn; a.rp.V[slot] = Vf; a.rp.ADV[slot] = Qf - Vf;
      a.bt.dq[b] = (double)E;
      a.bt.pEid[b] = eidv;
      a.bt.pNextOf[b] = wroteNext ? B : -1;      // setValues(t + 1, Q~_next): the bookkeeping pass takes it as a truncated next state's value
      if (wroteNext) { a.bt.oldNextV[b] = a.rp.V[slot + 1]; a.bt.oldNextADV[b] = a.rp.ADV[slot + 1]; a.bt.nextV[b] = Vnext; a.rp.V[slot + 1] = Vnext; a.rp.ADV[slot + 1] = 0.f; }
    }
  }
  __syncthreads();
  // ---- back-propagation into the last hidden blocks: a thread per hidden unit, columns in ascending order ----
  for (int k = tid; k < H; k += 256) {
    float acc = 0.f;
    for (int c = 0; c < dA; ++c) acc += Wo[(size_t)k * a.ldWo + c] * sDelta[c];
    const size_t o = (size_t)b * a.ldD + k;
    a.Dres[o] = acc; a.D[o] = acc * actDiff(a.func, a.Xlast[o], a.Ylast[o]);
  }
  const float dc = sDc;
  for (int k = tid; k < q.cH; k += 256) {
    const float acc = cWo[(size_t)k * q.cLdWo] * dc;
    const size_t o = (size_t)b * q.cLd + k;
    q.cDres[o] = acc; q.cD[o] = acc * actDiff(q.cFunc, q.cX[o], q.cY[o]);
  }
}
hipError_t launch_head_dpg(const DpgHeadArgs& a, hipStream_t s) {
  if (a.h.dA < 1 || a.h.dA > DPG_MAX_DIMA || a.h.nDense != a.h.dA || a.h.nOut != 2 * a.h.dA || a.h.nSig != a.h.dA || a.h.ldDo < a.h.dA || a.h.ldY < a.h.H ||
      a.cLd < a.cH || a.cLdDo < 1 || !a.qT || !a.qN || !a.dQda) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dpg_head_kernel, dim3(a.h.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

// rows 0 .. B-1 of the critic's input: [standardised s_t (the sampler's row) | the stored action]
__global__ __launch_bounds__(256) void dpg_critic_gather_kernel(DevReplay rp, const long long* slot, const float* X0, int ldX0, float* Xc, int ldXc, int dS, int dA, int B) {
  const int w = dS + dA; const long long n = (long long)B * w;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int b = (int)(e / w), i = (int)(e - (long long)b * w);
    Xc[(size_t)b * ldXc + i] = i < dS ? X0[(size_t)b * ldX0 + i] : (float)rp.A[(size_t)slot[b] * dA + (i - dS)];
  }
}
hipError_t launch_dpg_critic_gather(const DevReplay& rp, const long long* slot, const float* X0, int ldX0, float* Xc, int ldXc, int dS, int dA, int B, hipStream_t s) {
  const long long n = (long long)B * (dS + dA);
  hipLaunchKernelGGL(dpg_critic_gather_kernel, dim3((unsigned)std::min<long long>(1024, (n + 255) / 256)), dim3(256), 0, s, rp, slot, X0, ldX0, Xc, ldXc, dS, dA, B);
  return hipGetLastError();
}

// Adam and the target update (naf_adam_target_kernel's element) over the actor's range, then the critic's: each with its own
// learning-rate factor and nnLambda
__global__ __launch_bounds__(256) void dpg_adam_target_kernel(DpgAdamArgs q) {
  const long long n = q.a[0].n + q.a[1].n;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) twoNetAdamElement(q, e);
}
hipError_t launch_dpg_adam_target(const DpgAdamArgs& a, hipStream_t s) {
  const long long n = a.a[0].n + a.a[1].n;
  hipLaunchKernelGGL(dpg_adam_target_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace hl
