// smarties_amd/csrc/headdq.hip -- DQN learners (include/smarties_hip_dqn.h): output layer, softmax-policy Q head with the double-Q target,
// and the backward of the output layer into the last hidden block, as ONE launch with the minibatch rows on the rows of fp32 MFMA tiles.
//
//   output InnerProduct layer (Layer_Base.h:64-95) of a net whose nOpt outputs are the Q values; DQN::Train (Learners/DQN.cpp:150-210) in
//   fp64 with Discrete_policy_t<Exp> (Math/Discrete_policy.h): rho, D_KL, the far-policy rule, the beta-mixed penalty KLDivGradient(mu, -1),
//   write-backs MiniBatch::setMseDklImpw / setValues (MiniBatch.h:161-175).
//
// head_wide_kernel (headw.hip) puts a wavefront on each sample, and every wavefront streams the whole output-weight block twice.  Here the
// work is split the other way: ONE WORKGROUP of four wavefronts owns a tile of 16 minibatch rows and all nOpt columns, so a weight tile is
// read once per 16 samples, and the Q rows stay in LDS between the product and the head:
//
//   A  products  Q = Y Wo + b on v_mfma_f32_16x16x4_f32 for up to three row sets: the live activations of the tile's rows; with
//                returnsEstimator "none" the live activations on s_{t+1}; with a target net also the target activations on s_{t+1} against
//                the target Wo.  Wavefront w owns the 16-column tiles w, w + 4, ..: NQ of them, accumulators in registers.  The hidden units
//                go in chunks of 64: the Y chunk of every row set is staged once in LDS for all wavefronts (pitch 68: the A operand's 64
//                lanes, (row li, k = 4 s + lg), hit 64 different banks).  The Wo chunk reaches the B operand by DIRECT LOADS: a column
//                tile belongs to one wavefront, so a trip through LDS would buy no reuse, and the operand's (k, column li) elements are
//                four full 64-byte runs of the weight rows.  Accumulation in ascending k.  The Q rows land in LDS as fp32
//                [row set][16][ldQ], ldQ = 64 NQ + 4: the MFMA result's (row 4 lg + i, column li) stores and the operand reads of phase C
//                then spread over all banks (ldQ = 4 mod 16); 3 x 16 x 516 x 4 = 99 KB at 512 options.
//   B  head      each wavefront takes four of the 16 rows in turn, option lane + 64 q in register slot q, fp64.  The delta row goes back to
//                LDS as fp32 over the live Q row.  Rows >= B (next rows of a truncated episode end, estimators other than "none") write
//                stateValue[t+1] alone.
//   C  backward  dY[16][H] = delta[16][nOpt] Wo^T on the MFMA: wavefront w owns the 16-unit tiles w, w + 4, .. of H; its Wo tile
//                [16 units][64 options] comes in as 16-byte loads along the weight rows and is transposed on its way through the wavefront's
//                own LDS region (the B operand reads (k = option, unit li) there); k ascends over the options.  The output layer's own
//                weight gradient stays with the dW launches, which read the deltas.
//
// ORDER OF EVERY SUM of the head (Z, D_KL, V, sum_j tau_j p_j, the target's sums): each lane adds its own options in ascending slot order
// q = 0, 1, .. from 0.0; the 64 lane sums go through waveSum (headw.hip documents the same order).  The label's terms are picked, not
// summed.  No atomics and no order that depends on timing: the same inputs give the same bits.
#include <algorithm>
#include "dev_common.h"

namespace hl {

constexpr int DQ_KC = 64, DQ_LDS_Y = DQ_KC + 4;      // hidden units (phase A) / options (phase C) per chunk; pitch of the staged chunk
typedef float dqF4 __attribute__((ext_vector_type(4)));

template <int NQ> constexpr int dqLdQ() { return 64 * NQ + 4; }
// floats of LDS: Q rows [nSets][16][ldQ] | staging: phase A [nSets][16][68], phase C [4 wavefronts][16][68]
static size_t dqnHeadLds(int NQ, int nSets) { return ((size_t)nSets * 16 * (64 * NQ + 4) + (size_t)4 * 16 * DQ_LDS_Y) * sizeof(float); }

__device__ __forceinline__ double dqSafeExp(double x) { return exp(fmin(8.0, fmax(-8.0, x))); }      // safeExp (Utils/FunctionUtilities.h), as nnSafeExp in fp64

template <int NQ>
__global__ __launch_bounds__(256) void dqn_head_kernel(DqnHeadArgs q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smemDq[];
  const HeadArgs& a = q.h;
  constexpr int LDQ = dqLdQ<NQ>();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const DevScalars* sc = a.sc;
  const int nRowsNow = sc->nRows[a.parity];
  const int B = a.B, nOpt = a.nOpt, nOut = a.nOut, H = a.H;
  const int row0 = (int)blockIdx.x * 16;
  // (a tile without work: behind the rows of this step, or -- "none" -- among the next rows, which that estimator takes from its own chains)
  if (row0 >= nRowsNow || (q.retNone && row0 >= B)) return;
  const int nSets = q.retNone ? (q.hasTgt ? 3 : 2) : 1;
  float* sQ = reinterpret_cast<float*>(smemDq);
  float* sStage = sQ + (size_t)nSets * 16 * LDQ;
  const float* __restrict__ Wo = a.params + a.indWo;
  const float* __restrict__ WoT = q.hasTgt ? q.tgtParams + a.indWo : Wo;
  const int ldWo = a.ldWo;

  // ---- phase A: Q = Y Wo + b, rows of the tile x all options, per row set --------------------------------------------------
  dqF4 acc[3][NQ];
#pragma unroll
  for (int t = 0; t < NQ; ++t) { acc[0][t] = dqF4{0.f, 0.f, 0.f, 0.f}; acc[1][t] = acc[0][t]; acc[2][t] = acc[0][t]; }
  for (int k0 = 0; k0 < H; k0 += DQ_KC) {
    __syncthreads();      // (the chunk before this one has been read)
    {   // stage: thread -> (row tid / 16, hidden units k0 + 4 (tid % 16) ..+3) of every row set; rows and units beyond the arrays: zeros
      const int r = tid >> 4, kk = (tid & 15) * 4, k = k0 + kk, row = row0 + r;
      for (int set = 0; set < nSets; ++set) {
        const float* Y = set == 0 ? a.Yin : (set == 1 ? q.Ynxt : q.Ytgt);
        // set 0: every row of this step (next rows included); sets 1, 2: the B rows of the next-state chains
        const bool rowOn = set == 0 ? (row < nRowsNow && !(q.retNone && row >= B)) : row < B;
        dqF4 v{0.f, 0.f, 0.f, 0.f};
        if (rowOn && k < a.ldY) v = *reinterpret_cast<const dqF4*>(Y + (size_t)row * a.ldY + k);      // (ldY is a multiple of 16: the four lie inside the row)
        if (k + 0 >= H) v.x = 0.f;
        if (k + 1 >= H) v.y = 0.f;
        if (k + 2 >= H) v.z = 0.f;
        if (k + 3 >= H) v.w = 0.f;
        *reinterpret_cast<dqF4*>(sStage + ((size_t)set * 16 + r) * DQ_LDS_Y + kk) = v;
      }
    }
    __syncthreads();
    const int ks = min(DQ_KC / 4, (H - k0 + 3) / 4);
#pragma unroll 2
    for (int s = 0; s < ks; ++s) {
      const int k = k0 + 4 * s + lg; const bool kin = k < H;
      const float a0 = sStage[(size_t)li * DQ_LDS_Y + 4 * s + lg];
      const float a1 = q.retNone ? sStage[((size_t)16 + li) * DQ_LDS_Y + 4 * s + lg] : 0.f;
      const float a2 = q.hasTgt ? sStage[((size_t)32 + li) * DQ_LDS_Y + 4 * s + lg] : 0.f;
#pragma unroll
      for (int t = 0; t < NQ; ++t) {
        const int c0 = 16 * (wave + 4 * t);
        if (c0 < nOpt) {      // (wavefront-uniform)
          const bool on = kin && c0 + li < nOpt;
          const size_t off = (size_t)(on ? k : 0) * ldWo + (on ? c0 + li : 0);
          const float b = on ? Wo[off] : 0.f;
          acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b, acc[0][t], 0, 0, 0);
          if (q.retNone) acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b, acc[1][t], 0, 0, 0);
          if (q.hasTgt) { const float bT = on ? WoT[off] : 0.f; acc[2][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, bT, acc[2][t], 0, 0, 0); }
        }
      }
    }
  }
  // the pre-activations x = (sum, k ascending) + b into LDS: result element i of a lane is (row 4 lg + i, column li) of its tile
#pragma unroll
  for (int t = 0; t < NQ; ++t) {
    const int c = 16 * (wave + 4 * t) + li;      // < 64 NQ
    const bool on = c < nOpt;
    const float bo = on ? a.params[a.indBo + c] : 0.f;
    const float bT = (on && q.hasTgt) ? q.tgtParams[a.indBo + c] : bo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * lg + i;
      sQ[(size_t)r * LDQ + c] = on ? acc[0][t][i] + bo : 0.f;
      if (q.retNone) sQ[((size_t)16 + r) * LDQ + c] = on ? acc[1][t][i] + bo : 0.f;
      if (q.hasTgt) sQ[((size_t)32 + r) * LDQ + c] = on ? acc[2][t][i] + bT : 0.f;
    }
  }
  __syncthreads();

  // ---- phase B: the head, four rows per wavefront ------------------------------------------------------------------------------
  const double beta = sc->beta, Cmax = sc->Cmax, Cinv = sc->Cinv;
  const double EPS = 2.220446049250313e-16;
  for (int j = 0; j < 4; ++j) {
    const int r = wave + 4 * j, row = row0 + r;
    if (row >= nRowsNow) continue;
    const bool isNext = row >= B;
    if (isNext && q.retNone) continue;
    float* sRow = sQ + (size_t)r * LDQ;
    const int b = isNext ? a.bt.nextSrc[row - B] : row;
    const long long slot = a.bt.slot[b];
    // BaseLayer::forward of the output layer: y = f(x), f = settings nnOutputFunc
    float xo[NQ]; double Q[NQ], un[NQ];
    double sZ = 0;
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
      const int c = lane + 64 * s; const bool on = c < nOpt;
      xo[s] = on ? sRow[c] : 0.f;
      Q[s] = on ? (double)(a.outFunc == HL_FUNC_LINEAR ? xo[s] : actEval(a.outFunc, xo[s])) : 0.0;
      un[s] = on ? dqSafeExp(Q[s]) : 0.0; sZ += un[s];
      if (on) a.bt.O[(size_t)row * nOut + c] = Q[s];
    }
    const double Z = fmax(waveSum(sZ), EPS);
    if (isNext) {   // DQN.cpp:164-169: V(s_{t+1}) = sum_i p_i Q_i of the live net at a truncated episode end
      double sV = 0;
#pragma unroll
      for (int s = 0; s < NQ; ++s) sV += (un[s] / Z) * Q[s];
      const double Vn = waveSum(sV);
      if (lane == 0) {
        const float Vf = (float)Vn;
        a.bt.oldNextV[b] = a.rp.V[slot + 1]; a.bt.oldNextADV[b] = a.rp.ADV[slot + 1];
        a.rp.V[slot + 1] = Vf; a.rp.ADV[slot + 1] = 0.f; a.bt.nextV[b] = Vf;
      }
      continue;
    }
    // the sample's replay row
    double act = 0, rew = 0; int eidv = 0, nxtv = -1, tv = 0, epN = 0, epTerm = 0;
    if (lane == 0) {
      act = discreteLabel(a, slot); eidv = a.bt.eid[b]; nxtv = a.bt.nextOf[b];
      if (q.retNone) { tv = a.bt.t[b]; rew = a.rp.R[slot]; epN = a.rp.epN[eidv]; epTerm = a.rp.epTerm[eidv]; }
    }
    float misc = 0.f;      // lanes 0..5: RET, DQ, DKL, IMPW, V, ADV of the sampled step
    {
      const float* arr = lane == 0 ? a.rp.RET : lane == 1 ? a.rp.DQ : lane == 2 ? a.rp.DKL : lane == 3 ? a.rp.IMPW : lane == 4 ? a.rp.V : lane == 5 ? a.rp.ADV : nullptr;
      if (arr) misc = arr[slot];
    }
    double mu[NQ];
#pragma unroll
    for (int s = 0; s < NQ; ++s) { const int c = lane + 64 * s; mu[s] = c < nOpt ? a.rp.MU[(size_t)slot * nOpt + c] : 1.0; }
    const int label = min(max((int)floor(__shfl(act, 0, 64)), 0), nOpt - 1);      // (a label beyond the options: the last one, never an index out of the arrays)
    const int labLane = label & 63, labQ = label >> 6;
    double lr[NQ];
    double sKl = 0, sV = 0, sTp = 0, pL = 0, mL = 1, qL = 0;
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
      const bool on = lane + 64 * s < nOpt;
      const double p = un[s] / Z;
      lr[s] = on ? log(p / mu[s]) : 0.0;
      sKl += on ? p * lr[s] : 0.0;                     // KLDivergence
      sV += p * Q[s];                                  // expectedValue(Qs, Qs)
      sTp += on ? (-(1 + lr[s]) / Z) * p : 0.0;        // KLDivGradient(mu, -1): sum_j tau_j p_j
      if (s == labQ) { pL = p; mL = mu[s]; qL = Q[s]; }
    }
    const double RHO = __shfl(pL, labLane, 64) / __shfl(mL, labLane, 64);      // importanceWeight, no clipping
    const double DKL = waveSum(sKl), V = waveSum(sV), tp = waveSum(sTp);
    const double Qa = __shfl(qL, labLane, 64);
    const float Wf = (float)RHO, Cf = (float)Cmax, iCf = (float)Cinv;
    const bool far = (Cf > 1.f) && (Wf > Cf || Wf < iCf);      // isFarPolicy, as head_body.h evaluates it
    // ---- target ----
    double target;
    if (q.retNone) {
      const int t0 = __shfl(tv, 0, 64), N0 = __shfl(epN, 0, 64), term0 = __shfl(epTerm, 0, 64);
      const bool nextTerminal = (t0 + 2 == N0) && term0 != 0;
      const double rr = __shfl(rew, 0, 64);
      target = (double)(float)((rr - (double)sc->rewMean) * (double)sc->rewScale);      // Episode::scaledReward, as the NAF head reads it
      if (!nextTerminal) {   // double Q (DQN.cpp:176-182): the live net's policy on s_{t+1} evaluates the target net's Q values
        const float* sHat = sQ + ((size_t)16 + r) * LDQ;
        const float* sTil = q.hasTgt ? sQ + ((size_t)32 + r) * LDQ : sHat;
        double uh[NQ], qt[NQ], sZh = 0, sE = 0;
#pragma unroll
        for (int s = 0; s < NQ; ++s) {
          const int c = lane + 64 * s; const bool on = c < nOpt;
          const float xh = on ? sHat[c] : 0.f, xt = on ? sTil[c] : 0.f;
          const double qh = (double)(a.outFunc == HL_FUNC_LINEAR ? xh : actEval(a.outFunc, xh));
          qt[s] = on ? (double)(a.outFunc == HL_FUNC_LINEAR ? xt : actEval(a.outFunc, xt)) : 0.0;
          uh[s] = on ? dqSafeExp(qh) : 0.0; sZh += uh[s];
        }
        const double Zh = fmax(waveSum(sZh), EPS);
#pragma unroll
        for (int s = 0; s < NQ; ++s) sE += (uh[s] / Zh) * qt[s];
        target += q.gamma * waveSum(sE);
      }
    } else target = (double)__shfl(misc, 0, 64);
    const double err = target - Qa;
    // ---- gradient: e on the label, refer's clipping and penalty; then BaseLayer::backward's f'(x, y) ----
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
      const int c = lane + 64 * s;
      float dl = 0.f;
      if (c < nOpt) {
        double g = c == label ? err : 0.0;
        if (Cmax > 1) {
          if (far) g = 0.0;
          const double pen = un[s] * (-(1 + lr[s]) / Z - tp);      // _evalDiff = u_i
          g = beta * g + (1 - beta) * pen;
        }
        dl = (float)g;
        a.bt.G[(size_t)b * nOut + c] = (double)dl;
        if (a.outFunc != HL_FUNC_LINEAR) dl *= actDiff(a.outFunc, xo[s], (float)Q[s]);
        a.dOut[(size_t)b * a.ldDo + c] = dl;
      }
      sRow[c] = dl;      // (c < 64 NQ < ldQ: zeros beyond the options, phase C reads whole groups of four)
    }
    {
      const float oDQ = __shfl(misc, 1, 64), oDKL = __shfl(misc, 2, 64), oW = __shfl(misc, 3, 64);
      const float oV = __shfl(misc, 4, 64), oADV = __shfl(misc, 5, 64);
      if (lane == 0) {
        a.bt.rho[b] = RHO; a.bt.dkl[b] = DKL; a.bt.far[b] = far ? 1 : 0;
        a.bt.pEid[b] = eidv; a.bt.pNextOf[b] = q.retNone ? -1 : nxtv;      // ("none": nothing is written to stateValue[t+1])
        const float E = (float)err, D = (float)DKL, Wn = (float)RHO, Vf = (float)V, Qf = (float)Qa;
        a.bt.oldDQ[b] = oDQ; a.bt.oldDKL[b] = oDKL; a.bt.oldW[b] = oW; a.bt.oldV[b] = oV; a.bt.oldADV[b] = oADV;
        a.bt.newDQ[b] = E; a.bt.newDKL[b] = D; a.bt.newW[b] = Wn; a.bt.newV[b] = Vf; a.bt.newQ[b] = Qf;
        a.rp.DQ[slot] = E; a.rp.DKL[slot] = D; a.rp.IMPW[slot] = Wn; a.rp.V[slot] = Vf; a.rp.ADV[slot] = Qf - Vf;
        a.bt.dq[b] = (double)E;
      }
    }
  }
  __syncthreads();
  if (row0 >= B) return;      // (next rows only: no gradient)

  // ---- phase C: dY = delta Wo^T, the wavefront's tiles of 16 hidden units ---------------------------------------------------
  float* sW = sStage + (size_t)wave * 16 * DQ_LDS_Y;      // [16 units][68]: the wavefront's own region
  const int nK = (nOpt + 3) / 4;      // groups of four options
  for (int n0 = 16 * wave; n0 < H; n0 += 64) {
    dqF4 d4{0.f, 0.f, 0.f, 0.f};
    for (int o0 = 0; o0 < nOpt; o0 += DQ_KC) {
      __builtin_amdgcn_wave_barrier(); __threadfence_block();      // (the chunk before this one has been read)
#pragma unroll
      for (int u = 0; u < 4; ++u) {      // lane -> (unit lg + 4 u, options o0 + 4 li ..+3): 16-byte loads along the weight row
        const int n = n0 + lg + 4 * u, o = o0 + 4 * li;
        dqF4 w{0.f, 0.f, 0.f, 0.f};
        if (n < H && o < ldWo) w = *reinterpret_cast<const dqF4*>(Wo + (size_t)n * ldWo + o);      // (ldWo is a multiple of 4)
        if (o + 0 >= nOpt) w.x = 0.f;
        if (o + 1 >= nOpt) w.y = 0.f;
        if (o + 2 >= nOpt) w.z = 0.f;
        if (o + 3 >= nOpt) w.w = 0.f;
        *reinterpret_cast<dqF4*>(sW + (size_t)(lg + 4 * u) * DQ_LDS_Y + 4 * li) = w;
      }
      __builtin_amdgcn_wave_barrier(); __threadfence_block();
      const int ks = min(DQ_KC / 4, nK - o0 / 4);
      for (int s = 0; s < ks; ++s) {      // A = delta (row li, option o0 + 4 s + lg); B = Wo^T (option, unit n0 + li)
        const float av = sQ[(size_t)li * LDQ + o0 + 4 * s + lg];
        const float bv = sW[(size_t)li * DQ_LDS_Y + 4 * s + lg];
        d4 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, d4, 0, 0, 0);
      }
    }
    const int k = n0 + li;
    if (k < H) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = row0 + 4 * lg + i;      // (sample rows: b = row)
        if (row < B) {
          const float g = d4[i];
          a.Dres[(size_t)row * a.ldD + k] = g;
          a.D[(size_t)row * a.ldD + k] = g * actDiff(a.func, a.Xlast[(size_t)row * a.ldD + k], a.Ylast[(size_t)row * a.ldD + k]);
        }
      }
    }
  }
}

template <int NQ> static hipError_t dqnHeadLaunch(const DqnHeadArgs& a, int maxRows, hipStream_t s) {
  const size_t lds = dqnHeadLds(NQ, a.retNone ? (a.hasTgt ? 3 : 2) : 1);
  hipError_t e = ensureDynLds(reinterpret_cast<const void*>(&dqn_head_kernel<NQ>), lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((dqn_head_kernel<NQ>), dim3((maxRows + 15) / 16), dim3(256), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_head_dqn(const DqnHeadArgs& a, int maxRows, hipStream_t s) {
  const HeadArgs& h = a.h;
  // what the kernel is written for: nOpt outputs and nothing else, 16-byte loads along the activation and the weight rows, a target
  // net only where its rows exist
  if (h.nOpt < 2 || h.nOpt > DISC_MAX_OPT || h.nDense != h.nOpt || h.nOut != h.nOpt || h.nSig != 0 || h.deferBeta || h.H < 1 || h.H > 2048 ||
      h.ldWo < h.nOpt || (h.ldWo & 3) || (h.indWo & 3) || h.ldDo < h.nOpt || (h.ldY & 3) || h.ldY < h.H || h.ldD < h.H ||
      (a.hasTgt && !a.retNone) || (a.retNone && !a.Ynxt) || (a.hasTgt && (!a.Ytgt || !a.tgtParams))) return hipErrorInvalidValue;
  if (h.nOpt <= 64) return dqnHeadLaunch<1>(a, maxRows, s);
  if (h.nOpt <= 128) return dqnHeadLaunch<2>(a, maxRows, s);
  if (h.nOpt <= 256) return dqnHeadLaunch<4>(a, maxRows, s);
  return dqnHeadLaunch<8>(a, maxRows, s);
}

}  // namespace hl
