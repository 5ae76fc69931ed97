// smarties_amd/csrc/headw.hip -- the head launch for discrete actions of 65 .. 512 options (include/smarties_hip_discrete.h).
//
//   output InnerProduct layer (Layer_Base.h:64-95), RACER::Train (Learners/RACER_train.cpp:14-67) in fp64 with Discrete_policy
//   (Math/Discrete_policy.h:17-208) and Discrete_advantage (Math/Discrete_advantage.h:17-100), the write-backs and the backward of the
//   output layer into the last hidden block: head_body.h:181-219 and its tail, for outputs [V | A x nOpt | logits x nOpt] of up to
//   1 + 2 x 512 = 1025 columns.
//
// head_kernel_t puts one option on each lane of the sample's wavefront and the hidden units of the output layer on the lanes as well,
// eight output columns per wave reduction: 129 rounds of eight reductions at 1025 columns.  Here the work is split the other way round:
//
//   * one wavefront per sample as there, four samples per workgroup, so every reduction of the head stays a wave reduction and nothing
//     crosses a barrier;
//   * output layer: the lanes own the output COLUMNS, column lane + 64 j in accumulator j (NT = 2 NQ + 1 tiles), and walk the hidden
//     units k in ascending order -- row k of the weights is read 64 consecutive floats per tile, the activation y[k] is a broadcast
//     read of the sample's row in LDS, no cross-lane step at all: O[o] = (sum_k y[k] W[k][o], k ascending, fused multiply-adds) + b[o];
//   * head: option lane + 64 q in slot q of the lane, NQ = 2 / 4 / 8 slots (up to 128 / 256 / 512 options); logit, advantage, behaviour
//     probability, unnormalised and normalised probability and log(p / mu) of a slot stay in registers; the outputs and the staged deltas
//     pass through LDS per wavefront (the column owner of the output layer is not the option owner of the head);
//   * backward of the output layer: deltas of the lane's columns in registers, hidden unit k's gradient = sum over the lane's tiles in
//     ascending order, then one wave reduction, four units in flight.
//
// ORDER OF EVERY SUM of the head (norm, DKL, E[A], sum_j tmp_j p_j): each lane adds its own options in ascending tile order q = 0, 1, ..,
// starting from 0.0; the 64 lane sums then go through waveSum (dev_common.h: the xor butterfly 32, 16, .., 1).  Against a sum in option
// order that moves an fp64 sum of n non-negative terms by at most ~ (NQ + 6) x 2^-53 relative to the sum of their magnitudes; the
// tolerance of tests/test_discrete_wide.py follows from this.  The label's own terms (p, mu, A of the label) are picked, not summed.
#include <algorithm>
#include "head_body.h"

namespace hl {

// floats of LDS per wavefront: outputs fp64 [LDO] | deltas [LDO] | pre-activations [LDO] | hidden activations [ldH]
template <int NQ> constexpr int headWideLdo() { return 128 * NQ + 8; }
static size_t headWideLds(int NQ, int H) {
  const size_t perWave = (size_t)(128 * NQ + 8) * 16 + (size_t)((H + 63) & ~63) * 4;
  return std::max((size_t)TAIL_LDS_BYTES, 4 * perWave);
}

template <int NQ>
__global__ __launch_bounds__(256) void head_wide_kernel(HeadArgs a, ExtraArgs extra) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smemW[];
  // horizontal fusion as head_kernel_t: workgroup 0 runs the sampler phase of the next step, the workgroups behind it its gather
  const int nExtra = extra.role ? 1 + extra.helpers : 0;
  if (extra.role && blockIdx.x == 0) { runExtra(extra, smemW); return; }
  if ((int)blockIdx.x < nExtra) { gatherHelper(extra.samp, blockIdx.x - 1, extra.helpers, smemW); return; }
  constexpr int NT = 2 * NQ + 1, LDO = headWideLdo<NQ>();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = (int)(blockIdx.x - nExtra) * 4 + wave;
  const int H = a.H, ldH = (H + 63) & ~63;
  unsigned char* mine = smemW + (size_t)wave * ((size_t)LDO * 16 + (size_t)ldH * 4);
  double* sO = reinterpret_cast<double*>(mine);
  float* sDelta = reinterpret_cast<float*>(mine + (size_t)LDO * 8);
  float* sXo = sDelta + LDO;
  float* sY = sXo + LDO;
  const DevScalars* sc = a.sc;
  const int nRowsNow = sc->nRows[a.parity];
  long long slotEarly = 0;
  if (row < a.B) slotEarly = a.bt.slot[row];
  if (row >= nRowsNow) return;
  const int B = a.B, nDense = a.nDense, nOpt = a.nOpt, nOut = a.nOut, pA = 1, pP = 1 + nOpt;
  const bool isNext = row >= B;
  const int b = isNext ? a.bt.nextSrc[row - B] : row;
  const long long slot = isNext ? a.bt.slot[b] : slotEarly;
  const float* __restrict__ Wo = a.params + a.indWo;
  const int ldWo = a.ldWo;

  if (isNext) {   // RACER_train.cpp:23-27: V(s_{t+1}) of a truncated episode end -- column 0 alone, the hidden units over the lanes
    float p = 0.f;
    for (int k = lane; k < H; k += 64) p = fmaf(a.Yin[(size_t)row * a.ldY + k], Wo[(size_t)k * ldWo], p);
    p = waveSumF(p);
    if (lane == 0) {
      const float x = p + a.params[a.indBo];
      const double O0 = (double)(a.outFunc == HL_FUNC_LINEAR ? x : actEval(a.outFunc, x));
      const float Vn = (float)scaleNet2V(O0);
      a.bt.oldNextV[b] = a.rp.V[slot + 1]; a.bt.oldNextADV[b] = a.rp.ADV[slot + 1];
      a.rp.V[slot + 1] = Vn; a.rp.ADV[slot + 1] = 0.f; a.bt.nextV[b] = Vn;
      a.bt.O[(size_t)row * nOut] = O0;
    }
    return;
  }

  // ---- the sample's replay row, requested in front of the output layer ---------------------------------------------------
  int eidv = 0, nxtv = 0;
  if (lane == 0) { eidv = a.bt.eid[b]; nxtv = a.bt.nextOf[b]; }
  const double beta = sc->beta, Cmax = sc->Cmax, Cinv = sc->Cinv;
  double act = 0;
  if (lane == 0) act = discreteLabel(a, slot);
  double mu[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) { const int c = lane + 64 * q; mu[q] = c < nOpt ? a.rp.MU[(size_t)slot * nOpt + c] : 1.0; }
  float misc = 0.f;      // lanes 0..5: RET, DQ, DKL, IMPW, V, ADV of the sampled step
  {
    const float* arr = lane == 0 ? a.rp.RET : lane == 1 ? a.rp.DQ : lane == 2 ? a.rp.DKL : lane == 3 ? a.rp.IMPW : lane == 4 ? a.rp.V : lane == 5 ? a.rp.ADV : nullptr;
    if (arr) misc = arr[slot];
  }

  // ---- output layer: columns over the lanes, hidden units in ascending order ---------------------------------------------
  for (int k = lane; k < ldH; k += 64) sY[k] = k < H ? a.Yin[(size_t)row * a.ldY + k] : 0.f;
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
  // (the column predicates lane + 64 j < nDense are compared where they are used: 17 lane masks held across the kernel cost 34 scalar registers)
  float acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = 0.f;
#pragma unroll 4
  for (int k = 0; k < H; ++k) {
    const float y = sY[k];
    const float* __restrict__ wr = Wo + (size_t)k * ldWo + lane;
#pragma unroll
    for (int j = 0; j < NT; ++j) if (lane + 64 * j < nDense) acc[j] = fmaf(y, wr[64 * j], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) if (lane + 64 * j < nDense) {      // BaseLayer::forward of the output layer: y = f(x), f = settings nnOutputFunc (Approximator.cpp:228)
    const int o = lane + 64 * j;
    const float x = acc[j] + a.params[a.indBo + o];
    const double v = (double)(a.outFunc == HL_FUNC_LINEAR ? x : actEval(a.outFunc, x));
    sXo[o] = x; sO[o] = v; a.bt.O[(size_t)row * nOut + o] = v;
  }
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();

  // ---- head: Discrete_policy + Discrete_advantage, option lane + 64 q in slot q; two passes ---------------------------------
  auto sp = [](double x) { return (x + sqrt(1 + x * x)) / 2; };
  auto spD = [](double x) { return (1 + x / sqrt(1 + x * x)) / 2; };
  const int label = min(max((int)floor(__shfl(act, 0, 64)), 0), nOpt - 1);      // (a label beyond the options: the last one, never an index out of the arrays)
  const int labLane = label & 63, labQ = label >> 6;
  double logit[NQ], advJ[NQ], un[NQ], pj[NQ], lr[NQ];
  double sNorm = 0;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {      // pass 1: the normalisation
    const int c = lane + 64 * q; const bool on = c < nOpt;
    logit[q] = on ? sO[pP + c] : 0.0; advJ[q] = on ? sO[pA + c] : 0.0;
    un[q] = on ? sp(logit[q]) : 0.0; sNorm += un[q];
  }
  const double norm = fmax(waveSum(sNorm), 2.220446049250313e-16);
  double sKl = 0, sEa = 0, sTp = 0, pL = 0, mL = 1, aL = 0;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {      // pass 2: probabilities, KL divergence, expected advantage, sum_j tmp_j p_j
    const bool on = lane + 64 * q < nOpt;
    pj[q] = un[q] / norm;
    lr[q] = on ? log(pj[q] / mu[q]) : 0.0;
    sKl += on ? pj[q] * lr[q] : 0.0;                     // KLDivergence (:126-130)
    sEa += on ? pj[q] * advJ[q] : 0.0;
    sTp += on ? (-(1 + lr[q]) / norm) * pj[q] : 0.0;     // KLDivGradient(mu, -1) (:152-162): sum_j tmp_j ((i == j) - p_j) = tmp_i - sum_j tmp_j p_j
    if (q == labQ) { pL = pj[q]; mL = mu[q]; aL = advJ[q]; }
  }
  const double RHO = __shfl(pL, labLane, 64) / __shfl(mL, labLane, 64);      // importanceWeight (:84-91), no clipping
  const double DKL = waveSum(sKl);
  const float Wf = (float)RHO, Cf = (float)Cmax, iCf = (float)Cinv;
  const bool far = (Cf > 1.f) && (Wf > Cf || Wf < iCf);
  const double expA = waveSum(sEa);
  const double Aval = __shfl(aL, labLane, 64) - expA;                         // computeAdvantage (:64-70)
  const double O0 = sO[0], V = scaleNet2V(O0);
  const double Qret = (double)__shfl(misc, 0, 64);
  const double A_RET = Qret - V, dQ = A_RET - Aval;
  const double g0 = far ? 0.0 : fmin(1.0, RHO) * dQ * beta * scaleVdiff(O0);
  const double Qer = far ? 0.0 : beta * (fmin(Cmax, RHO) * dQ);
  const double tp = waveSum(sTp);
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int c = lane + 64 * q;
    if (c < nOpt) {
      const double tmp = -(1 + lr[q]) / norm;
      const double dpos = spD(logit[q]);
      const double penal = (tmp - tp) * dpos;
      double pol = 0;
      if (!far) { const double factor = A_RET * fmin(Cmax, RHO); pol = ((c == label ? factor / un[q] : 0.0) - factor / norm) * dpos; }   // policyGradient (:136-144)
      const double gP = beta * pol + (1 - beta) * penal;                    // penalizeReFER + makeNetworkGrad
      const double gA = Qer * ((c == label ? 1.0 : 0.0) - pj[q]);           // Discrete_advantage::grad (:51-58)
      sDelta[pP + c] = (float)gP; sDelta[pA + c] = (float)gA;
      a.bt.G[(size_t)b * nOut + pP + c] = (double)(float)gP;
      a.bt.G[(size_t)b * nOut + pA + c] = (double)(float)gA;
    }
  }
  {   // the write-back tail of head_body.h
    const float oDQ = __shfl(misc, 1, 64), oDKL = __shfl(misc, 2, 64), oW = __shfl(misc, 3, 64);
    const float oV = __shfl(misc, 4, 64), oADV = __shfl(misc, 5, 64);
    if (lane == 0) {
      sDelta[0] = (float)g0;
      a.bt.G[(size_t)b * nOut] = (double)(float)g0;
      a.bt.rho[b] = RHO; a.bt.dkl[b] = DKL; a.bt.far[b] = far ? 1 : 0;
      a.bt.pEid[b] = eidv; a.bt.pNextOf[b] = nxtv;      // the (episode, next-row) map of THIS minibatch for the bookkeeping pass
      // write-backs (Fval casts, MiniBatch.h:161-175); old values kept for the aggregate updates
      const float E = (float)dQ, D = (float)DKL, Wn = (float)RHO, Vf = (float)V;
      a.bt.oldDQ[b] = oDQ; a.bt.oldDKL[b] = oDKL; a.bt.oldW[b] = oW; a.bt.oldV[b] = oV; a.bt.oldADV[b] = oADV;
      a.bt.newDQ[b] = E; a.bt.newDKL[b] = D; a.bt.newW[b] = Wn; a.bt.newV[b] = Vf;
      const float Qf = (float)(Aval + V);                     // Episode::updateValues_atomic(t, V, Q): advantage = Q - V in Fval
      a.rp.DQ[slot] = E; a.rp.DKL[slot] = D; a.rp.IMPW[slot] = Wn; a.rp.V[slot] = Vf; a.rp.ADV[slot] = Qf - Vf;
      a.bt.newQ[b] = Qf;
      a.bt.dq[b] = (double)E;
    }
  }
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();

  // ---- deltas of the output layer (BaseLayer::backward: deltas *= f'(x, y), Layer_Base.h:104-109) back into the column owners' registers,
  // then the gradient of the last hidden block: unit k = sum over the lane's tiles in ascending order, one wave reduction --------------
  float d[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int o = lane + 64 * j;
    d[j] = 0.f;
    if (lane + 64 * j < nDense) {
      d[j] = sDelta[o];
      if (a.outFunc != HL_FUNC_LINEAR) d[j] *= actDiff(a.outFunc, sXo[o], (float)sO[o]);
      a.dOut[(size_t)b * a.ldDo + o] = d[j];
    }
  }
  for (int k0 = 0; k0 < H; k0 += 64) {
    float keep = 0.f;
    const int kEnd = min(64, H - k0);
    for (int kk = 0; kk < kEnd; kk += 4) {
      float s[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = k0 + kk + u;
        const float* __restrict__ wr = Wo + (size_t)(k < H ? k : 0) * ldWo + lane;      // (a unit beyond the layer: row 0, its sum is dropped)
        s[u] = 0.f;
#pragma unroll
        for (int j = 0; j < NT; ++j) if (lane + 64 * j < nDense) s[u] = fmaf(wr[64 * j], d[j], s[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) { s[u] = waveSumF(s[u]); if (lane == kk + u) keep = s[u]; }
    }
    const int k = k0 + lane;
    if (k < H) {
      a.Dres[(size_t)b * a.ldD + k] = keep;
      a.D[(size_t)b * a.ldD + k] = keep * actDiff(a.func, a.Xlast[(size_t)row * a.ldD + k], a.Ylast[(size_t)row * a.ldD + k]);
    }
  }
}

template <int NQ> static hipError_t headWideLaunch(const HeadArgs& a, int maxRows, const ExtraArgs& ex, hipStream_t s) {
  const int nEx = ex.role ? 1 + ex.helpers : 0;
  const size_t lds = headWideLds(NQ, a.H);
  hipError_t e = ensureDynLds(reinterpret_cast<const void*>(&head_wide_kernel<NQ>), lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((head_wide_kernel<NQ>), dim3((maxRows + 3) / 4 + nEx), dim3(256), lds, s, a, ex);
  return hipGetLastError();
}

hipError_t launch_head_wide(const HeadArgs& a, int maxRows, const ExtraArgs* extra, hipStream_t s) {
  ExtraArgs ex{}; if (extra) ex = *extra;
  // what the kernel is written for: the discrete head's layout, its own beta (no rider of this launch publishes it), a hidden row and
  // 1 + 2 x 512 columns within a workgroup's LDS
  if (a.nOpt <= 64 || a.nOpt > DISC_MAX_OPT || a.nDense != 1 + 2 * a.nOpt || a.nOut != a.nDense || a.nSig != 0 || a.deferBeta || a.H < 1 || a.H > 2048 ||
      a.ldWo < a.nDense || a.ldDo < a.nDense) return hipErrorInvalidValue;
  if (a.nOpt <= 128) return headWideLaunch<2>(a, maxRows, ex, s);
  if (a.nOpt <= 256) return headWideLaunch<4>(a, maxRows, ex, s);
  return headWideLaunch<8>(a, maxRows, ex, s);
}

}  // namespace hl
