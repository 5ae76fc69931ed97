// smarties_amd/csrc/headppo.hip -- PPO learners (include/smarties_hip_ppo.h): both nets' output layers, the head of PPO::Train and both
// output layers' backward as ONE launch behind the actor's and the critic's forward chains; Adam over both nets with the serial penalty /
// DKL_target chain.
//
//   PPO::Train (Learners/PPO_train.cpp:28-78, with PPO_learnDKLt, PPO_PENALKL and PPO_CLIPPED as PPO.cpp:11-13 defines them) in fp64 on
//   Continuous_policy (Math/Continuous_policy.h; SMARTIES_OPPOSITE_KL, the forms of head_body.h) or Discrete_policy =
//   Discrete_policy_t<SoftPlus> (Math/Discrete_policy.h); updatePenalizationCoef (:14-25), updateDKL_target (PPO_common.cpp:15-26).
//
// ppo_head_kernel<NQ, DISC>: laid out as dqn_head_kernel (headdq.hip), ONE WORKGROUP of four wavefronts per 16 minibatch rows.
//
//   A  products  the actor's P = Ya Wo + b on v_mfma_f32_16x16x4_f32: wavefront w owns the 16-column tiles w, w + 4, .. (NQ of them; the
//                dimA <= 16 means of a continuous policy are wavefront 0's one tile), the Ya chunk of 64 hidden units staged in LDS at
//                pitch 68 (4 mod 16), Wo by direct loads.  The loads of PP_SB = 4 reduction steps -- 4 NQ per lane, 32 at 512 options --
//                are issued together, ahead of the 4 NQ MFMAs that use them (loads next to their MFMAs made
//                dpg_target_kernel wait out a memory round trip per step).  k ascends within every accumulator.
//                The critic's one column: wavefront 3, lane = (row lane & 15, quarter lane >> 4) walks its quarter of the last hidden
//                block in ascending order; the quarters are joined (q0 + q1) + (q2 + q3).  P rows [16][ldP] (ldP = 64 NQ + 4) and V stay in LDS.
//   B  head      continuous: the 16 lanes of a row's group (thread = (row tid / 16, component tid % 16)), sums over the group by
//                butterflies of width 16; discrete: a wavefront per row, four rows in turn, option lane + 64 s in slot s, each lane's
//                slots in ascending order, then waveSum.  penalCoef comes from device memory (queued steps need no host round trip).
//                The delta rows go back to LDS over the P rows and out to memory for the dW launches; RHO, D_KL and isOff of every row
//                go to PpoHeadArgs::rowStat for the scalar chain.
//   C  backward  dYa = delta Wo^T on the MFMA, Wo tiles transposed through the wavefront's own LDS region (phase C of dqn_head_kernel);
//                dYc = g wo, rank 1.
//
// Every sum has a fixed order, there are no atomics: the same inputs give the same bits.
// LDS (dynamic): (16 (64 NQ + 4) + 4 x 16 x 68 + 64 + 16 + 16) x 4 bytes = 22 KB at NQ = 1, 50 KB at NQ = 8.
#include <algorithm>
#include "dev_common.h"

namespace hl {

constexpr int PP_KC = 64, PP_LDY = PP_KC + 4, PP_SB = 4;      // hidden units (A) / outputs (C) per chunk; pitch of the staged chunk; reduction steps whose Wo loads go out together
typedef float ppF4 __attribute__((ext_vector_type(4)));

template <int NQ> constexpr int ppLdP() { return 64 * NQ + 4; }
size_t ppo_head_lds(int nq) { return ((size_t)16 * (64 * nq + 4) + (size_t)4 * 16 * PP_LDY + 64 + 16 + 16) * sizeof(float); }

__device__ __forceinline__ double ppSp(double x) { return (x + sqrt(1 + x * x)) / 2; }            // SoftPlus::_eval (Functions.h:541-584)
__device__ __forceinline__ double ppSpDiff(double x) { return (1 + x / sqrt(1 + x * x)) / 2; }
__device__ __forceinline__ double ppGroupSum(double v) {      // over the 16 lanes of a row's group, the same tree for every group
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
  return v;
}

// what lane `on` of a row's group (continuous) or lane 0 of its wavefront (discrete) leaves behind the policy's part: the critic's output
// gradient (verr x isOff, PPO_train.cpp:77), the write-backs setMseDklImpw(verr, DKL, RHO, 1 + C, 1 - C) and setValues(t, V, V), the rows
// of the scalar chain
__device__ __forceinline__ void ppoRowTail(const PpoHeadArgs& q, int b, int r, long long slot, double RHO, double DKL, bool isOff, double gain, double ret,
                                           float Vf32, float* sDc) {
  const HeadArgs& a = q.h; const int B = a.B;
  const double Vd = (double)Vf32, verr = ret - Vd;
  const float dc = (float)(verr * (isOff ? 1 : 0));
  sDc[r] = dc; q.cDOut[(size_t)b * q.cLdDo] = dc; q.cV[b] = Vd; q.cG[b] = (double)dc; q.gain[b] = gain;
  q.rowStat[b] = RHO; q.rowStat[(size_t)B + b] = DKL; q.rowStat[2 * (size_t)B + b] = isOff ? 1.0 : 0.0;
  a.bt.rho[b] = RHO; a.bt.dkl[b] = DKL; a.bt.far[b] = isOff ? 1 : 0;
  a.bt.pEid[b] = a.bt.eid[b]; a.bt.pNextOf[b] = -1;      // (nothing is written to stateValue[t+1])
  const float E = (float)verr, D = (float)DKL, Wn = (float)RHO;
  a.bt.oldDQ[b] = a.rp.DQ[slot]; a.bt.oldDKL[b] = a.rp.DKL[slot]; a.bt.oldW[b] = a.rp.IMPW[slot]; a.bt.oldV[b] = a.rp.V[slot]; a.bt.oldADV[b] = a.rp.ADV[slot];
  a.bt.newDQ[b] = E; a.bt.newDKL[b] = D; a.bt.newW[b] = Wn; a.bt.newV[b] = Vf32; a.bt.newQ[b] = Vf32;
  a.rp.DQ[slot] = E; a.rp.DKL[slot] = D; a.rp.IMPW[slot] = Wn; a.rp.V[slot] = Vf32; a.rp.ADV[slot] = 0.f;
  a.bt.dq[b] = (double)E;
}
// gain = RHO (ret - Vold) on the STORED estimate and value, with the two zeroings of PPO_CLIPPED (PPO_train.cpp:50-53)
__device__ __forceinline__ double ppoGain(double RHO, double ret, double Vold, double C) {
  double gain = RHO * (ret - Vold);
  if (ret > 0 && RHO > 1 + C) gain = 0;
  if (ret < 0 && RHO < 1 - C) gain = 0;
  return gain;
}
__device__ __forceinline__ bool ppoIsOff(double RHO, double C) {      // isFarPolicyPPO (Episode.h:22-27), Fval
  const float W = (float)RHO, Cf = (float)C;
  return W > 1.f + Cf || W < 1.f - Cf;
}

template <int NQ, bool DISC>
__global__ __launch_bounds__(256) void ppo_head_kernel(PpoHeadArgs q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smemPp[];
  const HeadArgs& a = q.h;
  constexpr int LDP = ppLdP<NQ>();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int B = a.B, nC = a.nDense, nOut = a.nOut, H = a.H, dA = a.dA;
  const int row0 = (int)blockIdx.x * 16;
  if (row0 >= B) return;
  float* sP = reinterpret_cast<float*>(smemPp);
  float* sStage = sP + (size_t)16 * LDP;
  float* sPart = sStage + (size_t)4 * 16 * PP_LDY;      // [4 quarters][16 rows]
  float* sV = sPart + 64;
  float* sDc = sV + 16;
  const float* __restrict__ Wo = a.params + a.indWo;
  const float* __restrict__ cWo = q.cW + q.cIndWo;
  const int ldWo = a.ldWo;

  // ---- phase A: the critic's column (wavefront 3), the actor's P = Ya Wo + b -------------------------------------------------
  if (wave == 3) {
    const int r = li, row = row0 + r, per = (q.cH + 3) / 4, k0 = lg * per, k1 = min(q.cH, k0 + per);
    float s = 0.f;
    if (row < B) for (int k = k0; k < k1; ++k) s = fmaf(q.cYin[(size_t)row * q.cLd + k], cWo[(size_t)k * q.cLdWo], s);
    sPart[lg * 16 + r] = s;
  }
  ppF4 acc[NQ];
#pragma unroll
  for (int t = 0; t < NQ; ++t) acc[t] = ppF4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < H; k0 += PP_KC) {
    __syncthreads();      // (the chunk before this one has been read)
    {   // stage: thread -> (row tid / 16, hidden units k0 + 4 (tid % 16) ..+3); rows and units beyond the arrays: zeros
      const int r = tid >> 4, kk = (tid & 15) * 4, k = k0 + kk, row = row0 + r;
      ppF4 v{0.f, 0.f, 0.f, 0.f};
      if (row < B && k < a.ldY) v = *reinterpret_cast<const ppF4*>(a.Yin + (size_t)row * a.ldY + k);      // (ldY is a multiple of 16: the four lie inside the row)
      if (k + 0 >= H) v.x = 0.f;
      if (k + 1 >= H) v.y = 0.f;
      if (k + 2 >= H) v.z = 0.f;
      if (k + 3 >= H) v.w = 0.f;
      *reinterpret_cast<ppF4*>(sStage + (size_t)r * PP_LDY + kk) = v;
    }
    __syncthreads();
    const int ks = min(PP_KC / 4, (H - k0 + 3) / 4);
    for (int s0 = 0; s0 < ks; s0 += PP_SB) {
      float av[PP_SB], bv[PP_SB][NQ];
#pragma unroll
      for (int u = 0; u < PP_SB; ++u) {      // every load of these steps first (steps beyond the chunk: zeros against the zero-filled staging)
        const int s = s0 + u, k = k0 + 4 * s + lg; const bool kin = s < ks && k < H;
        av[u] = sStage[(size_t)li * PP_LDY + 4 * s + lg];      // (4 s + lg <= 63)
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
          const int c = 16 * (wave + 4 * t) + li; const bool on = kin && c < nC;
          bv[u][t] = on ? Wo[(size_t)k * ldWo + c] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < PP_SB; ++u)
#pragma unroll
        for (int t = 0; t < NQ; ++t)
          if (16 * (wave + 4 * t) < nC) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u][t], acc[t], 0, 0, 0);      // (wavefront-uniform)
    }
  }
  // the pre-activations into LDS: result element i of a lane is (row 4 lg + i, column li) of its tile
#pragma unroll
  for (int t = 0; t < NQ; ++t) {
    const int c = 16 * (wave + 4 * t) + li;      // < 64 NQ
    const bool on = c < nC;
    const float bo = on ? a.params[a.indBo + c] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) sP[(size_t)(4 * lg + i) * LDP + c] = on ? acc[t][i] + bo : 0.f;
  }
  __syncthreads();
  if (tid < 16) sV[tid] = ((sPart[tid] + sPart[16 + tid]) + (sPart[32 + tid] + sPart[48 + tid])) + q.cW[q.cIndBo];      // (the critic's output layer is Linear)
  __syncthreads();

  // ---- phase B: the head ------------------------------------------------------------------------------------------------------
  const double penalCoef = q.pen[0], C = q.Cpol;
  if (!DISC) {
    const int r = tid >> 4, i = tid & 15, row = row0 + r;
    const bool valid = row < B, on = valid && i < dA;
    const long long slot = valid ? a.bt.slot[row] : 0;
    const double MAXM = 8.31776613503286;
    double lw = 0, kl = 0, mean = 0, stdev = 1, invStd = 1, dPos = 0, bMean = 0, bStd = 1, pp = 0, act = 0;
    float xo = 0.f; bool bnd = false;
    if (on) {
      bnd = a.bounded[i] != 0;
      act = a.rp.A[(size_t)slot * dA + i];
      bMean = a.rp.MU[(size_t)slot * 2 * dA + i]; bStd = a.rp.MU[(size_t)slot * 2 * dA + dA + i];
      xo = sP[(size_t)r * LDP + i];
      mean = (double)(a.outFunc == HL_FUNC_LINEAR ? xo : actEval(a.outFunc, xo));
      pp = (double)a.params[a.indBp + i];      // ParamLayer, Linear
      stdev = ppSp(pp); invStd = 1 / stdev; dPos = ppSpDiff(pp);
      const double bInv = 1 / bStd;
      const double m = bnd ? (mean > MAXM ? MAXM : (mean < -MAXM ? -MAXM : mean)) : mean;
      const double u1 = (act - m) * invStd, u2 = (act - bMean) * bInv;
      const double qq = stdev * bInv, lq = log(qq);
      lw = (u2 * u2 - u1 * u1) / 2 - lq;      // (head_body.h: the Jacobian and the constants cancel)
      const double dm = (mean - bMean) * bInv;
      kl = (qq * qq - 1 + dm * dm - 2 * lq) / 2;
    }
    const double logW = ppGroupSum(lw), DKL = ppGroupSum(kl);
    const double RHO = exp(logW > 7 ? 7 : (logW < -7 ? -7 : logW));
    const bool isOff = ppoIsOff(RHO, C);
    const double ret = valid ? (double)a.rp.RET[slot] : 0.0, Vold = valid ? (double)a.rp.V[slot] : 0.0;
    const double gain = ppoGain(RHO, ret, Vold, C);
    float dl = 0.f;
    if (on) {
      // policyGradient(a, gain) = gradLogP (NormalPolicy / the bounded policy as head_body.h has it); KLDivGradient(mu, -penalCoef)
      double polM, polS;
      if (bnd) {
        const double dLogPdMean = (act - mean) * invStd * invStd;
        const double m = mean > MAXM ? MAXM : (mean < -MAXM ? -MAXM : mean);
        const double u = (act - m) * invStd;
        polS = dPos * gain * ((u * u - 1) * invStd);
        if (mean >= MAXM && gain * dLogPdMean > 0) polM = 0;
        else if (mean <= -MAXM && gain * dLogPdMean < 0) polM = 0;
        else polM = gain * dLogPdMean;
      } else {
        const double u = (act - mean) * invStd;
        polM = gain * (u * invStd);
        polS = dPos * gain * ((u * u - 1) * invStd);
      }
      const double invVarMu = 1 / (bStd * bStd);
      const double penM = -penalCoef * ((mean - bMean) * invVarMu);
      const double penS = dPos * -penalCoef * ((invVarMu - invStd * invStd) * stdev);
      const double W1 = 1;      // weightSum2Grads(polG, penG, 1)
      const double gM = W1 * polM + (1 - W1) * penM, gS = W1 * polS + (1 - W1) * penS;
      dl = (float)gM;
      a.bt.G[(size_t)row * nOut + i] = (double)dl;
      a.bt.G[(size_t)row * nOut + dA + i] = (double)(float)gS;
      a.bt.gParam[(size_t)row * dA + i] = (float)gS;
      a.bt.O[(size_t)row * nOut + i] = mean; a.bt.O[(size_t)row * nOut + dA + i] = pp;
      if (a.outFunc != HL_FUNC_LINEAR) dl *= actDiff(a.outFunc, xo, (float)mean);      // BaseLayer::backward: deltas *= f'(x, y)
      a.dOut[(size_t)row * a.ldDo + i] = dl;
    }
    sP[(size_t)r * LDP + i] = dl;      // (zeros beyond dimA and beyond the rows: phase C reads whole groups of four)
    if (i == 0) { if (valid) ppoRowTail(q, row, r, slot, RHO, DKL, isOff, gain, ret, sV[r], sDc); else sDc[r] = 0.f; }
  } else {
    const double EPS = 2.220446049250313e-16;
    const int nOpt = nC;
    for (int j = 0; j < 4; ++j) {
      const int r = wave + 4 * j, row = row0 + r;
      float* sRow = sP + (size_t)r * LDP;
      if (row >= B) {
#pragma unroll
        for (int s = 0; s < NQ; ++s) sRow[lane + 64 * s] = 0.f;
        if (lane == 0) sDc[r] = 0.f;
        continue;
      }
      const long long slot = a.bt.slot[row];
      float xo[NQ]; double y[NQ], un[NQ], mu[NQ], lr[NQ];
      double sZ = 0;
#pragma unroll
      for (int s = 0; s < NQ; ++s) {
        const int c = lane + 64 * s; const bool on = c < nOpt;
        xo[s] = on ? sRow[c] : 0.f;
        y[s] = on ? (double)(a.outFunc == HL_FUNC_LINEAR ? xo[s] : actEval(a.outFunc, xo[s])) : 0.0;
        un[s] = on ? ppSp(y[s]) : 0.0; sZ += un[s];
        mu[s] = on ? a.rp.MU[(size_t)slot * nOpt + c] : 1.0;
        if (on) a.bt.O[(size_t)row * nOut + c] = y[s];
      }
      const double Z = fmax(waveSum(sZ), EPS);
      double act = 0;
      if (lane == 0) act = discreteLabel(a, slot);
      const int label = min(max((int)floor(__shfl(act, 0, 64)), 0), nOpt - 1);      // (a label beyond the options: the last one, never an index out of the arrays)
      const int labLane = label & 63, labQ = label >> 6;
      double sKl = 0, sTp = 0, pL = 0, mL = 1;
#pragma unroll
      for (int s = 0; s < NQ; ++s) {
        const bool on = lane + 64 * s < nOpt;
        const double p = un[s] / Z;
        lr[s] = on ? log(p / mu[s]) : 0.0;
        sKl += on ? p * lr[s] : 0.0;                                  // KLDivergence
        sTp += on ? (-penalCoef * (1 + lr[s]) / Z) * p : 0.0;         // KLDivGradient(mu, -penalCoef): sum_j tmp_j p_j
        if (s == labQ) { pL = p; mL = mu[s]; }
      }
      const double RHO = __shfl(pL, labLane, 64) / __shfl(mL, labLane, 64);      // importanceWeight
      const double DKL = waveSum(sKl), tp = waveSum(sTp);
      const bool isOff = ppoIsOff(RHO, C);
      const double ret = (double)a.rp.RET[slot], Vold = (double)a.rp.V[slot];
      const double gain = ppoGain(RHO, ret, Vold, C);
#pragma unroll
      for (int s = 0; s < NQ; ++s) {
        const int c = lane + 64 * s;
        float dl = 0.f;
        if (c < nOpt) {
          const double dP = ppSpDiff(y[s]);
          const double pol = ((c == label ? gain / un[s] : 0.0) - gain / Z) * dP;      // policyGradient(label, gain)
          const double pen = ((-penalCoef * (1 + lr[s]) / Z) - tp) * dP;
          const double W1 = 1;      // weightSum2Grads(polG, penG, 1)
          const double g = W1 * pol + (1 - W1) * pen;
          dl = (float)g;
          a.bt.G[(size_t)row * nOut + c] = (double)dl;
          if (a.outFunc != HL_FUNC_LINEAR) dl *= actDiff(a.outFunc, xo[s], (float)y[s]);
          a.dOut[(size_t)row * a.ldDo + c] = dl;
        }
        sRow[c] = dl;      // (c < 64 NQ < ldP: zeros beyond the options)
      }
      if (lane == 0) ppoRowTail(q, row, r, slot, RHO, DKL, isOff, gain, ret, sV[r], sDc);
    }
  }
  __syncthreads();

  // ---- phase C: dYa = delta Wo^T, the wavefront's tiles of 16 hidden units; dYc = g wo ----------------------------------------
  float* sW = sStage + (size_t)wave * 16 * PP_LDY;      // [16 units][68]: the wavefront's own region
  const int nK = (nC + 3) / 4;      // groups of four outputs
  for (int n0 = 16 * wave; n0 < H; n0 += 64) {
    ppF4 d4{0.f, 0.f, 0.f, 0.f};
    for (int o0 = 0; o0 < nC; o0 += PP_KC) {
      __builtin_amdgcn_wave_barrier(); __threadfence_block();      // (the chunk before this one has been read)
#pragma unroll
      for (int u = 0; u < 4; ++u) {      // lane -> (unit lg + 4 u, outputs o0 + 4 li ..+3): 16-byte loads along the weight row
        const int n = n0 + lg + 4 * u, o = o0 + 4 * li;
        ppF4 w{0.f, 0.f, 0.f, 0.f};
        if (n < H && o < ldWo) w = *reinterpret_cast<const ppF4*>(Wo + (size_t)n * ldWo + o);      // (ldWo is a multiple of 4)
        if (o + 0 >= nC) w.x = 0.f;
        if (o + 1 >= nC) w.y = 0.f;
        if (o + 2 >= nC) w.z = 0.f;
        if (o + 3 >= nC) w.w = 0.f;
        *reinterpret_cast<ppF4*>(sW + (size_t)(lg + 4 * u) * PP_LDY + 4 * li) = w;
      }
      __builtin_amdgcn_wave_barrier(); __threadfence_block();
      const int ks = min(PP_KC / 4, nK - o0 / 4);
      for (int s = 0; s < ks; ++s) {      // A = delta (row li, output o0 + 4 s + lg); B = Wo^T (output, unit n0 + li)
        const float av = sP[(size_t)li * LDP + o0 + 4 * s + lg];
        const float bv = sW[(size_t)li * PP_LDY + 4 * s + lg];
        d4 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, d4, 0, 0, 0);
      }
    }
    const int k = n0 + li;
    if (k < H) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = row0 + 4 * lg + i;
        if (row < B) {
          const float g = d4[i];
          a.Dres[(size_t)row * a.ldD + k] = g;
          a.D[(size_t)row * a.ldD + k] = g * actDiff(a.func, a.Xlast[(size_t)row * a.ldD + k], a.Ylast[(size_t)row * a.ldD + k]);
        }
      }
    }
  }
  {   // the critic: thread -> (row tid / 16, units tid % 16, + 16, ..)
    const int r = tid >> 4, row = row0 + r;
    if (row < B) {
      const float dc = sDc[r];
      for (int k = tid & 15; k < q.cH; k += 16) {
        const float g = cWo[(size_t)k * q.cLdWo] * dc;
        const size_t o = (size_t)row * q.cLd + k;
        q.cDres[o] = g; q.cD[o] = g * actDiff(q.cFunc, q.cX[o], q.cY[o]);
      }
    }
  }
}

template <int NQ, bool DISC> static hipError_t ppoHeadLaunch(const PpoHeadArgs& a, hipStream_t s) {
  const size_t lds = ppo_head_lds(NQ);
  hipError_t e = ensureDynLds(reinterpret_cast<const void*>(&ppo_head_kernel<NQ, DISC>), lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((ppo_head_kernel<NQ, DISC>), dim3((a.h.B + 15) / 16), dim3(256), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_head_ppo(const PpoHeadArgs& a, hipStream_t s) {
  const HeadArgs& h = a.h;
  const bool disc = h.nOpt > 0;
  // what the kernel is written for: the policy's outputs and nothing else, 16-byte loads along the activation and the weight rows
  if (h.B < 1 || h.H < 1 || h.H > 2048 || a.cH < 1 || a.cH > 2048 || a.cLd < a.cH || a.cLdDo < 1 || a.cLdWo < 1 || h.ldWo < h.nDense || (h.ldWo & 3) || (h.indWo & 3) ||
      h.ldDo < h.nDense || (h.ldY & 3) || h.ldY < h.H || h.ldD < h.H || h.deferBeta || !a.pen || !a.rowStat || !(a.Cpol < 1)) return hipErrorInvalidValue;
  if (!disc) {
    if (h.dA < 1 || h.dA > 16 || h.nDense != h.dA || h.nOut != 2 * h.dA || h.nSig != h.dA) return hipErrorInvalidValue;
    return ppoHeadLaunch<1, false>(a, s);
  }
  if (h.nOpt < 2 || h.nOpt > DISC_MAX_OPT || h.nDense != h.nOpt || h.nOut != h.nOpt || h.nSig != 0) return hipErrorInvalidValue;
  if (h.nOpt <= 64) return ppoHeadLaunch<1, true>(a, s);
  if (h.nOpt <= 128) return ppoHeadLaunch<2, true>(a, s);
  if (h.nOpt <= 256) return ppoHeadLaunch<4, true>(a, s);
  return ppoHeadLaunch<8, true>(a, s);
}

// ---- Adam over both nets; the serial scalar chain -----------------------------------------------------------------------------
// Workgroups 0 .. nb-1: twoNetAdamElement (dev_common.h) over the actor's range, then the critic's.  Workgroup nb, its first wavefront:
// the bookkeeping PPO::Train does per sample on penalUpdateCount / penalUpdateDelta / DKL_target (PPO_train.cpp:44-54; the reference's
// OpenMP threads race there: ascending b is this project's order), then updatePenalizationCoef (:14-25) -- with one rank
// DelayedReductor::update stores {count, delta} and get() returns them (its initial {0, 1} is never seen).  fp64 where the reference
// has Real and long double.  The rows' values come 64 at a time and are walked by lane reads, as the sweeps of misc.hip do.
__global__ __launch_bounds__(256) void ppo_adam_kernel(DpgAdamArgs q, PpoAdamArgs p) {
  const long long n = q.a[0].n + q.a[1].n;
  if (blockIdx.x + 1 < gridDim.x) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) twoNetAdamElement(q, e);
    return;
  }
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x, B = p.B;
  double coef = p.pen[0], tgt = p.pen[1], cnt = p.pen[2], del = p.pen[3];
  double lo = tgt / 1.5, hi = 1.5 * tgt;      // the two thresholds, formed again only where DKL_target moves (the same quotient and product)
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int b = b0 + lane; const bool in = b < B;
    const double rho = in ? p.rowStat[b] : 0.0, dkl = in ? p.rowStat[(size_t)B + b] : 0.0, off = in ? p.rowStat[2 * (size_t)B + b] : 0.0;
    const int m = min(64, B - b0);
    for (int j = 0; j < m; ++j) {
      const double R = __shfl(rho, j, 64), D = __shfl(dkl, j, 64); const bool isOff = __shfl(off, j, 64) != 0.0;
      cnt += 1;
      if (D < lo) del -= coef / 2;
      if (D > hi) del += coef;
      // updateDKL_target(isOff, RHO): the reference passes RHO where the parameter is called DivKL
      const double moved = (isOff && tgt > R) ? tgt * 0.9995 : ((!isOff && tgt < R) ? tgt * 1.0001 : tgt);
      if (moved != tgt) { tgt = moved; lo = tgt / 1.5; hi = 1.5 * tgt; }
    }
  }
  coef += 1e-4 * del / fmax(1.0, cnt);
  const double nnEPS = 1.1920928955078125e-07;      // std::numeric_limits<float>::epsilon() (Settings/Bund.h:118)
  if (coef <= nnEPS) coef = nnEPS;
  if (lane == 0) { p.pen[0] = coef; p.pen[1] = tgt; p.pen[2] = 0; p.pen[3] = 0; }
}
hipError_t launch_ppo_adam(const DpgAdamArgs& a, const PpoAdamArgs& p, hipStream_t s) {
  if (a.mode != NAF_TGT_KEEP || p.B < 1 || !p.pen || !p.rowStat) return hipErrorInvalidValue;
  const long long n = a.a[0].n + a.a[1].n;
  hipLaunchKernelGGL(ppo_adam_kernel, dim3((unsigned)((n + 255) / 256) + 1), dim3(256), 0, s, a, p);
  return hipGetLastError();
}

}  // namespace hl
