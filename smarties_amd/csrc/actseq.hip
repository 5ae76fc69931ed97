// smarties_amd/csrc/actseq.hip -- rollout inference of recurrent nets for MANY agents in one launch (hl_forward_sequences).
//
//   reference: ReplayMemory/MemoryBuffer.cpp:440-467 (agentToMinibatch: the agent's last min(nnBPTTseq, t) + 1 steps),
//   Approximator::forward(agent) (every step of that window forwarded from a zero recurrent state, the last one's output is the
//   policy's input), Network/Layers/Layer_LSTM.h:78-165, Layer_MGU.h, Layer_Base.h:64-113 (one step of each layer type),
//   Layers.h:347-361 (parametric residual), Episode.h:172-183 (appended observations).
//
// hl_forward_sequence serves ONE agent with the training pass's window kernels (rec.hip) plus the output-layer launch.  Here a
// launch has min(n, CUs) workgroups of 256 threads; each
//   * stages the recurrent stack's weights in LDS ONCE (transposed, a row per gate column, 16-byte reads; stacks beyond the LDS
//     budget read them through the L2), biases and residual parameters behind them,
//   * then walks its agents i = blockIdx.x, blockIdx.x + gridDim.x, ...: the window's raw states come straight from pinned host
//     memory (prefix sums of the window lengths stand beside them), are standardised into LDS in one round, the window runs with
//     the recurrent state in LDS and nothing stored per step, the output layer follows in the same kernel (the arithmetic of
//     act_forward_kernel's tail, misc.hip), the outputs go to pinned host memory as doubles and the agent's stamp is released.
// hl_forward_sequences_dev (include/smarties_hip_dev.h) runs the same kernel on windows that lie in DEVICE memory (template parameter DEV):
// agent i's states are rows firstRow[i] + t rowStride of the caller's array, the tables are device arrays too, the newest
// nnBPTTseq + 1 + nAppendedObs rows are gathered into LDS, the outputs go to device memory and nothing is stamped -- ONE launch for any n.
// Gate sums: the G = gates x cells columns of a layer are spread over the 256 threads with P = 4 / 2 / 1 neighbouring lanes per
// column (G <= 64 / 128 / more), lane p summing the 16-byte chunks p, p + P, ... of the column; the shares are joined by shuffles, the
// first lane adds the bias and applies the gate's function, the cell's thread finishes the step behind ONE barrier (MGU: three).
// The sums are therefore formed in another order than in rec.hip and in the oracle: differences at the 1e-7 level.
#include "rec_dev.h"

namespace hl {

#define ASQ_MAXC 256       // cells per layer   (REC_GENC of rec.hip)
#define ASQ_MAXIN 1024     // inputs per layer  (REC_GENIN)

// LDS copy of a layer's weights: TRANSPOSED, one row per column o of the blob's [W_in; W_rec] -- [W_in column, padded to 4 | W_rec
// column, padded to 4], zeros in the padding -- with a row pitch whose quarter is odd, so that the 16-byte reads of neighbouring
// columns spread over all banks (as lstm_forward_lds_kernel of rec.hip lays them out)
struct AsqGeo { int inPad, recPad, ld; };
__host__ __device__ __forceinline__ AsqGeo asqGeo(int nIn, int nC) {
  AsqGeo g; g.inPad = (nIn + 3) & ~3; g.recPad = (nC + 3) & ~3; g.ld = g.inPad + g.recPad;
  if (!((g.ld >> 2) & 1)) g.ld += 4;
  return g;
}

// this lane's share of column o against an operand segment v[0..n): LDS copy -- the 16-byte chunks p, p + P, ... of the column's row
// (the operand is read to the padded length: zeros in the weights there, finite values in the operand); global memory -- all rows
// of the blob (one lane per column there).  The P lanes of a column are neighbours: asqJoin adds their shares.
template <bool LDSW>
__device__ __forceinline__ float asqDot(const float* sW, const float* gW, int gp, int row0, int o, const float* v, int n, int p, int P) {
  float acc = 0.f;
  if constexpr (LDSW) {
    const float4* w4 = reinterpret_cast<const float4*>(sW);
    const float4* v4 = reinterpret_cast<const float4*>(v);
    const int nq = (n + 3) >> 2;
#pragma unroll 4
    for (int q = p; q < nq; q += P) {
      const float4 w = w4[q], x = v4[q];
      acc = fmaf(x.x, w.x, acc); acc = fmaf(x.y, w.y, acc); acc = fmaf(x.z, w.z, acc); acc = fmaf(x.w, w.w, acc);
    }
  } else {
    const float* w = gW + (size_t)row0 * gp + o;      // (P == 1 here)
#pragma unroll 8
    for (int i = 0; i < n; ++i) acc = fmaf(v[i], w[(size_t)i * gp], acc);
  }
  return acc;
}
__device__ __forceinline__ float asqJoin(float acc, int P) {
  if (P >= 2) acc += __shfl_xor(acc, 1, 64);
  if (P >= 4) acc += __shfl_xor(acc, 2, 64);
  return acc;
}

// GATES: 4 LSTM, 2 MGU, 1 plain recurrent layers -- at compile time: with the layer type read from the arguments the walk of a window was
// mostly scalar branches (measured: 2.2 us per layer-step at 32 cells)
// DEV: the windows lie in the caller's device memory (hl_forward_sequences_dev) -- strided rows gathered here, the newest recWin + nApp
// states of each; outputs to device memory, completion is stream order.  From sStates on both variants run the same code
template <bool LDSW, int GATES, bool DEV>
__global__ __launch_bounds__(256) void act_seq_kernel(ActSeqArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sDyn[];      // [weights (LDSW)] [bias | residual w | residual b per layer] [window states]
  __shared__ __attribute__((aligned(16))) float sBuf[2][ASQ_MAXIN];      // input of the current layer / output of the current block
  __shared__ __attribute__((aligned(16))) float sPrevOut[HL_MAX_HIDDEN][ASQ_MAXC];
  __shared__ __attribute__((aligned(16))) float sFP[ASQ_MAXC];           // MGU: previous output x forget gate
  __shared__ float sPrevSt[HL_MAX_HIDDEN][ASQ_MAXC];
  __shared__ float sX[4 * ASQ_MAXC];                       // the layer-step's gate values
  __shared__ int sL[HL_MAX_HIDDEN][8];                     // per layer: inputs, cells, width of the residual (0: none), LDS offsets of weights / parameters, LDS geometry, blob offset
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* W = a.W;
  float* sPar = sDyn + a.parOff;
  float* sStates = sDyn + a.stOff;
  // ---- once per workgroup: weights, biases, residual parameters ----
  if constexpr (LDSW) { for (int e = tid; e < a.parOff; e += 256) sDyn[e] = 0.f; }
  for (int e = tid; e < 2 * ASQ_MAXIN; e += 256) (&sBuf[0][0])[e] = 0.f;      // (operands are read to a padded length: finite values there)
  if (tid < ASQ_MAXC) sFP[tid] = 0.f;
  // (every access to the layer table of the argument segment has a constant index: the loops below read these copies)
#pragma unroll
  for (int q = 0; q < HL_MAX_HIDDEN; ++q) if (tid == q && q < a.nL) {
    const ActSeqLayer& L = a.L[q]; const AsqGeo g = asqGeo(L.nIn, L.nC);
    sL[q][0] = L.nIn; sL[q][1] = L.nC; sL[q][2] = L.hasRes ? L.resW : 0; sL[q][3] = L.wOff; sL[q][4] = L.pOff; sL[q][5] = g.inPad; sL[q][6] = g.ld;
    sL[q][7] = (int)L.indW;      // (act_seq_plan: below 2^31)
  }
  __syncthreads();
  for (int j = 0; j < a.nL; ++j) {
    const ActSeqLayer L = a.L[j];
    const int G = GATES * L.nC;
    if constexpr (LDSW) {
      const int gp = GATES == 1 ? (L.nC + 7) & ~7 : G;      // row pitch of the blob (Layer_Base.h:46 / Layer_LSTM.h)
      const AsqGeo geo = asqGeo(L.nIn, L.nC);
      const int total = (L.nIn + L.nC) * gp;
      const float* src = W + L.indW;
      // eight loads in flight per thread
      for (int e0 = tid; e0 < total; e0 += 256 * 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u; v[u] = e < total ? src[e] : 0.f; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u; if (e < total) { const int i = e / gp, o = e - i * gp;
          if (o < G) sDyn[L.wOff + o * geo.ld + (i < L.nIn ? i : geo.inPad + i - L.nIn)] = v[u]; } }
      }
    }
    for (int o = tid; o < G; o += 256) sPar[L.pOff + o] = W[L.indB + o];
    if (L.hasRes) for (int o = tid; o < L.resW; o += 256) { sPar[L.pOff + G + o] = W[L.indWr + o]; sPar[L.pOff + G + L.resW + o] = W[L.indBr + o]; }
  }
  const int dS = a.dS, dIn = a.L[0].nIn, nL = a.nL, maxSteps = a.recWin + a.nApp;
  __syncthreads();
  // ---- the workgroup's agents ----
  for (int ag = blockIdx.x; ag < a.n; ag += gridDim.x) {
    int off = 0, len = 0;
    if constexpr (DEV) len = a.nSteps[ag]; else { off = a.offset[ag]; len = a.offset[ag + 1] - off; }
    const int ns = max(1, min(len, maxSteps));      // (the host refuses longer windows; the LDS copy holds maxSteps states)
    const int win = min(ns, a.recWin), ctx = ns - win;
    if constexpr (DEV) {
      // the window's newest ns rows of the caller's array (MemoryBuffer::agentToMinibatch's truncation), gathered and standardised in one
      // round; row arithmetic in 64 bits
      const long long stride = a.rowStride, row0 = a.firstRow[ag] + (long long)(max(len, 1) - ns) * stride;
      const int total = ns * dS;
      for (int e0 = tid; e0 < total; e0 += 256 * 4) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int e = e0 + 256 * u, g = e / dS, i = e - g * dS; v[u] = e < total ? a.states[(row0 + g * stride) * dS + i] : 0.f; }
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int e = e0 + 256 * u; if (e < total) { const int i = e % dS; sStates[e] = (v[u] - a.stMean[i]) * a.stScale[i]; } }
      }
    } else {
      // the whole window in one round from pinned host memory, standardised (Episode::standardizedState, Episode.h:172-183)
      const float* src = a.states + (size_t)off * dS;
      const int total = ns * dS;
      for (int e0 = tid; e0 < total; e0 += 256 * 4) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int e = e0 + 256 * u; v[u] = e < total ? src[e] : 0.f; }
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int e = e0 + 256 * u; if (e < total) { const int i = e % dS; sStates[e] = (v[u] - a.stMean[i]) * a.stScale[i]; } }
      }
    }
    // zero recurrent state (MemoryBuffer.cpp:440-467: the window starts the recurrence)
    for (int e = tid; e < nL * ASQ_MAXC; e += 256) { (&sPrevOut[0][0])[e] = 0.f; (&sPrevSt[0][0])[e] = 0.f; }
    __syncthreads();
    int cur = 0;
    for (int k = 0; k < win; ++k) {
      // the step's input: its state followed by the nApp before it; steps before the first given state repeat it (recInputAt, acting)
      for (int e = tid; e < dIn; e += 256) { const int j = e / dS, i = e - j * dS; const int g = max(ctx + k - j, 0); sBuf[0][e] = sStates[g * dS + i]; }
      __syncthreads();
      cur = 0;
      for (int j = 0; j < nL; ++j) {
        // (the layer's numbers from LDS: out of the kernel-argument segment they stayed in scalar registers across the loops, more than there are)
        const int nIn = sL[j][0], nC = sL[j][1], resW = sL[j][2], wOff = sL[j][3], pOff = sL[j][4], G = GATES * nC;
        const int gp = GATES == 1 ? (nC + 7) & ~7 : G;
        AsqGeo geo; geo.inPad = sL[j][5]; geo.ld = sL[j][6];
        const float* gW = LDSW ? W : W + sL[j][7];
        const float* in = sBuf[cur];
        const float* po = sPrevOut[j];
        const float* bias = sPar + pOff;
        // P neighbouring lanes per column
        // (weights through the L2: a thread per column, as the general kernels of rec.hip)
        const int sh = !LDSW ? 0 : G <= 64 ? 2 : G <= 128 ? 1 : 0, P = 1 << sh, cols = 256 >> sh, p = tid & (P - 1), o0 = tid >> sh;
        // gate sums.  LSTM (4 nC columns: cell input, input / forget / output gate) and plain recurrent layers (nC columns): inputs and
        // previous outputs; MGU (forget gate, state): the state columns take the inputs now and (previous output x forget gate) below
        for (int o = o0; o < G; o += cols) {
          const float* sWo = sDyn + wOff + o * geo.ld;
          float acc = asqDot<LDSW>(sWo, gW, gp, 0, o, in, nIn, p, P);
          if (GATES != 2 || o < nC) acc += asqDot<LDSW>(sWo + geo.inPad, gW, gp, nIn, o, po, nC, p, P);
          acc = asqJoin(acc, P);
          if (p == 0) {
            float x = acc + bias[o];
            if constexpr (GATES == 4) { if (o >= nC) x = recSigm(x); }                   // Layer_LSTM.h:78-120: the gates
            else if constexpr (GATES == 2) { if (o < nC) { x = recSigm(x); sFP[o] = po[o] * x; } }      // Layer_MGU.h: forget gate
            else x = actEval(a.func, x);                                         // Layer_Base.h:64-113
            sX[o] = x;
          }
        }
        __syncthreads();
        if constexpr (GATES == 2) {
          for (int o = nC + o0; o < G; o += cols) {
            float acc = asqDot<LDSW>(sDyn + wOff + o * geo.ld + geo.inPad, gW, gp, nIn, o, sFP, nC, p, P);
            acc = asqJoin(acc, P);
            if (p == 0) sX[o] = actEval(HL_FUNC_TANH, sX[o] + acc);
          }
          __syncthreads();
        }
        if (tid < nC) {
          float out;
          if constexpr (GATES == 4) {
            const float st = sX[tid] * sX[nC + tid] + sPrevSt[j][tid] * sX[2 * nC + tid];
            out = sX[3 * nC + tid] * actEval(HL_FUNC_TANH, st);
            sPrevSt[j][tid] = st;
          } else if constexpr (GATES == 2) {
            const float f = sX[tid];
            out = f * sX[nC + tid] + (1.f - f) * po[tid];
          } else out = sX[tid];
          float blk = out;                                   // ParametricResidualLayer::forward (Layers.h:347-361)
          if (tid < resW) blk += in[tid] * bias[G + tid] + bias[G + resW + tid];
          sBuf[cur ^ 1][tid] = blk;
          sPrevOut[j][tid] = out;      // (every read of the previous output lies in front of the barriers above)
        }
        __syncthreads();
        cur ^= 1;
      }
    }
    // output layer (Linear) + ParamLayer: one output per wavefront at a time, lanes over the hidden units
    const float* hid = sBuf[cur];
    const int H = sL[nL - 1][1];
    double* out = a.out + (size_t)ag * a.nOut;
    for (int o = wave; o < a.nDense; o += 4) {
      float s = 0.f;
      for (int k = lane; k < H; k += 64) s = fmaf(hid[k], W[a.indWo + (long long)k * a.ldWo + o], s);
      s = waveSumF(s);
      if (lane == 0) out[o] = (double)actEval(a.outFunc, s + W[a.indBo + o]);
    }
    if (tid < a.nSig) out[a.nDense + tid] = (double)W[a.indBp + tid];
    if constexpr (!DEV) {
      __threadfence_system();
      __syncthreads();
      if (tid == 0) __hip_atomic_store(const_cast<unsigned*>(a.done) + ag, a.tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }      // (DEV: the next agent's first barrier stands behind these reads of sBuf)
  }
}

// floats of LDS behind the static arrays: the weights (0 where they stay in global memory), the per-layer parameters, one window.
// Fills the layers' offsets.  The static arrays take 31 KB of the 160 KB.
constexpr size_t ASQ_LDS_BUDGET = 124 * 1024;
bool act_seq_plan(ActSeqArgs* a) {
  if (a->nL < 1 || a->nL > HL_MAX_HIDDEN || (a->gates != 4 && a->gates != 2 && a->gates != 1)) return false;
  size_t w = 0, par = 0;
  for (int j = 0; j < a->nL; ++j) {
    ActSeqLayer& L = a->L[j];
    if (L.indW < 0 || L.indW >= (1ll << 31)) return false;
    if (L.nC < 1 || L.nC > ASQ_MAXC || L.nIn < 1 || L.nIn > ASQ_MAXIN || (L.hasRes && L.resW > L.nC)) return false;
    if (j > 0 && L.nIn != a->L[j - 1].nC) return false;
    const int G = a->gates * L.nC, gp = a->gates == 1 ? (L.nC + 7) & ~7 : G;
    L.wOff = (int)w; w += (size_t)G * asqGeo(L.nIn, L.nC).ld; (void)gp;
    L.pOff = (int)par; par += (size_t)G + (L.hasRes ? 2 * L.resW : 0);
  }
  if (a->L[0].nIn != a->dS * (1 + a->nApp)) return false;
  const size_t st = (size_t)(a->recWin + a->nApp) * a->dS;
  if (st * sizeof(float) > 64 * 1024) return false;      // (the parameters take up to 48 KB: both always fit)
  a->ldsW = (w + par + st) * sizeof(float) <= ASQ_LDS_BUDGET ? 1 : 0;
  if (!a->ldsW) w = 0;
  a->parOff = (int)w; a->stOff = (int)(w + par); a->ldsBytes = (w + par + st) * sizeof(float);
  return true;
}
template <bool LDSW, int GATES, bool DEV> static hipError_t actSeqLaunch(const ActSeqArgs& a, int nBlocks, hipStream_t s) {
  hipError_t e = ensureDynLds(reinterpret_cast<const void*>(act_seq_kernel<LDSW, GATES, DEV>), a.ldsBytes); if (e != hipSuccess) return e;
  hipLaunchKernelGGL((act_seq_kernel<LDSW, GATES, DEV>), dim3(nBlocks), dim3(256), a.ldsBytes, s, a);
  return hipGetLastError();
}
template <bool DEV> static hipError_t actSeqPick(const ActSeqArgs& a, int nBlocks, hipStream_t s) {
  if (a.gates == 4) return a.ldsW ? actSeqLaunch<true, 4, DEV>(a, nBlocks, s) : actSeqLaunch<false, 4, DEV>(a, nBlocks, s);
  if (a.gates == 2) return a.ldsW ? actSeqLaunch<true, 2, DEV>(a, nBlocks, s) : actSeqLaunch<false, 2, DEV>(a, nBlocks, s);
  return a.ldsW ? actSeqLaunch<true, 1, DEV>(a, nBlocks, s) : actSeqLaunch<false, 1, DEV>(a, nBlocks, s);
}
hipError_t launch_act_seq(const ActSeqArgs& a, int nBlocks, hipStream_t s) { return actSeqPick<false>(a, nBlocks, s); }
hipError_t launch_act_seq_dev(const ActSeqArgs& a, int nBlocks, hipStream_t s) {
  if (a.n < 1 || nBlocks < 1) return hipSuccess;
  if (!a.firstRow || !a.nSteps || !a.states || !a.out || a.rowStride < 1) return hipErrorInvalidValue;
  return actSeqPick<true>(a, nBlocks, s);
}

}  // namespace hl
