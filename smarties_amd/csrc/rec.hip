// smarties_amd/csrc/rec.hip -- recurrent (LSTM) hidden layers with truncated back-propagation through time.
//
//   reference: Network/Layers/Layer_LSTM.h:78-165 (forward / backward of one step), Network/Network.h:102-193
//   (forward with the previous step as recurrent input, backProp over the time series), Approximator.h:116-173
//   (every step of the window is forwarded), ReplayMemory/MemoryBuffer.cpp:391-402 (the window: min(nnBPTTseq, t)
//   steps before the sampled one), Network/Layers/Layers.h:324-393 (parametric residual).
//
// First device version of this path: ONE workgroup per sample walks the sample's window step by step (the recurrence
// is sequential; samples are independent), gates one per thread, weights read through the L2.  It stores, per
// (sample, step) row, the operands of the weight-gradient contractions -- inputs [in | previous output] and the four
// gate deltas -- so that all weight gradients (and Adam) are formed by the same dW kernel as for dense layers, as
// X^T delta over the rows; rows of unused steps carry zero deltas.
//
// Three families of kernels, each folded onto __device__ __forceinline__ pieces that stand once:
//   workgroup per sample   rec_*, lstm_*_lds, mgu_*, rnn_* (below): every net the other two do not take.  Pieces: stage8, recCols /
//                          recLdsFloats / recStageWeights / RecWeights (one layout of [W_in; W_rec]), recCopyLayers, RecWin, recLoadParams,
//                          recPreloadStates / recStateOf / recFirstInput, recStoreOperandRow, recBlockOutput, recStoreYout, recZeroRows,
//                          recTopError, recResidualBack, recErrorRows, lstmCellDeltas
//   wavefront per (sample, layer)   two layers of 32 cells (wave32*, lstm32*, mgu32*), alone or as the one-launch step
//   time-step-major        rectm.hip
// Which kernel a net gets is decided in ONE place, recRoute() near the end of this file; rec_route_name() prints it.
#include <cstdio>
#include <string>
#include "head_rows.h"     // (tail_dev.h; the head of the one-launch step: lstm32_step_wave_kernel)
#include "rec_dev.h"

namespace hl {

#define REC_MAXC 64       // cells per layer (4 gates x 64 = 256 threads)
#define REC_MAXIN 256     // inputs of the first layer
#define REC_STATES 4608   // window states kept in LDS (e.g. 18 steps x 256 state components)
// the one-gate-per-thread kernels (rec_*, mgu_*, rnn_*: every shape the specialised ones do not take) loop over gates and cells:
#define REC_GENC 256      // cells per layer there
#define REC_GENIN 1024    // inputs of the first layer there (stacked observations, or the output of a convolutional stack)

// workgroup barrier that orders LDS traffic only: __syncthreads() also waits for the global stores of the step
// (the rows kept for the backward pass / the dW launch), ~1 us each, and nothing in these kernels reads them back
__device__ __forceinline__ void ldsBarrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// End of a kernel prologue: every global load issued so far has landed.  Values fetched once before the step loops (biases,
// residual parameters, state scales) otherwise look "possibly in flight" at the loop head, and the compiler guards each use
// inside the loop with s_waitcnt vmcnt(0) -- which also waits for every row store of the previous layer-step to be acknowledged.
__device__ __forceinline__ void vmDrain() { __builtin_amdgcn_s_waitcnt(0x0F70); }   // vmcnt(0), expcnt / lgkmcnt untouched


// ---- pieces of the workgroup-per-sample kernels (rec_*, lstm_*_lds, mgu_*, rnn_*: every net the specialised kernels further down do
// not take).  Each stands once.  A kernel keeps what is its own: its LDS arrays, its split of the gates over threads, its gate sums and
// cell, and its barriers -- no piece holds an ldsBarrier() or the vmDrain() of the prologue. ----
// copy loop with eight loads in flight per thread, then eight stores (a rolled loop pays one L2 / HBM round trip per element: 50 in a
// row at 32 cells); load(e) / store(e, value) of elements e < total
template <class T, class Load, class Store>
__device__ __forceinline__ void stage8(int total, Load load, Store store) {
  for (int e0 = threadIdx.x; e0 < total; e0 += 256 * 8) {
    T v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u; v[u] = T{}; if (e < total) v[u] = load(e); }
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u; if (e < total) store(e, v[u]); }
  }
}
// Layout of [W_in; W_rec] (rec_*, mgu_*, rnn_*), stated once for the staging loop, the kernels' accessor and the launcher's byte count:
// rows of recCols() floats in global memory (the gate columns; "RNN" layers: the dense layers' pitch roundUp(cells, 8)); the LDS copy
// of all layers pads every row by one float (the forward pass reads columns, the backward pass rows, both conflict-free), layer behind
// layer.  Nets whose copy does not fit read the weights through the L2 (LDSW = 0).
__host__ __device__ __forceinline__ int recCols(int gates, int nC) { return gates == 1 ? (nC + 7) & ~7 : gates * nC; }
// ... floats of a layer in the LDS copy; first float of layer j (j = nL: the size of the copy)
__host__ __device__ __forceinline__ int recLayerFloats(int gates, const RecLayer& L) { return (L.nIn + L.nC) * (recCols(gates, L.nC) + 1); }
__host__ __device__ __forceinline__ int recLdsFloats(const RecArgs& a, int gates, int j) {
  int off = 0;
  for (int q = 0; q < j; ++q) off += recLayerFloats(gates, a.L[q]);
  return off;
}
__device__ __forceinline__ void recStageWeights(const RecArgs& a, int gates, float* sW) {
  int off = 0;
  for (int j = 0; j < a.nL; ++j) {
    const RecLayer& L = a.L[j];
    const int cols = recCols(gates, L.nC);
    const float* src = a.W + L.indW;
    stage8<float>((L.nIn + L.nC) * cols, [&](int e) { return src[e]; },
                  [&](int e, float v) { const int i = e / cols, o = e - i * cols; sW[off + i * (cols + 1) + o] = v; });
    off += recLayerFloats(gates, L);
  }
}
// element (i, o) of layer j's [W_in; W_rec]: the LDS copy or global memory, decided at compile time
template <bool LDSW>
struct RecWeights {
  const float* base; int ld;
  __device__ __forceinline__ RecWeights(const RecArgs& a, const float* sW, int gates, int j, const RecLayer& L)
    : base(LDSW ? sW + recLdsFloats(a, gates, j) : a.W + L.indW), ld(recCols(gates, L.nC) + (LDSW ? 1 : 0)) {}
  __device__ __forceinline__ float operator()(int i, int o) const { if constexpr (LDSW) return base[i * ld + o]; else return base[(size_t)i * ld + o]; }
};
// layer descriptors copied out of the kernel-argument segment once (inside the step loops every field access was a scalar load of its
// own).  LL is indexed inside unrolled loops only: a run-time index puts the whole array on the stack (976 bytes of scratch per lane in
// lstm_backward_lds_kernel<0> until round 5) -- the pieces below take the one layer, or the arrays by reference.
template <int MAXL>
__device__ __forceinline__ void recCopyLayers(const RecArgs& a, RecLayer (&LL)[MAXL]) {
#pragma unroll
  for (int j = 0; j < MAXL; ++j) LL[j] = a.L[j];
}
// Sample b's window: steps t - T .. t and, behind a truncated episode end, step t + 1 (output row nextRow).  Acting (MemoryBuffer::
// agentToMinibatch, MemoryBuffer.cpp:440-467): the agent's last `actWin` steps, from a zero recurrent state.
struct RecWinGeo { int t, T, nextRow, nSteps; long long slot; };
__device__ __forceinline__ RecWinGeo recWindowGeo(const RecArgs& a, int b, bool acting, int actWin) {
  RecWinGeo g;
  g.t = acting ? 0 : a.bt.t[b]; g.slot = acting ? 0 : a.bt.slot[b];
  g.T = acting ? actWin - 1 : min(a.nBPTT, g.t);
  g.nextRow = acting ? -1 : a.bt.nextOf[b];
  g.nSteps = g.T + 1 + (g.nextRow >= 0 ? 1 : 0);
  return g;
}
// ... of workgroup b of the forward kernels (acting: the one agent's window or, MANY, agent b's of the per-agent tables)
template <bool MANY>
struct RecWin : RecWinGeo {
  RecActWin<MANY> aw; bool acting;
  __device__ __forceinline__ RecWin(const RecArgs& a, int b) : aw(a, b), acting(a.actStates != nullptr) { static_cast<RecWinGeo&>(*this) = recWindowGeo(a, b, acting, aw.win(a)); }
};
// this thread's parameters per layer, requested in the prologue (they must land ahead of vmDrain()): the bias of gate column `tid`
// (GATES columns per cell) and the residual weight and bias of cell `tid`; backward: the residual weight alone
template <int GATES, int MAXL>
__device__ __forceinline__ void recLoadParams(const RecArgs& a, int nL, float (&bias)[MAXL], float (&wr)[MAXL], float (&br)[MAXL]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < MAXL; ++j) {
    bias[j] = 0.f; wr[j] = 0.f; br[j] = 0.f;
    if (j < nL) {
      const RecLayer& L = a.L[j];
      if (tid < GATES * L.nC) bias[j] = a.W[L.indB + tid];
      if (L.hasRes && tid < L.resW) { wr[j] = a.W[L.indWr + tid]; br[j] = a.W[L.indBr + tid]; }
    }
  }
}
template <int MAXL>
__device__ __forceinline__ void recLoadResWeights(const RecLayer* L, const float* W, int nL, float (&wr)[MAXL]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < MAXL; ++j) { wr[j] = 0.f; if (j < nL && L[j].hasRes && tid < L[j].resW) wr[j] = W[L[j].indWr + tid]; }
}
// The first layer's input.  plain: a step's input is that step's observed state (no rows of a convolutional stack, no appended
// observations; GENERAL = 0: the kernel is launched for nothing else); preload: the standardised states of the whole window
// (Episode::standardizedState, Episode.h:172-183) sit in sStates, fetched in one round -- where they fit REC_STATES (PRELOAD = 0: the
// kernel has no sStates); otherwise component `tid` of each step is fetched when its step comes, with this thread's mean and scale.
struct RecIn { bool plain, preload; int dIn; float sMean, sScale; };
template <bool GENERAL, bool PRELOAD, bool MANY>
__device__ __forceinline__ RecIn recPreloadStates(const RecArgs& a, const RecWin<MANY>& win, float* sStates) {
  const int tid = threadIdx.x;
  RecIn in; in.dIn = a.L[0].nIn;
  in.plain = !GENERAL || (a.Xin == nullptr && a.nApp == 0);
  in.preload = PRELOAD && in.plain && win.nSteps * a.dS <= REC_STATES;
  if constexpr (PRELOAD) if (in.preload) for (int e = tid; e < win.nSteps * a.dS; e += 256) {
    const int kk = e / a.dS, i = e - kk * a.dS;
    const float raw = win.acting ? win.aw.states(a)[e] : a.rp.S[(size_t)(win.slot - win.T + kk) * a.dS + i];
    sStates[e] = (raw - a.rp.stMean[i]) * a.rp.stScale[i];
  }
  in.sMean = tid < a.dS ? a.rp.stMean[tid] : 0.f; in.sScale = tid < a.dS ? a.rp.stScale[tid] : 1.f;
  return in;
}
// standardised state component `tid` of step k (threads tid < dS)
template <bool MANY>
__device__ __forceinline__ float recStateOf(const RecArgs& a, const RecWin<MANY>& win, const RecIn& in, const float* sStates, int k) {
  const int tid = threadIdx.x;
  if (in.preload) return sStates[k * a.dS + tid];
  const float raw = win.acting ? win.aw.states(a)[(size_t)k * a.dS + tid] : a.rp.S[(size_t)(win.slot - win.T + k) * a.dS + tid];
  return (raw - in.sMean) * in.sScale;
}
// step k's input of the first layer into dst
template <bool MANY>
__device__ __forceinline__ void recFirstInput(const RecArgs& a, const RecWin<MANY>& win, const RecIn& in, const float* sStates, int b, int k, float* dst) {
  const int tid = threadIdx.x;
  if (!in.plain) { for (int e = tid; e < in.dIn; e += 256) dst[e] = recInputAtWin<MANY>(a, win.acting, win.aw, b, win.slot, win.t, win.T, win.nextRow, k, e); }
  else if (tid < a.dS) dst[tid] = recStateOf(a, win, in, sStates, k);
}
// row r of the dW operand [input | previous output] (zero at the window's first step)
__device__ __forceinline__ void recStoreOperandRow(const RecLayer& L, long long r, const float* in, const float* prevOut, int k) {
  const int tid = threadIdx.x;
  for (int i = tid; i < L.nIn; i += 256) L.A[r * L.ldA + i] = in[i];
  if (tid < L.nC) L.A[r * L.ldA + L.nIn + tid] = k > 0 ? prevOut[tid] : 0.f;
}
// ParametricResidualLayer::forward (Layers.h:347-361): the block's output for cell c, whose layer output is `out` and whose block input in[c]
__device__ __forceinline__ float recBlockOutput(const RecLayer& L, float out, const float* in, float wr, float br, int c) {
  float blk = out;
  if (L.hasRes && c < L.resW) blk += in[c] * wr + br;
  return blk;
}
// component c of the last block's output at step k (*v, read where it is stored): the head's input row at the sampled step (k = T) and at the next state (k = T + 1)
// or -- ROWS: the lower segment of a two-type stack -- every step's, as an input row of the segment above
template <bool ROWS, bool MANY>
__device__ __forceinline__ void recStoreYout(const RecArgs& a, const RecWin<MANY>& win, int b, int k, int c, const float* v) {
  if (ROWS && a.YoutRows) {
    const long long ro = k <= win.T ? (long long)b * a.K + k : (long long)a.B * a.K + (win.nextRow - a.B);
    a.YoutRows[ro * a.ldYR + c] = *v;
  } else {
    if (k == win.T) a.Yout[(size_t)b * a.ldY + c] = *v;
    if (k == win.T + 1) a.Yout[(size_t)win.nextRow * a.ldY + c] = *v;
  }
}
// backward: rows of the steps this sample does not have get zero deltas (their stale inputs then add nothing to the gradients)
__device__ __forceinline__ void recZeroRows(const RecArgs& a, int nL, int gates, int b, int T) {
  const int tid = threadIdx.x;
  for (int k = T + 1; k < a.K; ++k) {
    const long long r = (long long)b * a.K + k;
    for (int j = 0; j < nL; ++j) {
      const RecLayer& L = a.L[j];
      for (int o = tid; o < gates * L.nC; o += 256) L.D[r * gates * L.nC + o] = 0.f;
      if (L.hasRes && tid < L.nC) L.Rd[r * L.ldR + tid] = 0.f;
    }
  }
}
// error w.r.t. component c of the last block's output at step k (row r): the head's at the sampled step or -- ROWS -- the upper segment's of every step
template <bool ROWS>
__device__ __forceinline__ float recTopError(const RecArgs& a, int b, long long r, int k, int T, int c) {
  if (ROWS && a.DresRows) return a.DresRows[r * a.ldDR + c];
  return k == T ? a.Dres[(size_t)b * a.ldD + c] : 0.f;
}
// ParametricResidualLayer::backward (Layers.h:363-393): the delta passes to the layer's output, and through w to the block input (threads tid < nC)
__device__ __forceinline__ void recResidualBack(const RecLayer& L, long long r, float eTop, float wr, float* sRes) {
  const int tid = threadIdx.x;
  if (L.hasRes) { L.Rd[r * L.ldR + tid] = eTop; sRes[tid] = tid < L.resW ? eTop * wr : 0.f; }
}
// Layer::backward (Layers.h:123-188): one row of [W_in; W_rec] (nCols delta columns) per group of four lanes, each lane its columns in
// ascending order, quarter sums joined by two shuffles.  Rows 0..nIn-1 give the error of the block below (skipped under the first
// layer), rows nIn.. the error handed to step k - 1.  QUADS: nCols is a multiple of 4 (the four gates of LSTM cells), so all lanes walk
// the same number of columns -- a loop on a scalar counter, unrolled by 8; otherwise a lane's own count, left to the compiler (measured
// on the 24-cell encoder of pomdp_rnn24_mgu2x16_b128_bptt5: unrolled by 8 its six terms per lane all run in the remainder loop, 14.1 -> 14.6 us).
template <bool QUADS, class Weights>
__device__ __forceinline__ void recErrorRows(const RecLayer& L, const Weights& w, int j, int k, int nCols, const float* sD, const float* sRes, float* topBelow, float* recNew) {
  const int tid = threadIdx.x, part = tid & 3, nIn = L.nIn, row0 = j > 0 ? 0 : nIn, nRow = nIn + (k > 0 ? L.nC : 0);
  for (int i0 = row0; i0 < nRow; i0 += 64) {
    const int i = i0 + (tid >> 2);
    float e = 0.f;
    if (i < nRow) {
      if constexpr (QUADS) {
#pragma unroll 8
        for (int u = 0; u < nCols / 4; ++u) { const int o = 4 * u + part; e += w(i, o) * sD[o]; }
      } else for (int o = part; o < nCols; o += 4) e += w(i, o) * sD[o];
    }
    e += __shfl_xor(e, 1, 64); e += __shfl_xor(e, 2, 64);
    if (part == 0 && i < nRow) {
      if (i < nIn) topBelow[i] = (L.hasRes && i < L.resW ? sRes[i] : 0.f) + e;
      else recNew[i - nIn] = e;
    }
  }
}
// LSTMLayer::backward (Layer_LSTM.h:127-165) of cell `tid` at step k (row r): D the error w.r.t. its output, the step's stored
// activations, prevSt the state of step k - 1; deltas into sD and the row of L.D, the state delta and forget gate kept for step k - 1
__device__ __forceinline__ void lstmCellDeltas(const RecLayer& L, long long r, int k, int T, float D, float cellInpt, float IG, float FG, float OG, float co,
                                               float prevSt, float* sD, float* nxtSt, float* nxtF) {
  const int tid = threadIdx.x, nC = L.nC, NO = 4 * nC;
  const float diff = (1.f - co * co) * D;
  const float sd = diff * OG + (k < T ? nxtSt[tid] * nxtF[tid] : 0.f);
  const float d0 = IG * sd;
  const float d1 = IG * (1.f - IG) * cellInpt * sd;
  const float d2 = k > 0 ? FG * (1.f - FG) * prevSt * sd : 0.f;
  const float d3 = OG * (1.f - OG) * D * co;
  sD[tid] = d0; sD[nC + tid] = d1; sD[2 * nC + tid] = d2; sD[3 * nC + tid] = d3;
  L.D[r * NO + tid] = d0; L.D[r * NO + nC + tid] = d1; L.D[r * NO + 2 * nC + tid] = d2; L.D[r * NO + 3 * nC + tid] = d3;
  nxtSt[tid] = sd; nxtF[tid] = FG;
}

#ifdef REC_STAMPS
__device__ unsigned long long recStamps[256];
// stamp i, taken by thread `thread` of the first sample's workgroup (the one-launch step: block 1 behind a rider; thread 0 / 64: its
// wavefront 0 / 1)
#define REC_STAMP(sample, thread, i) do { if ((sample) == 0 && threadIdx.x == (thread) && (i) < 256) recStamps[i] = wall_clock64(); } while (0)
#else
#define REC_STAMP(sample, thread, i) do {} while (0)
#endif
// rec_forward_kernel keeps the body it had before the pieces above were cut out of the other seven kernels: written with them it computes the
// same bits, but its <false, false> form (weights through the L2: an LSTM layer behind convolutions, conv2_lstm32_b64_bptt4 of bench.py) came
// out 2 us per launch slower (97.3 -> 99.3 us; 1362 -> 1473 reloads of spilled scalars in its unrolled eight-layer body), beyond the
// parent's own spread.  It shares the layout (recStageWeights, recLdsFloats) and nothing else.
template <bool LDSW, bool MANY>
__global__ __launch_bounds__(256) void rec_forward_kernel(RecArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sW[];
  __shared__ float sBuf[2][REC_GENIN];                    // input of the current layer / output of the current block
  __shared__ float sPrevOut[HL_MAX_HIDDEN][REC_GENC], sPrevSt[HL_MAX_HIDDEN][REC_GENC];
  __shared__ float sX[4 * REC_GENC];
  const int b = blockIdx.x, tid = threadIdx.x;
  REC_STAMP(blockIdx.x, 0, 0);
  // acting (MemoryBuffer::agentToMinibatch, MemoryBuffer.cpp:440-467): the agent's last steps, from a zero recurrent state
  const bool acting = a.actStates != nullptr;
  const int t = acting ? 0 : a.bt.t[b]; const long long slot = acting ? 0 : a.bt.slot[b];
  const RecActWin<MANY> aw(a, b);      // (acting: the one agent's window or, with the per-agent tables, agent b's)
  const int T = acting ? aw.win(a) - 1 : min(a.nBPTT, t);
  const int nextRow = acting ? -1 : a.bt.nextOf[b];
  const int nSteps = T + 1 + (nextRow >= 0 ? 1 : 0);
  const float* W = a.W;
  // layer descriptors copied out of the kernel-argument segment once (inside the step loops every field access was a scalar
  // load of its own)
  RecLayer LL[HL_MAX_HIDDEN];
#pragma unroll
  for (int j = 0; j < HL_MAX_HIDDEN; ++j) LL[j] = a.L[j];
  REC_STAMP(blockIdx.x, 0, 1);
  if constexpr (LDSW) recStageWeights(a, 4, sW);
  REC_STAMP(blockIdx.x, 0, 2);
  float bias[HL_MAX_HIDDEN], wr[HL_MAX_HIDDEN], br[HL_MAX_HIDDEN];      // this thread's gate bias / residual parameters per layer
#pragma unroll
  for (int j = 0; j < HL_MAX_HIDDEN; ++j) {
    bias[j] = 0.f; wr[j] = 0.f; br[j] = 0.f;
    if (j < a.nL) {
      const RecLayer& L = a.L[j];
      if (tid < 4 * L.nC) bias[j] = W[L.indB + tid];
      if (L.hasRes && tid < L.resW) { wr[j] = W[L.indWr + tid]; br[j] = W[L.indBr + tid]; }
    }
  }
  // the standardised states of the whole window, fetched in one round (Episode::standardizedState, Episode.h:172-183)
  __shared__ float sStates[REC_STATES];
  const int dIn = a.L[0].nIn;
  const bool plain = a.Xin == nullptr && a.nApp == 0;      // the input of a step is that step's observed state
  const bool preload = plain && nSteps * a.dS <= REC_STATES;
  if (preload) for (int e = tid; e < nSteps * a.dS; e += 256) {
    const int kk = e / a.dS, i = e - kk * a.dS;
    const float raw = acting ? aw.states(a)[e] : a.rp.S[(size_t)(slot - T + kk) * a.dS + i];
    sStates[e] = (raw - a.rp.stMean[i]) * a.rp.stScale[i];
  }
  const float sMean = tid < a.dS ? a.rp.stMean[tid] : 0.f, sScale = tid < a.dS ? a.rp.stScale[tid] : 1.f;
  vmDrain(); ldsBarrier();
  REC_STAMP(blockIdx.x, 0, 3);
  for (int k = 0; k < nSteps; ++k) {
    const bool store = !acting && k <= T;
    const long long r = (long long)b * a.K + k;
    const long long sl = slot - T + k;
    if (!plain) { for (int e = tid; e < dIn; e += 256) sBuf[0][e] = recInputAtWin<MANY>(a, acting, aw, b, slot, t, T, nextRow, k, e); }
    else if (tid < a.dS) {
      if (preload) sBuf[0][tid] = sStates[k * a.dS + tid];
      else { const float raw = acting ? aw.states(a)[(size_t)k * a.dS + tid] : a.rp.S[(size_t)sl * a.dS + tid]; sBuf[0][tid] = (raw - sMean) * sScale; }
    }
    ldsBarrier();
    REC_STAMP(blockIdx.x, 0, 4 + k * 5);
    int cur = 0;
#pragma unroll
    for (int j = 0; j < HL_MAX_HIDDEN; ++j) if (j < a.nL) {
      const RecLayer& L = LL[j];
      const int nIn = L.nIn, nC = L.nC, NO = 4 * nC;
      const float* in = sBuf[cur];
      // element (i, o) of [W_in; W_rec] of this layer: LDS copy (padded rows) or global memory, decided at compile time
      const int ldw = LDSW ? NO + 1 : NO, wOff = LDSW ? recLdsFloats(a, 4, j) : 0;
      const float* gWj = W + L.indW;
      auto wAt = [&](int i, int o) -> float { if constexpr (LDSW) return sW[wOff + i * ldw + o]; else return gWj[(size_t)i * ldw + o]; };
      if (store) {
        for (int i = tid; i < nIn; i += 256) L.A[r * L.ldA + i] = in[i];
        if (tid < nC) L.A[r * L.ldA + nIn + tid] = k > 0 ? sPrevOut[j][tid] : 0.f;
      }
      for (int o = tid; o < NO; o += 256) {                // (one gate per thread up to 64 cells, four at 256)
        float acc = o == tid ? bias[j] : W[L.indB + o];
        // (unrolled: the LDS reads of eight terms are in flight together; a rolled loop pays the LDS latency per term)
#pragma unroll 8
        for (int i = 0; i < nIn; ++i) acc += in[i] * wAt(i, o);
        if (k > 0) {
#pragma unroll 8
          for (int i = 0; i < nC; ++i) acc += sPrevOut[j][i] * wAt(nIn + i, o);
        }
        if (o >= nC) acc = recSigm(acc);                   // the gates overwrite their inputs
        sX[o] = acc;
        if (store) L.X[r * NO + o] = acc;
      }
      ldsBarrier();
      if (j < 2) REC_STAMP(blockIdx.x, 0, 4 + k * 5 + 1 + 2 * j);
      float out = 0.f, st = 0.f;
      if (tid < nC) {
        st = sX[tid] * sX[nC + tid] + (k > 0 ? sPrevSt[j][tid] * sX[2 * nC + tid] : 0.f);
        const float co = actEval(HL_FUNC_TANH, st);
        out = sX[3 * nC + tid] * co;
        if (store) { L.Y[r * NO + tid] = out; L.Y[r * NO + nC + tid] = st; L.Y[r * NO + 2 * nC + tid] = co; }
        float blk = out;                                   // ParametricResidualLayer::forward (Layers.h:347-361)
        if (L.hasRes && tid < L.resW) blk += in[tid] * wr[j] + br[j];
        sBuf[cur ^ 1][tid] = blk;
      }
      ldsBarrier();
      if (j < 2) REC_STAMP(blockIdx.x, 0, 4 + k * 5 + 2 + 2 * j);
      if (tid < nC) { sPrevOut[j][tid] = out; sPrevSt[j][tid] = st; }
      cur ^= 1;
    }
    const int nCl = a.L[a.nL - 1].nC;
    if (k == T && tid < nCl) a.Yout[(size_t)b * a.ldY + tid] = sBuf[cur][tid];
    if (k == T + 1 && tid < nCl) a.Yout[(size_t)nextRow * a.ldY + tid] = sBuf[cur][tid];
    ldsBarrier();
  }
  REC_STAMP(blockIdx.x, 0, 250);
}

// ---- LSTM forward, weights resident in LDS: the version the step uses whenever they fit --------------------------------
// Measured on the kernel above (device time stamps, 2 x 32 cells): a layer-step cost 1.1-1.3 us for the gate sums -- one
// thread per gate walking 36 / 64 terms, eight LDS reads in flight at a time, 0.11 us per batch of eight -- 0.4 us for the
// cell update behind a barrier of its own, and 0.5 us of per-step barriers.  Here
//   * the weights sit TRANSPOSED in LDS, one row per gate: [W_in column (padded to 4) | W_rec column (padded to 4) | bias,0,0,0]
//     with a row pitch whose quarter is odd, so that ds_read_b128 of 16 neighbouring gates touch all 64 banks once;
//   * the operand is ONE vector per layer, [input | previous output | 1,0,0,0], double-buffered over the steps (this step's
//     output goes into the other copy), which is also exactly the row stored for the weight-gradient contraction;
//   * P = 8 / 4 / 2 / 1 lanes share a gate (<= 8 / 16 / 32 / 64 cells), each lane reads four 16-byte chunks per round with all
//     eight reads in flight, partial sums joined by shuffles;
//   * the four gates of a cell sit in neighbouring lanes, so the cell update gathers them by shuffles instead of LDS + barrier:
//     ONE barrier per layer-step, none per step (the next step's state is written into the idle copy during the step).
// Sums are formed in a different order than in the oracle (four partial sums per lane, bias last): 1e-7-level differences.
// layout of a layer's transposed copy: padded input / recurrent parts, floats per gate row, row pitch, floats of the layer
struct LstmGeo { int inPad, recPad, nT, ld, floats; };
__host__ __device__ __forceinline__ LstmGeo lstmGeo(int nIn, int nC) {
  LstmGeo g; g.inPad = (nIn + 3) & ~3; g.recPad = (nC + 3) & ~3; g.nT = g.inPad + g.recPad + 4;
  g.ld = ((g.nT >> 2) & 1) ? g.nT : g.nT + 4; g.floats = 4 * nC * g.ld;
  return g;
}
#define LSTM_VEC (REC_MAXIN + REC_MAXC + 8)
// NL / NC: number of layers / cells of every layer known at compile time (0: read from the arguments) -- with the general
// eight-layer body the loop invariants alone are 450 spilled scalars and each layer-step some 600 instructions
template <int NL, int NC, bool MANY>
__global__ __launch_bounds__(256) void lstm_forward_lds_kernel(RecArgs a) {
  constexpr int MAXL = NL ? NL : HL_MAX_HIDDEN;
  const int nL = NL ? NL : a.nL;
  extern __shared__ __attribute__((aligned(16))) float sW[];
  __shared__ __attribute__((aligned(16))) float sA[HL_MAX_HIDDEN][2][LSTM_VEC];
  __shared__ float sStates[REC_STATES];
  const int b = blockIdx.x, tid = threadIdx.x;
  REC_STAMP(blockIdx.x, 0, 0);
  const RecWin<MANY> win(a, b);
  const float* W = a.W;
  RecLayer LL[MAXL];
  recCopyLayers(a, LL);
  REC_STAMP(blockIdx.x, 0, 1);
  // weights, transposed (coalesced 16-byte global reads along the gates of one input row, scattered LDS writes)
  {
    int off = 0;
    for (int j = 0; j < nL; ++j) {
      const RecLayer& L = a.L[j];
      const int nIn = L.nIn, nC = NC ? NC : L.nC, NO = 4 * nC, q4 = nC;          // q4: float4 per row (NO / 4)
      const LstmGeo g = lstmGeo(nIn, nC);
      const float4* src = reinterpret_cast<const float4*>(W + L.indW);                  // (indW is a multiple of 4: checked by the launcher)
      stage8<float4>((nIn + nC) * q4, [&](int e) { return src[e]; }, [&](int e, const float4& v) {
        const int i = e / q4, o = 4 * (e - i * q4), ti = i < nIn ? i : g.inPad + (i - nIn);
        float* d = sW + off + o * g.ld + ti;
        d[0] = v.x; d[g.ld] = v.y; d[2 * g.ld] = v.z; d[3 * g.ld] = v.w;
      });
      for (int o = tid; o < NO; o += 256) {
        float* d = sW + off + o * g.ld;
        for (int i = nIn; i < g.inPad; ++i) d[i] = 0.f;
        for (int i = g.inPad + nC; i < g.inPad + g.recPad; ++i) d[i] = 0.f;
        d[g.nT - 4] = W[L.indB + o]; d[g.nT - 3] = 0.f; d[g.nT - 2] = 0.f; d[g.nT - 1] = 0.f;
      }
      for (int i = tid; i < 2 * LSTM_VEC; i += 256) {                                  // operand vectors: zero, then the constant 1
        const int c = i / LSTM_VEC, e = i - c * LSTM_VEC;
        sA[j][c][e] = e == g.nT - 4 ? 1.f : 0.f;
      }
      off += g.floats;
    }
  }
  REC_STAMP(blockIdx.x, 0, 2);
  // this thread's role per layer: cell, gate, part; the parameters of its cell
  float wr[MAXL], br[MAXL], prevSt[MAXL];
#pragma unroll
  for (int j = 0; j < MAXL; ++j) {
    wr[j] = 0.f; br[j] = 0.f; prevSt[j] = 0.f;
    if (j < nL) {
      const RecLayer& L = a.L[j];
      const int nCj = NC ? NC : L.nC;
      const int P = nCj <= 8 ? 8 : (nCj <= 16 ? 4 : (nCj <= 32 ? 2 : 1)), c = tid / (4 * P);
      if (L.hasRes && c < L.resW && c < nCj) { wr[j] = W[L.indWr + c]; br[j] = W[L.indBr + c]; }
    }
  }
  const RecIn in0 = recPreloadStates<false, true>(a, win, sStates);
  vmDrain(); ldsBarrier();
  if (tid < a.dS) sA[0][0][tid] = recStateOf(a, win, in0, sStates, 0);
  ldsBarrier();
  REC_STAMP(blockIdx.x, 0, 3);
  for (int k = 0; k < win.nSteps; ++k) {
    const bool store = !win.acting && k <= win.T;
    const long long r = (long long)b * a.K + k;
    const int cb = k & 1;
    if (k + 1 < win.nSteps && tid < a.dS) sA[0][cb ^ 1][tid] = recStateOf(a, win, in0, sStates, k + 1);   // (that copy was last read a step ago)
    REC_STAMP(blockIdx.x, 0, 4 + k * 5);
    int off = 0;
#pragma unroll
    for (int j = 0; j < MAXL; ++j) if (j < nL) {
      const RecLayer& L = LL[j];
      const int nIn = (NC && j > 0) ? NC : L.nIn, nC = NC ? NC : L.nC, NO = 4 * nC;
      const LstmGeo g = lstmGeo(nIn, nC);
      const int P = nC <= 8 ? 8 : (nC <= 16 ? 4 : (nC <= 32 ? 2 : 1)), G = 4 * P;
      const int c = tid / G, gate = (tid & (G - 1)) / P, part = tid & (P - 1), o = gate * nC + c;
      const float* vec = sA[j][cb];
      if (store) {
        if (tid < nIn + nC) L.A[r * L.ldA + tid] = vec[tid < nIn ? tid : g.inPad + (tid - nIn)];   // (nIn + nC <= 256 + 64: second round below)
        if (tid + 256 < nIn + nC) L.A[r * L.ldA + tid + 256] = vec[tid + 256 < nIn ? tid + 256 : g.inPad + (tid + 256 - nIn)];
      }
      float acc = 0.f;
      if (c < nC) {
        const float4* row4 = reinterpret_cast<const float4*>(sW + off + o * g.ld);
        const float4* vec4 = reinterpret_cast<const float4*>(vec);
        // the bias chunk [b,0,0,0] x [1,0,0,0] is taken as one scalar (lane part 0), so that 64 terms are exactly eight chunks
        // per lane at two lanes per gate: ONE round of sixteen 16-byte reads in flight
        const int nCh = (g.nT >> 2) - 1;
        float p0 = part == 0 ? (sW + off + o * g.ld)[g.nT - 4] : 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
        for (int c0 = part; c0 < nCh; c0 += 8 * P) {
          float4 w[8], x[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int ch = c0 + u * P, cc = ch < nCh ? ch : part;
            w[u] = row4[cc]; x[u] = vec4[cc];
            if (ch >= nCh) w[u] = make_float4(0.f, 0.f, 0.f, 0.f);
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) { p0 += w[u].x * x[u].x; p1 += w[u].y * x[u].y; p2 += w[u].z * x[u].z; p3 += w[u].w * x[u].w; }
        }
        acc = (p0 + p1) + (p2 + p3);
      }
      if (P > 1) acc += __shfl_xor(acc, 1, 64);
      if (P > 2) acc += __shfl_xor(acc, 2, 64);
      if (P > 4) acc += __shfl_xor(acc, 4, 64);
      if (gate > 0) acc = recSigm(acc);                    // the gates overwrite their inputs
      if (store && part == 0 && c < nC) L.X[r * NO + o] = acc;
      const int base = (tid & 63) & ~(G - 1);
      const float x0 = __shfl(acc, base, 64), x1 = __shfl(acc, base + P, 64), x2 = __shfl(acc, base + 2 * P, 64), x3 = __shfl(acc, base + 3 * P, 64);
      if ((tid & (G - 1)) == 0 && c < nC) {
        const float st = x0 * x1 + prevSt[j] * x2;          // (prevSt is 0 at the first step of the window)
        const float co = actEval(HL_FUNC_TANH, st);
        const float out = x3 * co;
        prevSt[j] = st;
        if (store) { L.Y[r * NO + c] = out; L.Y[r * NO + nC + c] = st; L.Y[r * NO + 2 * nC + c] = co; }
        const float blk = recBlockOutput(L, out, vec, wr[j], br[j], c);
        sA[j][cb ^ 1][g.inPad + c] = out;                  // recurrent input of the next step
        if (j + 1 < nL) sA[j + 1][cb][c] = blk;
        else recStoreYout<false>(a, win, b, k, c, &blk);
      }
      ldsBarrier();
      if (j < 2) REC_STAMP(blockIdx.x, 0, 4 + k * 5 + 2 + 2 * j);
      off += g.floats;
    }
  }
  REC_STAMP(blockIdx.x, 0, 250);
}

template <bool LDSW>
__global__ __launch_bounds__(256) void rec_backward_kernel(RecArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sW[];
  __shared__ float sTop[2][REC_GENIN];                    // error w.r.t. the output of the current block (from above, same step)
  __shared__ float sRec[HL_MAX_HIDDEN][REC_GENC];          // error w.r.t. this step's LSTM output coming from step k+1
  __shared__ float sNxtSt[HL_MAX_HIDDEN][REC_GENC], sNxtF[HL_MAX_HIDDEN][REC_GENC];
  __shared__ float sD[4 * REC_GENC], sRes[REC_GENC], sRecNew[REC_GENC];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = min(a.nBPTT, a.bt.t[b]);
  RecLayer LL[HL_MAX_HIDDEN];
  recCopyLayers(a, LL);
  if constexpr (LDSW) recStageWeights(a, 4, sW);
  float wr[HL_MAX_HIDDEN];
  recLoadResWeights(a.L, a.W, a.nL, wr);
  vmDrain(); ldsBarrier();
  recZeroRows(a, a.nL, 4, b, T);
  for (int k = T; k >= 0; --k) {
    const long long r = (long long)b * a.K + k;
    int cur = 0;
    if (tid < a.L[a.nL - 1].nC) sTop[0][tid] = recTopError<false>(a, b, r, k, T, tid);
    // this step's stored activations of every layer, fetched in one round
    float vCo[HL_MAX_HIDDEN], vCi[HL_MAX_HIDDEN], vIG[HL_MAX_HIDDEN], vFG[HL_MAX_HIDDEN], vOG[HL_MAX_HIDDEN], vPs[HL_MAX_HIDDEN];
#pragma unroll
    for (int j = 0; j < HL_MAX_HIDDEN; ++j) {
      vCo[j] = vCi[j] = vIG[j] = vFG[j] = vOG[j] = vPs[j] = 0.f;
      if (j < a.nL && tid < a.L[j].nC) {
        const RecLayer& L = a.L[j]; const int nC = L.nC, NO = 4 * nC;
        vCo[j] = L.Y[r * NO + 2 * nC + tid]; vCi[j] = L.X[r * NO + tid]; vIG[j] = L.X[r * NO + nC + tid];
        vFG[j] = L.X[r * NO + 2 * nC + tid]; vOG[j] = L.X[r * NO + 3 * nC + tid];
        if (k > 0) vPs[j] = L.Y[(r - 1) * NO + nC + tid];
      }
    }
    ldsBarrier();
#pragma unroll
    for (int j = HL_MAX_HIDDEN - 1; j >= 0; --j) if (j < a.nL) {
      const RecLayer& L = LL[j];
      const RecWeights<LDSW> w(a, sW, 4, j, L);
      if (tid < L.nC) {
        const float eTop = sTop[cur][tid];
        recResidualBack(L, r, eTop, wr[j], sRes);
        const float D = eTop + (k < T ? sRec[j][tid] : 0.f);
        lstmCellDeltas(L, r, k, T, D, vCi[j], vIG[j], vFG[j], vOG[j], vCo[j], vPs[j], sD, sNxtSt[j], sNxtF[j]);
      }
      ldsBarrier();
      recErrorRows<true>(L, w, j, k, 4 * L.nC, sD, sRes, sTop[cur ^ 1], sRecNew);
      ldsBarrier();
      if (tid < L.nC) sRec[j][tid] = k > 0 ? sRecNew[tid] : 0.f;
      cur ^= 1;
    }
    ldsBarrier();
  }
}

// ---- LSTM back-propagation through the window, weights AND the window's stored activations resident in LDS ----------------
// Same findings as for the forward kernel; in addition the per-step reads of the stored gates sat behind the acknowledgement
// of the previous step's delta stores (one in-order memory counter).  Here the gates and states of the whole window are
// fetched once into LDS, so the step loop only stores; [W_in; W_rec] rows have a pitch of 16 (mod 64) floats so that the
// 16-byte reads of four rows x four lanes touch every bank once; two barriers per layer-step instead of three.
// layout: per layer its rows at lstmBwdPitch(), layer behind layer; behind them, per step, 6 floats per cell of every layer
__host__ __device__ __forceinline__ int lstmBwdPitch(int NO) { return NO + ((16 - NO % 64) + 64) % 64; }
__host__ __device__ __forceinline__ int lstmBwdFloats(int nIn, int nC) { return (nIn + nC) * lstmBwdPitch(4 * nC); }
__host__ __device__ __forceinline__ int lstmBwdActFloats(int nC) { return 6 * nC; }
template <int NL>
__global__ __launch_bounds__(256) void lstm_backward_lds_kernel(RecArgs a) {
  constexpr int MAXL = NL ? NL : HL_MAX_HIDDEN;
  const int nL = NL ? NL : a.nL;
  extern __shared__ __attribute__((aligned(16))) float sW[];
  __shared__ float sTop[2][REC_MAXIN];                    // error w.r.t. the output of the current block (from above, same step)
  __shared__ float sRec[MAXL][REC_MAXC];                   // error w.r.t. this step's LSTM output coming from step k+1
  __shared__ float sNxtSt[MAXL][REC_MAXC], sNxtF[MAXL][REC_MAXC];
  __shared__ __attribute__((aligned(16))) float sD[4 * REC_MAXC];
  __shared__ float sRes[REC_MAXC];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = min(a.nBPTT, a.bt.t[b]);
  RecLayer LL[MAXL];
  recCopyLayers(a, LL);
  // weights: rows of [W_in; W_rec] as in global memory, padded pitch
  int wOffs[MAXL], aOffs[MAXL];
  int off = 0, actPitch = 0;
#pragma unroll
  for (int j = 0; j < MAXL; ++j) {
    wOffs[j] = off; aOffs[j] = actPitch;
    if (j < nL) {
      const RecLayer& L = LL[j];
      const int nC = L.nC, ldb = lstmBwdPitch(4 * nC);
      const float4* src = reinterpret_cast<const float4*>(a.W + L.indW);
      stage8<float4>((L.nIn + nC) * nC, [&](int e) { return src[e]; },
                     [&](int e, const float4& v) { const int i = e / nC, q = e - i * nC; *reinterpret_cast<float4*>(sW + off + i * ldb + 4 * q) = v; });
      off += lstmBwdFloats(L.nIn, nC); actPitch += lstmBwdActFloats(nC);
    }
  }
  // stored activations of the window, per (step, layer): [cell input | input, forget, output gate | state | tanh(state)]
  float* sAct = sW + off;
  stage8<float>((T + 1) * actPitch, [&](int e) {
    const int k = e / actPitch, q = e - k * actPitch;
    const long long r = (long long)b * a.K + k;
    const float* p = nullptr;
#pragma unroll
    for (int j = 0; j < MAXL; ++j) if (j < nL && q >= aOffs[j] && q < aOffs[j] + 6 * LL[j].nC) {
      const int x = q - aOffs[j], nC = LL[j].nC;
      p = x < 4 * nC ? LL[j].X + r * 4 * nC + x : LL[j].Y + r * 4 * nC + nC + (x - 4 * nC);
    }
    return *p;
  }, [&](int e, float v) { sAct[e] = v; });
  float wr[MAXL];
  recLoadResWeights(LL, a.W, nL, wr);
  const int nCl = a.L[nL - 1].nC;      // (from the arguments: a run-time index into LL would put the whole array on the stack)
  const float dres = tid < nCl ? recTopError<false>(a, b, 0, T, T, tid) : 0.f;
  vmDrain(); ldsBarrier();
  recZeroRows(a, nL, 4, b, T);
  for (int k = T; k >= 0; --k) {
    const long long r = (long long)b * a.K + k;
    int cur = 0;
    if (tid < nCl) sTop[0][tid] = k == T ? dres : 0.f;
    ldsBarrier();
#pragma unroll
    for (int j = MAXL - 1; j >= 0; --j) if (j < nL) {
      const RecLayer& L = LL[j];
      const int nIn = L.nIn, nC = L.nC, ldb = lstmBwdPitch(4 * nC);
      if (tid < nC) {
        const float* act = sAct + k * actPitch + aOffs[j];
        const float eTop = sTop[cur][tid];
        recResidualBack(L, r, eTop, wr[j], sRes);
        const float D = eTop + (k < T ? sRec[j][tid] : 0.f);
        lstmCellDeltas(L, r, k, T, D, act[tid], act[nC + tid], act[2 * nC + tid], act[3 * nC + tid], act[5 * nC + tid],
                       k > 0 ? (act - actPitch)[4 * nC + tid] : 0.f, sD, sNxtSt[j], sNxtF[j]);
      }
      ldsBarrier();
      // Layer::backward (Layers.h:123-188): one row of [W_in; W_rec] per group of four lanes, 16-byte chunks of the row and of
      // the deltas, eight of each in flight per lane; rows 0..nIn-1 give the error of the block below (skipped under the first
      // layer), rows nIn.. the error handed to the previous step
      {
        const int part = tid & 3, row0 = j > 0 ? 0 : nIn, nRow = nIn + (k > 0 ? nC : 0), nCh = nC;
        const float4* d4 = reinterpret_cast<const float4*>(sD);
        for (int i0 = row0; i0 < nRow; i0 += 64) {
          const int i = i0 + (tid >> 2);
          float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
          if (i < nRow) {
            const float4* row4 = reinterpret_cast<const float4*>(sW + wOffs[j] + i * ldb);
            for (int u0 = 0; u0 < nCh; u0 += 32) {
              float4 w[8], d[8];
#pragma unroll
              for (int u = 0; u < 8; ++u) {
                const int ch = u0 + part + 4 * u, cc = ch < nCh ? ch : part;
                w[u] = row4[cc]; d[u] = d4[cc];
                if (ch >= nCh) w[u] = make_float4(0.f, 0.f, 0.f, 0.f);
              }
#pragma unroll
              for (int u = 0; u < 8; ++u) { p0 += w[u].x * d[u].x; p1 += w[u].y * d[u].y; p2 += w[u].z * d[u].z; p3 += w[u].w * d[u].w; }
            }
          }
          float e = (p0 + p1) + (p2 + p3);
          e += __shfl_xor(e, 1, 64); e += __shfl_xor(e, 2, 64);
          if (part == 0 && i < nRow) {
            if (i < nIn) sTop[cur ^ 1][i] = (L.hasRes && i < L.resW ? sRes[i] : 0.f) + e;
            else sRec[j][i - nIn] = e;                       // (read above, before the barrier; not used at k == 0)
          }
        }
      }
      ldsBarrier();
      cur ^= 1;
    }
  }
}

// ---- MGU layers (Network/Layers/Layer_GRU.h): forget = sigm(Wff in + Wfr prevOut + bf), state = tanh(Wsf in + Wsr (forget * prevOut)
// + bs), output = forget * state + (1 - forget) * prevOut.  Same structure as the LSTM kernels: one workgroup per sample. ----
template <bool LDSW, int NL, bool MANY>
__global__ __launch_bounds__(256) void mgu_forward_kernel(RecArgs a) {
  constexpr int MAXL = NL ? NL : HL_MAX_HIDDEN;
  const int nL = NL ? NL : a.nL;
  extern __shared__ __attribute__((aligned(16))) float sW[];
  __shared__ float sBuf[2][REC_GENIN];
  __shared__ float sPrevOut[MAXL][REC_GENC];
  __shared__ float sF[REC_GENC], sS[REC_GENC];
  __shared__ float sStates[REC_STATES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const RecWin<MANY> win(a, b);
  const float* W = a.W;
  RecLayer LL[MAXL];
  recCopyLayers(a, LL);
  if constexpr (LDSW) recStageWeights(a, 2, sW);
  float bias[MAXL], wr[MAXL], br[MAXL];
  recLoadParams<2>(a, nL, bias, wr, br);
  const RecIn in0 = recPreloadStates<true, true>(a, win, sStates);
  vmDrain(); ldsBarrier();
  for (int k = 0; k < win.nSteps; ++k) {
    const bool store = !win.acting && k <= win.T;
    const long long r = (long long)b * a.K + k;
    recFirstInput(a, win, in0, sStates, b, k, sBuf[0]);
    ldsBarrier();
    int cur = 0;
#pragma unroll
    for (int j = 0; j < MAXL; ++j) if (j < nL) {
      const RecLayer& L = LL[j];
      const int nIn = L.nIn, nC = L.nC, NO = 2 * nC;
      const float* in = sBuf[cur];
      const RecWeights<LDSW> w(a, sW, 2, j, L);
      if (store) recStoreOperandRow(L, r, in, sPrevOut[j], k);
      // (one gate per thread up to 128 cells, two at 256; the state gates' input sums wait in sS for the forget gates)
      for (int o = tid; o < NO; o += 256) {
        float acc = o == tid ? bias[j] : W[L.indB + o];
#pragma unroll 8
        for (int i = 0; i < nIn; ++i) acc += in[i] * w(i, o);
        if (o < nC) {          // forget gate
          if (k > 0) {
#pragma unroll 8
            for (int i = 0; i < nC; ++i) acc += w(nIn + i, o) * sPrevOut[j][i];
          }
          acc = recSigm(acc);
          sF[o] = acc;
          if (store) L.X[r * NO + o] = acc;
        } else sS[o - nC] = acc;
      }
      ldsBarrier();
      for (int o = nC + tid; o < NO; o += 256) {   // cell state
        float acc = sS[o - nC];
        if (k > 0) {
#pragma unroll 8
          for (int i = 0; i < nC; ++i) acc += w(nIn + i, o) * sPrevOut[j][i] * sF[i];
        }
        acc = actEval(HL_FUNC_TANH, acc);
        sS[o - nC] = acc;
        if (store) L.X[r * NO + o] = acc;
      }
      ldsBarrier();
      float out = 0.f;
      if (tid < nC) {
        const float f = sF[tid], st = sS[tid], po = k > 0 ? sPrevOut[j][tid] : 0.f;
        out = k > 0 ? f * st + (1.f - f) * po : f * st;
        if (store) { L.Y[r * NO + tid] = out; L.A2[r * L.ldA2 + tid] = po * f; }
        sBuf[cur ^ 1][tid] = recBlockOutput(L, out, in, wr[j], br[j], tid);
      }
      ldsBarrier();
      if (tid < nC) sPrevOut[j][tid] = out;
      cur ^= 1;
    }
    if (tid < a.L[nL - 1].nC) recStoreYout<false>(a, win, b, k, tid, &sBuf[cur][tid]);
    ldsBarrier();
  }
}

template <bool LDSW, int NL>
__global__ __launch_bounds__(256) void mgu_backward_kernel(RecArgs a) {
  constexpr int MAXL = NL ? NL : HL_MAX_HIDDEN;
  const int nL = NL ? NL : a.nL;
  extern __shared__ __attribute__((aligned(16))) float sW[];
  __shared__ float sTop[2][REC_GENIN];
  __shared__ float sRec[MAXL][REC_GENC];          // dLdprevOut handed from step k+1 to step k
  __shared__ float sDF[REC_GENC], sDS[REC_GENC], sFP[REC_GENC], sRes[REC_GENC];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = min(a.nBPTT, a.bt.t[b]);
  RecLayer LL[MAXL];
  recCopyLayers(a, LL);
  if constexpr (LDSW) recStageWeights(a, 2, sW);
  float wr[MAXL];
  recLoadResWeights(a.L, a.W, nL, wr);
  vmDrain(); ldsBarrier();
  recZeroRows(a, nL, 2, b, T);
  for (int k = T; k >= 0; --k) {
    const long long r = (long long)b * a.K + k;
    int cur = 0;
    if (tid < a.L[nL - 1].nC) sTop[0][tid] = recTopError<false>(a, b, r, k, T, tid);
    float vF[MAXL], vS[MAXL], vP[MAXL];
#pragma unroll
    for (int j = 0; j < MAXL; ++j) {
      vF[j] = vS[j] = vP[j] = 0.f;
      if (j < nL && tid < a.L[j].nC) {
        const RecLayer& L = a.L[j]; const int nC = L.nC, NO = 2 * nC;
        vF[j] = L.X[r * NO + tid]; vS[j] = L.X[r * NO + nC + tid];
        if (k > 0) vP[j] = L.Y[(r - 1) * NO + tid];
      }
    }
    ldsBarrier();
#pragma unroll
    for (int j = MAXL - 1; j >= 0; --j) if (j < nL) {
      const RecLayer& L = LL[j];
      const int nIn = L.nIn, nC = L.nC, NO = 2 * nC;
      const RecWeights<LDSW> w(a, sW, 2, j, L);
      float dLdO = 0.f;
      if (tid < nC) {
        const float eTop = sTop[cur][tid];
        recResidualBack(L, r, eTop, wr[j], sRes);
        dLdO = eTop + (k < T ? sRec[j][tid] : 0.f);
        sDS[tid] = dLdO * vF[j] * (1.f - vS[j] * vS[j]);                         // 1) dLdS
      }
      ldsBarrier();
      float fp = 0.f;
      if (tid < nC && k > 0) {                                                   // 2) dLdFprevOut = Wsr dLdS
#pragma unroll 8
        for (int o = 0; o < nC; ++o) fp += w(nIn + tid, nC + o) * sDS[o];
      }
      if (tid < nC) {
        sFP[tid] = fp;
        sDF[tid] = ((vS[j] - vP[j]) * dLdO + fp * vP[j]) * vF[j] * (1.f - vF[j]);   // 3) dLdF
        L.D[r * NO + tid] = sDF[tid]; L.D[r * NO + nC + tid] = sDS[tid];
      }
      ldsBarrier();
      // backprop to the block input: Wff dLdF + Wsf dLdS (+ the residual path); not below the first layer
      if (j > 0) for (int i = tid; i < nIn; i += 256) {
        float e1 = 0.f, e2 = 0.f;
#pragma unroll 8
        for (int o = 0; o < nC; ++o) { e1 += w(i, o) * sDF[o]; e2 += w(i, nC + o) * sDS[o]; }
        sTop[cur ^ 1][i] = ((L.hasRes && i < L.resW ? sRes[i] : 0.f) + e1) + e2;
      }
      float rec = 0.f;
      if (k > 0 && tid < nC) {                                                   // 4) dLdprevOut
        rec = (1.f - vF[j]) * dLdO + vF[j] * sFP[tid];
        float g = 0.f;
#pragma unroll 8
        for (int o = 0; o < nC; ++o) g += w(nIn + tid, o) * sDF[o];
        rec += g;
      }
      ldsBarrier();
      if (tid < nC) sRec[j][tid] = rec;
      cur ^= 1;
    }
    ldsBarrier();
  }
}


// ---- LSTM, two layers of 32 cells (settings/RACER_RNN.json): ONE WAVEFRONT PER (SAMPLE, LAYER), weights in registers ----------
// The kernels above spend a layer-step (128 gates x 64 terms = 8 k multiply-adds) mostly on LDS round trips for weights and
// operand, cross-lane joins and workgroup barriers: ~1.1 us, 38 + 41 us per window forward + BPTT.  Here a workgroup of two
// wavefronts owns a sample, one wavefront per layer:
//   forward   lane l of a layer's wavefront holds the two gate columns l and l + 64 of [W_in; W_rec] in registers; the operand
//             [input | previous output] lives in LDS and is read as broadcast 16-byte chunks; the two dot products of a lane
//             run as packed fp32 FMAs on four independent accumulators, no cross-lane join; the four gates of a cell meet
//             through one 32-lane shuffle.  Layer 0 never depends on layer 1, so its wavefront runs one step AHEAD: at
//             iteration i the first works on step i, the second on step i - 1 (software pipeline, one barrier per iteration).
//   backward  lane i holds ROW i of [W_in; W_rec] (128 values), the 128 gate deltas of the layer-step are broadcast from LDS.
//             Here the TOP layer never depends on the one below, so its wavefront runs one step ahead (k = T - i).
// Sigmoid / tanh use the hardware exponential and reciprocal (v_exp_f32, v_rcp_f32 + one Newton step: ~1e-7 relative, inside
// the tolerance these layers are tested to); the kernels above keep libm's.  Rows written for the weight-gradient launch
// are the same as those of the kernels above.
typedef float f32x2 __attribute__((ext_vector_type(2)));
// lanes 0..31 receive the value lane + 32 holds: one v_permlane32_swap (gfx950) instead of a trip through the LDS crossbar
// (ds_bpermute).  What lanes 32..63 receive is not used by any caller.
__device__ __forceinline__ float fromUpperHalf(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[1]);
}
__device__ __forceinline__ void waveLdsSync() { __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_s_waitcnt(0xC07F); __builtin_amdgcn_wave_barrier(); }
__device__ __forceinline__ float fastRcp(float d) { float r = __builtin_amdgcn_rcpf(d); return fmaf(fmaf(-d, r, 1.0f), r, r); }
__device__ __forceinline__ float fastSigm(float in) {      // Sigm::_eval with safeExp cut at 8, one exponential for both branches
  const float ex = __expf(fmaxf(-8.f, -fabsf(in))), r = fastRcp(1.f + ex);
  return in > 0.f ? r : ex * r;
}
__device__ __forceinline__ float fastTanh(float in) {      // Tanh::_eval (Functions.h:104-113)
  const float e = __expf(-2.f * fabsf(in)), y = (1.f - e) * fastRcp(1.f + e);
  return in > 0.f ? y : -y;
}

// one layer-step: the two gates of this lane (NT terms each, operand broadcast from LDS), cell update on lanes 0..31, the
// rows kept for the backward pass / the weight gradients
// (LDSACT: gates, state and tanh(state) of the step go to `actRow` in LDS -- the one-launch step keeps them for its own backward pass)
template <int NT, bool LDSACT = false>
__device__ __forceinline__ void lstm32LayerStep(const RecLayer& L, const f32x2 (&w)[NT], f32x2 bias, const float* vec, int inPad, int nInL,
                                                float& prevSt, float wr, float br, float* hNext, float& blkOut, bool store, long long r, int lane,
                                                float* actRow = nullptr) {
  constexpr int NC = 32, NO = 128;
  f32x2 a0 = bias, a1 = {0.f, 0.f}, a2 = {0.f, 0.f}, a3 = {0.f, 0.f};
  const f32x4* v4 = reinterpret_cast<const f32x4*>(vec);
  // every operand read before the first FMA: left to itself the compiler reads two 16-byte pieces at a time into the same
  // registers and waits for them (lgkmcnt(0)) in front of each batch of eight FMAs -- seven exposed LDS latencies per layer-step
  f32x4 vq[NT / 4];
#pragma unroll
  for (int q = 0; q < NT / 4; ++q) vq[q] = v4[q];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int q = 0; q < NT / 4; ++q) {
    const f32x4 v = vq[q];
    a0 += w[4 * q] * f32x2{v[0], v[0]}; a1 += w[4 * q + 1] * f32x2{v[1], v[1]};
    a2 += w[4 * q + 2] * f32x2{v[2], v[2]}; a3 += w[4 * q + 3] * f32x2{v[3], v[3]};
  }
  const f32x2 acc = (a0 + a1) + (a2 + a3);
  // lanes 0..31: acc = (cell input, forget gate); lanes 32..63: (input gate, output gate)
  const float g0 = lane < 32 ? acc[0] : fastSigm(acc[0]), g1 = fastSigm(acc[1]);
  if (store) { if (LDSACT) { actRow[lane] = g0; actRow[lane + 64] = g1; } else { L.X[r * NO + lane] = g0; L.X[r * NO + lane + 64] = g1; } }
  const float ig = fromUpperHalf(g0), og = fromUpperHalf(g1);
  if (store && lane < nInL + NC)          // the operand row [input | previous output]: A operand of the weight-gradient contraction (one store)
    L.A[r * L.ldA + lane] = vec[lane < nInL ? lane : inPad + (lane - nInL)];
  if (lane < NC) {
    const float st = g0 * ig + prevSt * g1;            // (prevSt is 0 at the first step of the window)
    const float co = fastTanh(st);
    const float out = og * co;
    prevSt = st;
    if (store) { if (LDSACT) { actRow[4 * NC + lane] = st; actRow[5 * NC + lane] = co; } else { L.Y[r * NO + lane] = out; L.Y[r * NO + NC + lane] = st; L.Y[r * NO + 2 * NC + lane] = co; } }
    float blk = out;                                   // ParametricResidualLayer::forward (Layers.h:347-361)
    if (L.hasRes && lane < L.resW) blk += vec[lane] * wr + br;
    hNext[lane] = out;
    blkOut = blk;
  }
}

// ---- pieces of the wave kernels.  Each stands once: the stand-alone forward / backward kernels and the one-launch step kernels below
// are these calls in a row, with what is their own (the acting form, the head, where rows come from and go to) between them.
// wave32*: LSTM and MGU alike (NO = gate columns of a layer, 128 / 64); lstm32* / mgu32*: the cell type's own. ----
// sample b's window: steps t - T .. t and, behind a truncated episode end, step t + 1 (output row nextRow); `acting`: the agent's last states
struct WaveWin { int b, T, nextRow, nSteps; long long slot; };
__device__ __forceinline__ WaveWin wave32Window(const RecArgs& a, int b, bool acting) {
  const RecWinGeo g = recWindowGeo(a, b, acting, a.actSteps);
  return WaveWin{b, g.T, g.nextRow, g.nSteps, g.slot};
}
// residual scalars of this lane's cell (forward)
__device__ __forceinline__ void wave32ResScalars(const RecLayer& L, const float* W, int lane, float& wr, float& br) {
  const int c = lane & 31;
  wr = 0.f; br = 0.f;
  if (L.hasRes && c < L.resW) { wr = W[L.indWr + c]; br = W[L.indBr + c]; }
}
// staging of a window forward (both wavefronts): the window's standardised states, zeroed operands of both layers (V0LEN floats / 128)
template <int V0LEN>
__device__ __forceinline__ void wave32StageWindow(const RecArgs& a, const WaveWin& win, bool acting, int tid, float* sStates, float* sV0, float* sV1) {
  const int dS = a.dS;
  for (int e = tid; e < win.nSteps * dS; e += 128) {
    const int kk = e / dS, i = e - kk * dS;
    const float raw = acting ? a.actStates[e] : a.rp.S[(size_t)(win.slot - win.T + kk) * dS + i];
    sStates[e] = (raw - a.rp.stMean[i]) * a.rp.stScale[i];
  }
  for (int i = tid; i < V0LEN; i += 128) sV0[i] = 0.f;
  for (int i = tid; i < 4 * 32; i += 128) sV1[i] = 0.f;
}
// staging done, layer 0's operand of step 0 in place (stamps 1 and 2 on either side of the first barrier)
__device__ __forceinline__ void wave32FirstOperand(const WaveWin& win, int layer, int lane, int dS, const float* sStates, float* sV0) {
  REC_STAMP(win.b, 0, 1);
  vmDrain(); ldsBarrier();
  REC_STAMP(win.b, 0, 2);
  if (layer == 0 && lane < dS) sV0[lane] = sStates[lane];
  ldsBarrier();
}
// backward: this lane's row of [W_in; W_rec] -- top layer row `lane` (0..31 input, 32..63 recurrent); layer 0 row nIn + lane (recurrent
// part only: nothing is propagated to the network input) -- and, requested behind the row, its residual weight
template <int NO>
__device__ __forceinline__ const f32x4* wave32WeightRow(const RecArgs& a, const RecLayer& L, int j, int lane) {
  return reinterpret_cast<const f32x4*>(a.W + L.indW + (size_t)(j == 1 ? lane : a.L[0].nIn + (lane & 31)) * NO);
}
__device__ __forceinline__ float wave32ResRowWeight(const RecArgs& a, const RecLayer& L, int lane) {
  return (L.hasRes && lane < L.resW) ? a.W[L.indWr + lane] : 0.f;
}
// rows of the steps this sample does not have: zero deltas
template <int NO>
__device__ __forceinline__ void wave32ZeroRows(const RecArgs& a, const RecLayer& L, int b, int T, int lane) {
  for (int k = T + 1; k < a.K; ++k) {
    const long long r = (long long)b * a.K + k;
#pragma unroll
    for (int o = 0; o < NO; o += 64) L.D[r * NO + lane + o] = 0.f;
    if (L.hasRes && lane < 32) L.Rd[r * L.ldR + lane] = 0.f;
  }
}
// error w.r.t. the output of layer-step (j, k) on lanes 0..31: from above (the top layer: the head's error at step T; layer 0: sTop) plus what
// step k + 1 handed back (sRec); the residual path's row goes to memory, its share of the error below into `res`
__device__ __forceinline__ float wave32OutputError(const RecLayer& L, int j, int k, int T, long long r, int lane, float dres, float wr,
                                                   const float (*sTop)[32], const float (*sRec)[32], float& res) {
  const float eTop = j == 1 ? (k == T ? dres : 0.f) : sTop[k & 1][lane];
  if (L.hasRes) { L.Rd[r * L.ldR + lane] = eTop; res = lane < L.resW ? eTop * wr : 0.f; }
  return eTop + (k < T ? sRec[j][lane] : 0.f);
}

// ---- LSTM ----
constexpr int lstm32Terms(int in0) { return (in0 + 32) > 2 * 32 ? (in0 + 32) : 2 * 32; }      // terms per gate as the unrolled loop walks them (zero weights behind the layer's own)
// this lane's gate columns of its layer: o = lane (cell input | input gate) and lane + 64 (forget | output gate); bias, residual scalars
template <int IN0, int NT>
__device__ __forceinline__ void lstm32LoadColumns(const RecArgs& a, const RecLayer& L, int layer, int lane, f32x2 (&w)[NT], f32x2& bias, float& wr, float& br) {
  constexpr int NC = 32, NO = 128;
  const float* W = a.W;
  const float* Wl = W + L.indW;
  const int nIn = a.L[0].nIn;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    int row;
    if (layer == 0) row = i < IN0 ? (i < nIn ? i : -1) : (i < IN0 + NC ? nIn + (i - IN0) : -1);
    else row = i < 2 * NC ? i : -1;
    w[i] = row >= 0 ? f32x2{Wl[(size_t)row * NO + lane], Wl[(size_t)row * NO + lane + 64]} : f32x2{0.f, 0.f};
  }
  bias = f32x2{W[L.indB + lane], W[L.indB + lane + 64]};
  wave32ResScalars(L, W, lane, wr, br);
}
// the window forward: wavefront 0 = layer 0 at step k = it, wavefront 1 = layer 1 one step behind.  `store`: a training window (rows
// of steps <= T kept); LDSACT: their gates and states go to sAct [2][17][ACT].  idle(): wavefront 1 at it = 0, no layer-step yet;
// top(k, blk): the top layer's block output of step k, lanes 0..31 (the caller keeps steps T and T + 1).
template <int IN0, int NT, bool LDSACT, class Idle, class Top>
__device__ __forceinline__ void lstm32ForwardWindow(const RecArgs& a, const RecLayer& L, const WaveWin& win, int layer, int lane, bool store, const f32x2 (&w)[NT], f32x2 bias,
                                                    float wr, float br, float (*sV0)[NT], float (*sV1)[64], const float* sStates, float* sAct, Idle idle, Top top) {
  constexpr int NC = 32, ACT = 6 * NC;
  const int nIn = a.L[0].nIn, dS = a.dS, T = win.T, nSteps = win.nSteps;
  float prevSt = 0.f;
  for (int it = 0; it <= nSteps; ++it) {
    REC_STAMP(win.b, 0, 4 + it);
    if (layer == 0) {
      const int k = it;
      if (k < nSteps) {
        const int cb = k & 1;
        if (k + 1 < nSteps && lane < dS) sV0[cb ^ 1][lane] = sStates[(k + 1) * dS + lane];       // (that copy was last read a step ago)
        float blk = 0.f;
        lstm32LayerStep<NT, LDSACT>(L, w, bias, sV0[cb], IN0, nIn, prevSt, wr, br, &sV0[cb ^ 1][IN0], blk, store && k <= T, (long long)win.b * a.K + k, lane,
                                    LDSACT ? sAct + (0 * 17 + (k <= T ? k : 0)) * ACT : nullptr);
        if (lane < NC) sV1[cb][lane] = blk;
      }
    } else {
      const int k = it - 1;
      if (k < 0) idle();
      else {
        const int cb = k & 1;
        float blk = 0.f;
        lstm32LayerStep<NT, LDSACT>(L, w, bias, sV1[cb], NC, NC, prevSt, wr, br, &sV1[cb ^ 1][NC], blk, store && k <= T, (long long)win.b * a.K + k, lane,
                                    LDSACT ? sAct + (1 * 17 + (k <= T ? k : 0)) * ACT : nullptr);
        if (lane < NC) top(k, blk);
      }
    }
    ldsBarrier();
  }
}
// this lane's row (see wave32WeightRow) as 32 four-column pieces
__device__ __forceinline__ void lstm32LoadRow(const RecArgs& a, const RecLayer& L, int j, int lane, f32x4 (&wq)[32], float& wr) {
  const f32x4* rw = wave32WeightRow<128>(a, L, j, lane);
#pragma unroll
  for (int q = 0; q < 32; ++q) wq[q] = rw[q];
  wr = wave32ResRowWeight(a, L, lane);
}
// gate deltas of one layer-step on lanes 0..31 (LSTMLayer::backward, Layer_LSTM.h:127-165) into sDj [cell input | I | F | O]; D: error w.r.t.
// the step's output; nxtSt / nxtF: state error / forget gate of step k + 1, replaced by this step's
__device__ __forceinline__ void lstm32GateDeltas(const float* act, int k, int T, float D, float& nxtSt, float& nxtF, float* sDj, int lane) {
  constexpr int NC = 32, ACT = 6 * NC;
  const float cellInpt = act[lane], IG = act[NC + lane], FG = act[2 * NC + lane], OG = act[3 * NC + lane], co = act[5 * NC + lane];
  const float prevSt = k > 0 ? (act - ACT)[4 * NC + lane] : 0.f;
  const float diff = (1.f - co * co) * D;
  const float sd = diff * OG + (k < T ? nxtSt * nxtF : 0.f);
  const float d0 = IG * sd;
  const float d1 = IG * (1.f - IG) * cellInpt * sd;
  const float d2 = k > 0 ? FG * (1.f - FG) * prevSt * sd : 0.f;
  const float d3 = OG * (1.f - OG) * D * co;
  sDj[lane] = d0; sDj[NC + lane] = d1; sDj[2 * NC + lane] = d2; sDj[3 * NC + lane] = d3;
  nxtSt = sd; nxtF = FG;
}
// e_i = sum_o W[i][o] delta[o] for this lane's row (Layer::backward, Layers.h:123-188)
__device__ __forceinline__ float lstm32RowProduct(const f32x4 (&wq)[32], const float* sDj) {
  constexpr int NO = 128;
  const f32x4* d4 = reinterpret_cast<const f32x4*>(sDj);
  f32x2 p0 = {0.f, 0.f}, p1 = {0.f, 0.f}, p2 = {0.f, 0.f}, p3 = {0.f, 0.f};
  // (the reads of half the deltas before the first FMA of that half -- see lstm32LayerStep; all 32 pieces at once would
  //  take the step kernel past 256 VGPRs)
#pragma unroll
  for (int h0 = 0; h0 < NO / 4; h0 += NO / 8) {
    f32x4 dq[NO / 8];
#pragma unroll
    for (int q = 0; q < NO / 8; ++q) dq[q] = d4[h0 + q];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < NO / 8; q += 2) {
      const f32x4 da = dq[q], db = dq[q + 1];
      p0 += f32x2{wq[h0 + q][0], wq[h0 + q][1]} * f32x2{da[0], da[1]}; p1 += f32x2{wq[h0 + q][2], wq[h0 + q][3]} * f32x2{da[2], da[3]};
      p2 += f32x2{wq[h0 + q + 1][0], wq[h0 + q + 1][1]} * f32x2{db[0], db[1]}; p3 += f32x2{wq[h0 + q + 1][2], wq[h0 + q + 1][3]} * f32x2{db[2], db[3]};
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  const f32x2 ps = (p0 + p1) + (p2 + p3);
  return ps[0] + ps[1];
}
// back-propagation through time: wavefront 0 = the top layer (j = 1) at step k = T - it, wavefront 1 = layer 0 one step behind.  sAct
// [2][17][ACT]: per (layer, step) [cell input | I | F | O | state | tanh(state)]; dres: error w.r.t. the top block's output at step T.
__device__ __forceinline__ void lstm32BackwardWindow(const RecArgs& a, const RecLayer& L, int j, int b, int T, int lane, const f32x4 (&wq)[32], float wr, float dres,
                                                     const float* sAct, float (*sD)[128], float (*sTop)[32], float (*sRec)[32]) {
  constexpr int NC = 32, NO = 128, ACT = 6 * NC;
  float nxtSt = 0.f, nxtF = 0.f;                           // state error / forget gate of step k + 1 (lanes 0..31)
  for (int it = 0; it <= T + 1; ++it) {
    const int k = T - it + (j == 1 ? 0 : 1);               // the top layer is one step ahead
    if (k >= 0 && k <= T) {
      const long long r = (long long)b * a.K + k;
      float res = 0.f;
      if (lane < NC) {
        const float D = wave32OutputError(L, j, k, T, r, lane, dres, wr, sTop, sRec, res);
        lstm32GateDeltas(sAct + (j * 17 + k) * ACT, k, T, D, nxtSt, nxtF, sD[j], lane);
      }
      waveLdsSync();                                       // this wavefront's deltas are in LDS
      { const float u0 = sD[j][lane], u1 = sD[j][64 + lane]; L.D[r * NO + lane] = u0; L.D[r * NO + 64 + lane] = u1; }      // the row for the weight gradients: two whole-wavefront stores
      if (j == 1 || k > 0) {
        const float e = lstm32RowProduct(wq, sD[j]);
        if (j == 1) {   // rows 0..31: error of block 0's output (+ the residual path of this layer); rows 32..63: handed to step k - 1
          if (lane < NC) sTop[k & 1][lane] = res + e; else sRec[1][lane - NC] = e;
        } else if (lane < NC) sRec[0][lane] = e;
      }
    }
    ldsBarrier();
  }
}

template <int IN0>     // inputs of the first layer, padded to a multiple of 4 (<= 32)
__global__ __launch_bounds__(128) void lstm32_forward_wave_kernel(RecArgs a) {
  constexpr int NC = 32, NTMAX = lstm32Terms(IN0);
  __shared__ __attribute__((aligned(16))) float sV0[2][NTMAX];         // layer 0 operand [x_k | h0_{k-1} | 0 ...], double-buffered over the steps
  __shared__ __attribute__((aligned(16))) float sV1[2][2 * NC];        // layer 1 operand [block-0 output of step k | h1_{k-1}]
  __shared__ float sStates[18 * 32];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  REC_STAMP(b, 0, 0);
  const int layer = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave-uniform
  const bool acting = a.actStates != nullptr;                          // rollout inference: the agent's last states, nothing stored
  const WaveWin win = wave32Window(a, b, acting);
  const RecLayer L = a.L[layer];
  f32x2 w[NTMAX], bias; float wr, br;
  lstm32LoadColumns<IN0>(a, L, layer, lane, w, bias, wr, br);
  wave32StageWindow<2 * NTMAX>(a, win, acting, tid, sStates, &sV0[0][0], &sV1[0][0]);
  wave32FirstOperand(win, layer, lane, a.dS, sStates, sV0[0]);
  lstm32ForwardWindow<IN0, NTMAX, false>(a, L, win, layer, lane, !acting, w, bias, wr, br, sV0, sV1, sStates, nullptr, [] {},
    [&](int k, float blk) {
      if (k == win.T) a.Yout[(size_t)b * a.ldY + lane] = blk;
      if (k == win.T + 1) a.Yout[(size_t)win.nextRow * a.ldY + lane] = blk;
    });
  REC_STAMP(b, 0, 250);
}

__global__ __launch_bounds__(128) void lstm32_backward_wave_kernel(RecArgs a) {
  constexpr int NC = 32, NO = 128, ACT = 6 * NC;           // per (step, layer): [cell input | I | F | O | state | tanh(state)]
  __shared__ __attribute__((aligned(16))) float sD[2][NO]; // gate deltas of the layer-step, per layer
  __shared__ float sAct[2][17 * ACT];
  __shared__ float sTop[2][NC];                            // error w.r.t. block 0's output at step k (ring over k & 1), from the top layer
  __shared__ float sRec[2][NC];                            // error w.r.t. this step's LSTM output coming from step k + 1, per layer
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = 1 - wv;                                    // wavefront 0 = the top layer (one step ahead), wavefront 1 = layer 0
  const int T = min(a.nBPTT, a.bt.t[b]);
  const RecLayer L = a.L[j];
  f32x4 wq[NO / 4]; float wr;
  lstm32LoadRow(a, L, j, lane, wq, wr);
  {   // stored activations of this layer over the window
    const int total = (T + 1) * ACT;
    for (int e = lane; e < total; e += 64) {
      const int k = e / ACT, x = e - k * ACT;
      const long long r = (long long)b * a.K + k;
      sAct[j][e] = x < 4 * NC ? L.X[r * NO + x] : L.Y[r * NO + NC + (x - 4 * NC)];
    }
  }
  const float dres = (j == 1 && lane < NC) ? a.Dres[(size_t)b * a.ldD + lane] : 0.f;
  wave32ZeroRows<NO>(a, L, b, T, lane);
  vmDrain(); ldsBarrier();
  lstm32BackwardWindow(a, L, j, b, T, lane, wq, wr, dres, &sAct[0][0], sD, sTop, sRec);
}

// ---- the whole sample in ONE launch: window forward, output layer + RACER head, back-propagation through time ---------------------
// A sample's chain -- forward over its window, the head of its sampled step (and of step t+1 of a truncated episode end), backward
// over the window -- needs nothing from other samples, so the three launches of the recurrent step (lstm32_forward_wave_kernel,
// the head kernel, lstm32_backward_wave_kernel) are one workgroup's work here: no two launch boundaries (2 x 2.8 us), the gates and
// states of the window stay in LDS instead of going through memory (five of the forward pass's seven row stores per layer-step and
// the backward pass's prologue of dependent loads), the head's replay rows are requested in the prologue and its output-independent
// terms are formed while layer 0 runs its first step alone, the backward pass's weight rows arrive while the head runs.
// Wavefront 0 = layer 0, wavefront 1 = layer 1 in the forward pass (one step apart), the head on wavefront 1 (16-lane rows of
// head_rows.h: row 0 the sampled step, row 1 the next-state step), the top layer's backward on wavefront 0 as in the kernel above.
// Same arithmetic as the three kernels except the output layer and delta_y = delta_out W_out^T, which are plain fp32 dot products in
// index order here (MFMA contractions with K split over wavefronts there).  `extra`: a rider workgroup (launch of 256 threads).
constexpr int LS_LD = 38, LS_LO = 49;        // head rows in LDS: up to 32 dense outputs, 48 outputs in all
// LDS of the head phase, shared by the LSTM and the MGU form: the last block's outputs ([0] sampled step, [1] step t + 1), the error
// w.r.t. them, W_out [32][ldWo <= 40], and the rows HeadRow::compute works on
struct StepHeadLds {
  float (*sYo)[32]; float* sDres; float* sWo; float (*sXo)[LS_LD]; float (*sDelta)[LS_LD]; float (*sMisc)[8];
  double (*sO)[LS_LO]; double* sActMsg; double* sTq; double* sTr;
};
constexpr int STEP_HEAD_LDS = 2 * 32 * 4 + 32 * 4 + 32 * 40 * 4 + 2 * LS_LD * 4 * 2 + 2 * 8 * 4 + 2 * LS_LO * 8 + 2 * 8 + 2 * 2 * 64 * 8;
static_assert(STEP_HEAD_LDS % 8 == 0, "the double rows are 8-byte aligned");
__device__ __forceinline__ StepHeadLds stepHeadLds(unsigned char* p) {      // p: 8-byte aligned
  StepHeadLds S;
  S.sO = reinterpret_cast<double (*)[LS_LO]>(p); p += 2 * LS_LO * 8;
  S.sActMsg = reinterpret_cast<double*>(p); p += 2 * 8;
  S.sTq = reinterpret_cast<double*>(p); S.sTr = S.sTq + 2 * 64; p += 2 * 2 * 64 * 8;
  S.sYo = reinterpret_cast<float (*)[32]>(p); p += 2 * 32 * 4;
  S.sDres = reinterpret_cast<float*>(p); p += 32 * 4;
  S.sWo = reinterpret_cast<float*>(p); p += 32 * 40 * 4;
  S.sXo = reinterpret_cast<float (*)[LS_LD]>(p); p += 2 * LS_LD * 4;
  S.sDelta = reinterpret_cast<float (*)[LS_LD]>(p); p += 2 * LS_LD * 4;
  S.sMisc = reinterpret_cast<float (*)[8]>(p);
  return S;
}
// what the head lanes (wavefront 1, lanes 0..31: 16-lane row `em` = 0 the sampled step, 1 = step t + 1 of a truncated episode end)
// fetch in the kernel's prologue
struct StepHeadRegs { HeadRow<1> hr; float bpv[1]; float bov0, bov1; double beta, Cmax, Cinv; bool rowValid, isNext, live; int em, en; };
__device__ __forceinline__ void stepHeadLoad(StepHeadRegs& R, const HeadArgs& ha, const DevScalars* sc, int wv, int lane, long long slot, int nextRow) {
  R.em = (lane >> 4) & 1; R.en = lane & 15;
  const bool headLane = wv == 1 && lane < 32;
  R.rowValid = headLane && (R.em == 0 || nextRow >= 0); R.isNext = R.rowValid && R.em == 1; R.live = R.rowValid && !R.isNext;
  R.hr.load(ha, R.rowValid, R.isNext, slot, R.en);
  R.bpv[0] = 0.f; R.bov0 = 0.f; R.bov1 = 0.f;
  if (headLane) {
    if (R.en < ha.nSig) R.bpv[0] = ha.params[ha.indBp + R.en];
    if (R.en < ha.nDense) R.bov0 = ha.params[ha.indBo + R.en];
    if (R.en + 16 < ha.nDense) R.bov1 = ha.params[ha.indBo + R.en + 16];
  }
  R.beta = sc->beta; R.Cmax = sc->Cmax; R.Cinv = sc->Cinv;
}
// output layer + head of the sample's rows and the error w.r.t. the last block's output (S.sDres); all of wavefront 1
__device__ __forceinline__ void stepHeadRun(StepHeadRegs& R, const HeadArgs& ha, const StepHeadLds& S, int lane, int b, long long slot, int nextRow) {
  constexpr int NC = 32;
  const int em = R.em, en = R.en, nDense = ha.nDense, ldWo = ha.ldWo;
  if (lane < 32) {      // O[row][o] = y W_out + b_out, o = en and en + 16 (BaseLayer::forward of the output layer)
    float x0 = 0.f, x1 = 0.f;
    const float* y = S.sYo[em];
    const int o0 = en < ldWo ? en : ldWo - 1, o1 = en + 16 < ldWo ? en + 16 : ldWo - 1;
#pragma unroll 8
    for (int cc = 0; cc < NC; ++cc) { const float yv = y[cc]; x0 = fmaf(yv, S.sWo[cc * ldWo + o0], x0); x1 = fmaf(yv, S.sWo[cc * ldWo + o1], x1); }
    x0 += R.bov0; x1 += R.bov1;
    if (en < nDense) { S.sXo[em][en] = x0; S.sO[em][en] = (double)(ha.outFunc == HL_FUNC_LINEAR ? x0 : actEval(ha.outFunc, x0)); }
    if (en + 16 < nDense) { S.sXo[em][en + 16] = x1; S.sO[em][en + 16] = (double)(ha.outFunc == HL_FUNC_LINEAR ? x1 : actEval(ha.outFunc, x1)); }
    if (en < ha.nSig) S.sO[em][nDense + en] = (double)R.bpv[0];      // ParamLayer, Linear
    for (int o = en; o < LS_LD; o += 16) S.sDelta[em][o] = 0.f;
  }
  waveLdsSync();
  R.hr.compute(ha, S.sO[em], S.sDelta[em], S.sXo[em], S.sMisc[em], S.sTq + em * 64, S.sTr + em * 64, R.rowValid, R.isNext, true,
               b, slot, em ? nextRow : b, en, R.beta, R.Cmax, R.Cinv, S.sActMsg[em]);
  waveLdsSync();
  if (lane < NC) {      // delta_y = delta_out W_out^T: error w.r.t. the last block's output at the sampled step
    float e = 0.f;
    for (int o = 0; o < nDense; ++o) e = fmaf(S.sDelta[0][o], S.sWo[lane * ldWo + o], e);
    S.sDres[lane] = e;
  }
}

template <int IN0>
__global__ __launch_bounds__(256) void lstm32_step_wave_kernel(RecArgs a, HeadArgs ha, unsigned long long boundedMask, ExtraArgs extra) {
  constexpr int NC = 32, NO = 128, ACT = 6 * NC, NTMAX = lstm32Terms(IN0);
  constexpr int O_V0 = 2 * 17 * ACT * 4, O_V1 = O_V0 + 2 * NTMAX * 4, O_ST = O_V1 + 2 * 64 * 4, O_D = O_ST + 18 * 32 * 4, O_TOP = O_D + 2 * NO * 4,
                O_REC = O_TOP + 2 * NC * 4, O_HEAD = O_REC + 2 * NC * 4, TOTAL = O_HEAD + STEP_HEAD_LDS;
  static_assert(O_HEAD % 16 == 0, "alignment of the head rows");
  __shared__ __attribute__((aligned(16))) unsigned char smem[TOTAL > (int)TAIL_LDS_BYTES ? TOTAL : (int)TAIL_LDS_BYTES];
  if (extra.role) { if (blockIdx.x == 0) { runExtra(extra, smem); return; } if (threadIdx.x >= 128) return; }
  float* sAct = reinterpret_cast<float*>(smem);                                   // [2][17][ACT]: per (layer, step) [cell input | I | F | O | state | tanh(state)]
  float (*sV0)[NTMAX] = reinterpret_cast<float (*)[NTMAX]>(smem + O_V0);
  float (*sV1)[2 * NC] = reinterpret_cast<float (*)[2 * NC]>(smem + O_V1);
  float* sStates = reinterpret_cast<float*>(smem + O_ST);
  float (*sD)[NO] = reinterpret_cast<float (*)[NO]>(smem + O_D);
  float (*sTop)[NC] = reinterpret_cast<float (*)[NC]>(smem + O_TOP);
  float (*sRec)[NC] = reinterpret_cast<float (*)[NC]>(smem + O_REC);
  const StepHeadLds S = stepHeadLds(smem + O_HEAD);

  const int b = blockIdx.x - (extra.role ? 1 : 0), tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const WaveWin win = wave32Window(a, b, false);
  const int T = win.T;
  REC_STAMP(b, 0, 0);
  StepHeadRegs R;
  stepHeadLoad(R, ha, a.sc, wv, lane, win.slot, win.nextRow);
  {
    // ================================================ forward over the window ==================================================
    const int layer = wv;
    const RecLayer L = a.L[layer];
    f32x2 w[NTMAX], bias; float wr, br;
    lstm32LoadColumns<IN0>(a, L, layer, lane, w, bias, wr, br);
    wave32StageWindow<2 * NTMAX>(a, win, false, tid, sStates, &sV0[0][0], &sV1[0][0]);
    for (int e = tid; e < NC * ha.ldWo; e += 128) S.sWo[e] = ha.params[ha.indWo + e];
    if (wv == 1 && lane < 32) { if (R.en < 8) S.sMisc[R.em][R.en] = R.hr.misc; if (R.en == 0) S.sActMsg[R.em] = R.hr.actMsg; }
    wave32FirstOperand(win, layer, lane, a.dS, sStates, sV0[0]);
    lstm32ForwardWindow<IN0, NTMAX, true>(a, L, win, layer, lane, true, w, bias, wr, br, sV0, sV1, sStates, sAct,
      [&] { R.hr.hoist(ha, boundedMask, R.bpv, R.live, R.en); },
      [&](int k, float blk) {
        if (k == T) { a.Yout[(size_t)b * a.ldY + lane] = blk; S.sYo[0][lane] = blk; }       // (memory: A operand of the output layer's weight gradient)
        if (k == T + 1) S.sYo[1][lane] = blk;
      });
  }
  REC_STAMP(b, 0, 30);
  // ======================================================= backward: weight rows requested now ==================================
  const int j = 1 - wv;                                    // wavefront 0 = the top layer (one step ahead), wavefront 1 = layer 0
  const RecLayer L = a.L[j];
  f32x4 wq[NO / 4]; float wrB;
  lstm32LoadRow(a, L, j, lane, wq, wrB);
  wave32ZeroRows<NO>(a, L, b, T, lane);
  // ======================================================= output layer + head (wavefront 1) ====================================
  REC_STAMP(b, 0, 31);
  if (wv == 1) stepHeadRun(R, ha, S, lane, b, win.slot, win.nextRow);
  if (wv == 1) REC_STAMP(b, 64, 32);
  vmDrain(); ldsBarrier();
  REC_STAMP(b, 0, 33);
  // ======================================================= back-propagation through time ========================================
  lstm32BackwardWindow(a, L, j, b, T, lane, wq, wrB, (j == 1 && lane < NC) ? S.sDres[lane] : 0.f, sAct, sD, sTop, sRec);
  REC_STAMP(b, 0, 250);
}

// ---- MGU, two layers of 32 cells: the same arrangement ---------------------------------------------------------------------
// A layer-step has 64 gate columns -- forget gates on lanes 0..31, candidate states on lanes 32..63 (MGULayer::forward,
// Layer_GRU.h:64-124) -- and two dependent halves: the candidate's recurrent operand is prevOut * forget.  Lane o keeps column o
// of [W_in; W_rec] in registers; the forget lanes publish prevOut * f through LDS, the candidate lanes then add their 32
// recurrent terms.  Layer 0's wavefront runs one step ahead of layer 1's, as above.
template <int IN>
__device__ __forceinline__ float dotIn(const float (&w)[32], const float* vec) {
  const f32x4* v4 = reinterpret_cast<const f32x4*>(vec);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  f32x4 vq[IN / 4];      // (all reads before the first FMA: see lstm32LayerStep)
#pragma unroll
  for (int q = 0; q < IN / 4; ++q) vq[q] = v4[q];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int q = 0; q < IN / 4; ++q) { const f32x4 v = vq[q]; a0 += w[4 * q] * v[0]; a1 += w[4 * q + 1] * v[1]; a2 += w[4 * q + 2] * v[2]; a3 += w[4 * q + 3] * v[3]; }
  return (a0 + a1) + (a2 + a3);
}

// (LDSACT: forget gate, candidate and output of the step go to `actRow` in LDS -- the one-launch step keeps them for its backward pass)
template <int IN, bool LDSACT = false>      // IN: operand length of the input part as the unrolled loop walks it (zero weights behind the layer's own inputs)
__device__ __forceinline__ void mgu32LayerStep(const RecLayer& L, const float (&win)[32], const float (&wrec)[32], float bias, const float* vec,
                                               float* hf, int nInL, float wr, float br, float* hNext, float& blkOut, bool store, long long r, int lane,
                                               float* actRow = nullptr) {
  constexpr int NC = 32, NO = 64;
  const float* hPrev = vec + IN;
  const float accIn = bias + dotIn<IN>(win, vec);
  const float po = lane < NC ? hPrev[lane] : 0.f;
  const float f = fastSigm(accIn + dotIn<NC>(wrec, hPrev));            // (meaningful on the forget lanes)
  if (lane < NC) hf[lane] = po * f;
  waveLdsSync();
  const float sc = fastTanh(accIn + dotIn<NC>(wrec, hf));              // (meaningful on the candidate lanes)
  if (store) {
    if (LDSACT) actRow[lane] = lane < NC ? f : sc; else L.X[r * NO + lane] = lane < NC ? f : sc;
    if (lane < nInL + NC) L.A[r * L.ldA + lane] = vec[lane < nInL ? lane : IN + (lane - nInL)];      // [input | previous output], one store
  }
  const float st = fromUpperHalf(sc);
  if (lane < NC) {
    const float out = f * st + (1.f - f) * po;                           // (po is 0 at the first step of the window)
    if (store) { if (LDSACT) actRow[NO + lane] = out; else L.Y[r * NO + lane] = out; L.A2[r * L.ldA2 + lane] = po * f; }
    float blk = out;
    if (L.hasRes && lane < L.resW) blk += vec[lane] * wr + br;
    hNext[lane] = out;
    blkOut = blk;
  }
}

// this lane's gate column of its layer, input part (zeros behind the layer's own inputs) and recurrent part; bias, residual scalars
__device__ __forceinline__ void mgu32LoadColumns(const RecArgs& a, const RecLayer& L, int layer, int lane, float (&win)[32], float (&wrec)[32], float& bias, float& wr, float& br) {
  constexpr int NC = 32, NO = 64;
  const float* W = a.W;
  const float* Wl = W + L.indW;
  const int nInL = layer == 0 ? a.L[0].nIn : NC;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    win[i] = i < nInL ? Wl[(size_t)i * NO + lane] : 0.f;
    wrec[i] = Wl[(size_t)(nInL + i) * NO + lane];
  }
  bias = W[L.indB + lane];
  wave32ResScalars(L, W, lane, wr, br);
}
// the window forward (see lstm32ForwardWindow: the same skew, `store`, LDSACT into sAct [2][17][ACT], idle() and top(k, blk)); sHF: prevOut * forget, per layer
template <int IN0, bool LDSACT, class Idle, class Top>
__device__ __forceinline__ void mgu32ForwardWindow(const RecArgs& a, const RecLayer& L, const WaveWin& win, int layer, int lane, bool store, const float (&wIn)[32],
                                                   const float (&wrec)[32], float bias, float wr, float br, float (*sV0)[IN0 + 32], float (*sV1)[64], float (*sHF)[32],
                                                   const float* sStates, float* sAct, Idle idle, Top top) {
  constexpr int NC = 32, ACT = 3 * NC;
  const int nIn = a.L[0].nIn, dS = a.dS, T = win.T, nSteps = win.nSteps;
  for (int it = 0; it <= nSteps; ++it) {
    if (layer == 0) {
      const int k = it;
      if (k < nSteps) {
        const int cb = k & 1;
        if (k + 1 < nSteps && lane < dS) sV0[cb ^ 1][lane] = sStates[(k + 1) * dS + lane];
        float blk = 0.f;
        mgu32LayerStep<IN0, LDSACT>(L, wIn, wrec, bias, sV0[cb], sHF[0], nIn, wr, br, &sV0[cb ^ 1][IN0], blk, store && k <= T, (long long)win.b * a.K + k, lane,
                                    LDSACT ? sAct + (0 * 17 + (k <= T ? k : 0)) * ACT : nullptr);
        if (lane < NC) sV1[cb][lane] = blk;
      }
    } else {
      const int k = it - 1;
      if (k < 0) idle();
      else {
        const int cb = k & 1;
        float blk = 0.f;
        mgu32LayerStep<NC, LDSACT>(L, wIn, wrec, bias, sV1[cb], sHF[1], NC, wr, br, &sV1[cb ^ 1][NC], blk, store && k <= T, (long long)win.b * a.K + k, lane,
                                   LDSACT ? sAct + (1 * 17 + (k <= T ? k : 0)) * ACT : nullptr);
        if (lane < NC) top(k, blk);
      }
    }
    ldsBarrier();
  }
}
// backward (MGULayer::backward, Layer_GRU.h:126-231): lane i holds ROW i of [W_in; W_rec] (32 forget + 32 candidate columns); the
// top layer's lanes 0..31 are its input rows, 32..63 its recurrent rows; layer 0 needs its recurrent rows only (lanes 0..31)
__device__ __forceinline__ void mgu32LoadRow(const RecArgs& a, const RecLayer& L, int j, int lane, float (&wf)[32], float (&ws)[32], float& wr) {
  const f32x4* rw = wave32WeightRow<64>(a, L, j, lane);
#pragma unroll
  for (int q = 0; q < 8; ++q) { const f32x4 u = rw[q], v = rw[8 + q]; wf[4 * q] = u[0]; wf[4 * q + 1] = u[1]; wf[4 * q + 2] = u[2]; wf[4 * q + 3] = u[3];
                                ws[4 * q] = v[0]; ws[4 * q + 1] = v[1]; ws[4 * q + 2] = v[2]; ws[4 * q + 3] = v[3]; }
  wr = wave32ResRowWeight(a, L, lane);
}
// back-propagation through time (the skew of lstm32BackwardWindow).  sAct [2][17][ACT]: per (layer, step) [forget | candidate | output];
// wf / ws: this lane's row, forget / candidate columns; sDS / sDF: the deltas of the layer-step, per layer
__device__ __forceinline__ void mgu32BackwardWindow(const RecArgs& a, const RecLayer& L, int j, int b, int T, int lane, const float (&wf)[32], const float (&ws)[32], float wr,
                                                    float dres, const float* sAct, float (*sDS)[32], float (*sDF)[32], float (*sTop)[32], float (*sRec)[32]) {
  constexpr int NC = 32, NO = 64, ACT = 3 * NC;
  for (int it = 0; it <= T + 1; ++it) {
    const int k = T - it + (j == 1 ? 0 : 1);
    if (k >= 0 && k <= T) {
      const long long r = (long long)b * a.K + k;
      float res = 0.f, dLdO = 0.f, f = 0.f, sc = 0.f, po = 0.f, dS_ = 0.f;
      if (lane < NC) {
        const float* act = sAct + (j * 17 + k) * ACT;
        dLdO = wave32OutputError(L, j, k, T, r, lane, dres, wr, sTop, sRec, res);
        f = act[lane]; sc = act[NC + lane]; po = k > 0 ? (act - ACT)[2 * NC + lane] : 0.f;
        dS_ = dLdO * f * (1.f - sc * sc);                                         // 1) dLdS
        sDS[j][lane] = dS_;
      }
      waveLdsSync();
      const float viaS = dotIn<NC>(ws, sDS[j]);                                    // row i: sum_o W[i][nC + o] dLdS[o]
      float fp = j == 1 ? fromUpperHalf(viaS) : viaS;                              // 2) dLdFprevOut of cell c = the recurrent row nIn + c
      if (k == 0) fp = 0.f;
      if (lane < NC) {
        const float dF = ((sc - po) * dLdO + fp * po) * f * (1.f - f);             // 3) dLdF
        sDF[j][lane] = dF;
      }
      waveLdsSync();
      L.D[r * NO + lane] = lane < NC ? sDF[j][lane] : sDS[j][lane - NC];          // the row for the weight gradients [dLdF | dLdS]: one whole-wavefront store
      const float viaF = dotIn<NC>(wf, sDF[j]);                                    // row i: sum_o W[i][o] dLdF[o]
      const float g = j == 1 ? fromUpperHalf(viaF) : viaF;
      if (lane < NC) {
        if (j == 1) sTop[k & 1][lane] = (res + viaF) + viaS;                       // error of block 0's output (+ the residual path)
        if (k > 0) sRec[j][lane] = ((1.f - f) * dLdO + f * fp) + g;                // 4) dLdprevOut
      }
    }
    ldsBarrier();
  }
}

template <int IN0>
__global__ __launch_bounds__(128) void mgu32_forward_wave_kernel(RecArgs a) {
  constexpr int NC = 32;
  __shared__ __attribute__((aligned(16))) float sV0[2][IN0 + NC];      // layer 0 operand [x_k | h0_{k-1}], double-buffered over the steps
  __shared__ __attribute__((aligned(16))) float sV1[2][2 * NC];        // layer 1 operand [block-0 output of step k | h1_{k-1}]
  __shared__ __attribute__((aligned(16))) float sHF[2][NC];            // prevOut * forget, per layer
  __shared__ float sStates[18 * 32];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int layer = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool acting = a.actStates != nullptr;                          // rollout inference: the agent's last states, nothing stored
  const WaveWin win = wave32Window(a, b, acting);
  const RecLayer L = a.L[layer];
  float wIn[32], wrec[32], bias, wr, br;
  mgu32LoadColumns(a, L, layer, lane, wIn, wrec, bias, wr, br);
  wave32StageWindow<2 * (IN0 + NC)>(a, win, acting, tid, sStates, &sV0[0][0], &sV1[0][0]);
  wave32FirstOperand(win, layer, lane, a.dS, sStates, sV0[0]);
  mgu32ForwardWindow<IN0, false>(a, L, win, layer, lane, !acting, wIn, wrec, bias, wr, br, sV0, sV1, sHF, sStates, nullptr, [] {},
    [&](int k, float blk) {
      if (k == win.T) a.Yout[(size_t)b * a.ldY + lane] = blk;
      if (k == win.T + 1) a.Yout[(size_t)win.nextRow * a.ldY + lane] = blk;
    });
}

__global__ __launch_bounds__(128) void mgu32_backward_wave_kernel(RecArgs a) {
  constexpr int NC = 32, NO = 64, ACT = 3 * NC;            // per (step, layer): [forget | candidate | output]
  __shared__ __attribute__((aligned(16))) float sDS[2][NC], sDF[2][NC];
  __shared__ float sAct[2][17 * ACT];
  __shared__ float sTop[2][NC];
  __shared__ float sRec[2][NC];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = 1 - wv;                                    // wavefront 0 = the top layer (one step ahead), wavefront 1 = layer 0
  const int T = min(a.nBPTT, a.bt.t[b]);
  const RecLayer L = a.L[j];
  float wf[32], ws[32], wr;                                // this lane's row: forget columns, candidate columns
  mgu32LoadRow(a, L, j, lane, wf, ws, wr);
  {
    const int total = (T + 1) * ACT;
    for (int e = lane; e < total; e += 64) {
      const int k = e / ACT, x = e - k * ACT;
      const long long r = (long long)b * a.K + k;
      sAct[j][e] = x < NO ? L.X[r * NO + x] : L.Y[r * NO + (x - NO)];
    }
  }
  const float dres = (j == 1 && lane < NC) ? a.Dres[(size_t)b * a.ldD + lane] : 0.f;
  wave32ZeroRows<NO>(a, L, b, T, lane);
  vmDrain(); ldsBarrier();
  mgu32BackwardWindow(a, L, j, b, T, lane, wf, ws, wr, dres, &sAct[0][0], sDS, sDF, sTop, sRec);
}

// ---- the MGU form of the one-launch step (see lstm32_step_wave_kernel): window forward, output layer + head, back-propagation through
// time of a sample in one workgroup; forget gates, candidates and outputs of the window stay in LDS ---------------------------------
template <int IN0>
__global__ __launch_bounds__(256) void mgu32_step_wave_kernel(RecArgs a, HeadArgs ha, unsigned long long boundedMask, ExtraArgs extra) {
  constexpr int NC = 32, ACT = 3 * NC;                     // per (step, layer): [forget | candidate | output]
  constexpr int O_V0 = 2 * 17 * ACT * 4, O_V1 = O_V0 + 2 * (IN0 + NC) * 4, O_HF = O_V1 + 2 * 64 * 4, O_ST = O_HF + 2 * NC * 4, O_DS = O_ST + 18 * 32 * 4,
                O_DF = O_DS + 2 * NC * 4, O_TOP = O_DF + 2 * NC * 4, O_REC = O_TOP + 2 * NC * 4, O_HEAD = O_REC + 2 * NC * 4, TOTAL = O_HEAD + STEP_HEAD_LDS;
  static_assert(O_HEAD % 16 == 0 && O_V0 % 16 == 0 && O_V1 % 16 == 0 && O_HF % 16 == 0 && O_DS % 16 == 0 && O_DF % 16 == 0, "alignment of the 16-byte reads");
  __shared__ __attribute__((aligned(16))) unsigned char smem[TOTAL > (int)TAIL_LDS_BYTES ? TOTAL : (int)TAIL_LDS_BYTES];
  if (extra.role) { if (blockIdx.x == 0) { runExtra(extra, smem); return; } if (threadIdx.x >= 128) return; }
  float* sAct = reinterpret_cast<float*>(smem);                                   // [2][17][ACT]
  float (*sV0)[IN0 + NC] = reinterpret_cast<float (*)[IN0 + NC]>(smem + O_V0);
  float (*sV1)[2 * NC] = reinterpret_cast<float (*)[2 * NC]>(smem + O_V1);
  float (*sHF)[NC] = reinterpret_cast<float (*)[NC]>(smem + O_HF);
  float* sStates = reinterpret_cast<float*>(smem + O_ST);
  float (*sDS)[NC] = reinterpret_cast<float (*)[NC]>(smem + O_DS);
  float (*sDF)[NC] = reinterpret_cast<float (*)[NC]>(smem + O_DF);
  float (*sTop)[NC] = reinterpret_cast<float (*)[NC]>(smem + O_TOP);
  float (*sRec)[NC] = reinterpret_cast<float (*)[NC]>(smem + O_REC);
  const StepHeadLds S = stepHeadLds(smem + O_HEAD);

  const int b = blockIdx.x - (extra.role ? 1 : 0), tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const WaveWin win = wave32Window(a, b, false);
  const int T = win.T;
  StepHeadRegs R;
  stepHeadLoad(R, ha, a.sc, wv, lane, win.slot, win.nextRow);
  {
    // ================================================ forward over the window ==================================================
    const int layer = wv;
    const RecLayer L = a.L[layer];
    float wIn[32], wrec[32], bias, wr, br;
    mgu32LoadColumns(a, L, layer, lane, wIn, wrec, bias, wr, br);
    wave32StageWindow<2 * (IN0 + NC)>(a, win, false, tid, sStates, &sV0[0][0], &sV1[0][0]);
    for (int e = tid; e < NC * ha.ldWo; e += 128) S.sWo[e] = ha.params[ha.indWo + e];
    if (wv == 1 && lane < 32) { if (R.en < 8) S.sMisc[R.em][R.en] = R.hr.misc; if (R.en == 0) S.sActMsg[R.em] = R.hr.actMsg; }
    wave32FirstOperand(win, layer, lane, a.dS, sStates, sV0[0]);
    mgu32ForwardWindow<IN0, true>(a, L, win, layer, lane, true, wIn, wrec, bias, wr, br, sV0, sV1, sHF, sStates, sAct,
      [&] { R.hr.hoist(ha, boundedMask, R.bpv, R.live, R.en); },
      [&](int k, float blk) {
        if (k == T) { a.Yout[(size_t)b * a.ldY + lane] = blk; S.sYo[0][lane] = blk; }
        if (k == T + 1) S.sYo[1][lane] = blk;
      });
  }
  // ======================================================= backward: weight rows requested now ==================================
  const int j = 1 - wv;                                    // wavefront 0 = the top layer (one step ahead), wavefront 1 = layer 0
  const RecLayer L = a.L[j];
  float wf[32], ws[32], wrB;                               // this lane's row: forget columns, candidate columns
  mgu32LoadRow(a, L, j, lane, wf, ws, wrB);
  wave32ZeroRows<64>(a, L, b, T, lane);
  // ======================================================= output layer + head (wavefront 1) ====================================
  if (wv == 1) stepHeadRun(R, ha, S, lane, b, win.slot, win.nextRow);
  vmDrain(); ldsBarrier();
  // ======================================================= back-propagation through time ========================================
  mgu32BackwardWindow(a, L, j, b, T, lane, wf, ws, wrB, (j == 1 && lane < NC) ? S.sDres[lane] : 0.f, sAct, sDS, sDF, sTop, sRec);
}

// ---- nnType "RNN": dense layers with a recurrent term (BaseLayer with bRecurrent; Network/Builder.cpp:76-81,
// Network/Layers/Layer_Base.h:64-113): x_t = W_in^T in_t + W_rec^T y_{t-1} + b, y_t = f(x_t); weights [W_in; W_rec] row-major with the
// dense layers' pitch roundUp(cells, 8); backward Layer::backward with NR = cells (Layers.h:123-188).  One workgroup per sample
// walks the window; the weights of all layers sit in LDS (recCols(1, cells) + 1 floats per row); a cell's sum is split over the four
// wavefronts (rows i = wave, wave + 4, ...) and joined in wave order.  Rows kept per (sample, step): [input | previous output] (A
// operand of the weight gradients), x, y, and the deltas after f'.  The window's states are fetched step by step (no sStates). ----
template <bool LDSW, bool MANY>
__global__ __launch_bounds__(256) void rnn_forward_kernel(RecArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sW[];
  __shared__ float sBuf[2][REC_GENIN];
  __shared__ float sPrevOut[HL_MAX_HIDDEN][REC_GENC];
  __shared__ float sPart[4][REC_GENC];
  const int b = blockIdx.x, tid = threadIdx.x, c0 = tid & 63, part = tid >> 6;
  const RecWin<MANY> win(a, b);
  if constexpr (LDSW) recStageWeights(a, 1, sW);
  float bias[HL_MAX_HIDDEN], wr[HL_MAX_HIDDEN], br[HL_MAX_HIDDEN];
  recLoadParams<1>(a, a.nL, bias, wr, br);
  const RecIn in0 = recPreloadStates<true, false>(a, win, nullptr);
  vmDrain(); ldsBarrier();
  for (int k = 0; k < win.nSteps; ++k) {
    const bool store = !win.acting && k <= win.T;
    const long long r = (long long)b * a.K + k;
    recFirstInput(a, win, in0, nullptr, b, k, sBuf[0]);
    ldsBarrier();
    int cur = 0;
    for (int j = 0; j < a.nL; ++j) {
      const RecLayer& L = a.L[j];
      const int nIn = L.nIn, nC = L.nC;
      const float* in = sBuf[cur];
      const RecWeights<LDSW> w(a, sW, 1, j, L);
      if (store) recStoreOperandRow(L, r, in, sPrevOut[j], k);
      for (int c = c0; c < nC; c += 64) {       // quarter sums over the rows i = part, part + 4, ...: first the inputs, then the previous outputs
        float acc = 0.f;
#pragma unroll 4
        for (int i = part; i < nIn; i += 4) acc += in[i] * w(i, c);
        if (k > 0) {
#pragma unroll 4
          for (int i = part; i < nC; i += 4) acc += sPrevOut[j][i] * w(nIn + i, c);
        }
        sPart[part][c] = acc;
      }
      ldsBarrier();
      float out = 0.f;
      if (tid < nC) {
        const float x = bias[j] + ((sPart[0][tid] + sPart[1][tid]) + (sPart[2][tid] + sPart[3][tid]));
        out = actEval(a.func, x);
        if (store) { L.X[r * nC + tid] = x; L.Y[r * nC + tid] = out; }
        sBuf[cur ^ 1][tid] = recBlockOutput(L, out, in, wr[j], br[j], tid);
      }
      ldsBarrier();
      if (tid < nC) sPrevOut[j][tid] = out;
      cur ^= 1;
    }
    if (tid < a.L[a.nL - 1].nC) recStoreYout<true>(a, win, b, k, tid, &sBuf[cur][tid]);
    ldsBarrier();
  }
}
template <bool LDSW>
__global__ __launch_bounds__(256) void rnn_backward_kernel(RecArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sW[];
  __shared__ float sTop[2][REC_GENIN];                    // error w.r.t. the output of the current block (from above, same step)
  __shared__ float sRec[HL_MAX_HIDDEN][REC_GENC];          // error w.r.t. this step's output coming from step k+1
  __shared__ float sD[REC_GENC], sRes[REC_GENC], sRecNew[REC_GENC];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = min(a.nBPTT, a.bt.t[b]);
  if constexpr (LDSW) recStageWeights(a, 1, sW);
  float wr[HL_MAX_HIDDEN];
  recLoadResWeights(a.L, a.W, a.nL, wr);
  vmDrain(); ldsBarrier();
  recZeroRows(a, a.nL, 1, b, T);
  for (int k = T; k >= 0; --k) {
    const long long r = (long long)b * a.K + k;
    int cur = 0;
    if (tid < a.L[a.nL - 1].nC) sTop[0][tid] = recTopError<true>(a, b, r, k, T, tid);
    ldsBarrier();
    for (int j = a.nL - 1; j >= 0; --j) {
      const RecLayer& L = a.L[j];
      const int nC = L.nC;
      const RecWeights<LDSW> w(a, sW, 1, j, L);
      if (tid < nC) {
        const float eTop = sTop[cur][tid];
        recResidualBack(L, r, eTop, wr[j], sRes);
        const float D = eTop + (k < T ? sRec[j][tid] : 0.f);
        const float d = D * actDiff(a.func, L.X[r * nC + tid], L.Y[r * nC + tid]);     // BaseLayer::backward (Layer_Base.h:97-113)
        sD[tid] = d; L.D[r * nC + tid] = d;
      }
      ldsBarrier();
      recErrorRows<false>(L, w, j, k, nC, sD, sRes, sTop[cur ^ 1], sRecNew);
      ldsBarrier();
      if (tid < nC) sRec[j][tid] = k > 0 ? sRecNew[tid] : 0.f;
      cur ^= 1;
    }
    ldsBarrier();
  }
}

// Convolutional layers in front of recurrent ones: every step of a sample's window passes through the conv stack, so the conv
// launches run over B K window rows (+ the truncated next states behind them) instead of B sampled rows.  This kernel writes the
// row -> (replay slot, step) map in the form stack_gather_kernel / the conv kernels already read: rows r = b K + k < B K hold step
// t - T + min(k, T) of sample b (rows of steps a window does not have repeat its last one: their deltas are zero), next row j
// belongs to window row b K + T; the row count goes into a DevScalars of its own.
__global__ __launch_bounds__(256) void window_rows_kernel(WinRowsArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int nNext = a.sc->nRows[a.parity] - a.B, BK = a.B * a.K;
  if (i == 0) { a.scW->nRows[a.parity] = BK + nNext; a.scW->nNext[a.parity] = nNext; }
  if (i < BK) {
    const int b = i / a.K, k = i - b * a.K, t = a.t[b], T = min(a.nBPTT, t), kk = min(k, T);
    a.slotW[i] = a.slot[b] - T + kk; a.tW[i] = t - T + kk;
  } else if (i - BK < nNext) {
    const int j = i - BK, b = a.nextSrc[j];
    a.nextSrcW[j] = b * a.K + min(a.nBPTT, a.t[b]);
  }
}
hipError_t launch_window_rows(const WinRowsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(window_rows_kernel, dim3((a.B * a.K + a.B + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}


// the wave-per-(sample, layer) kernels serve two LSTM (gates = 4) or MGU (2) layers of 32 cells each over up to 32 inputs and 17 steps
static bool wave32(const RecArgs& a, int gates) {      // (forward: training windows and rollout inference; backward: training only)
  return a.gates == gates && (a.actStates == nullptr || a.actSteps <= 17) && a.nL == 2 && a.L[0].nC == 32 && a.L[1].nC == 32 && a.L[1].nIn == 32 &&
         a.L[0].nIn <= 32 && a.dS == a.L[0].nIn && a.K <= 17 && a.L[0].indW % 4 == 0 && a.L[1].indW % 4 == 0 && !a.L[0].hasRes;
}
// ... their forward and step kernels are instantiated for first-layer inputs padded to 4, 8, 16 and 32: launch(in0) with in0 a
// std::integral_constant launches the kernel of the family for that width
template <class Launch> static hipError_t launchWave32(const RecArgs& a, Launch launch) {
  const int in0 = (a.L[0].nIn + 3) & ~3;
  if (in0 <= 4) launch(std::integral_constant<int, 4>{});
  else if (in0 <= 8) launch(std::integral_constant<int, 8>{});
  else if (in0 <= 16) launch(std::integral_constant<int, 16>{});
  else launch(std::integral_constant<int, 32>{});
  return hipGetLastError();
}
// shapes only the one-gate-per-thread kernels serve: inputs other than the step's own observed state, layers wider than 64 cells
static bool recGeneral(const RecArgs& a) {
  bool wide = false;
  for (int j = 0; j < a.nL; ++j) wide = wide || a.L[j].nC > REC_MAXC || a.L[j].nIn > REC_MAXIN;
  return wide || a.Xin != nullptr || a.nApp > 0;
}
// ---- which kernel a net gets, stated ONCE: the launchers, rec_win_act_ok and rec_route_name read this.  The choice follows from the
// layers, the input form and K alone -- the two time-step-major predicates are the only rules that read B or the per-agent tables. ----
enum RecKind { REC_TM, REC_WAVE32, REC_RNN, REC_MGU, REC_LSTM, REC_LSTM_LDS };      // rectm.hip | *32_*_wave_kernel | rnn_* | mgu_* | rec_* | lstm_*_lds
struct RecRoute { RecKind kind; bool ldsw; int NL, NC; size_t lds; };               // ... its LDSW, NL, NC template arguments; dynamic LDS in bytes
static RecRoute recRoute(const RecArgs& a, bool backward) {
  // wide layers: time-step-major on the MFMA; forward also the acting window of nets wider than the kernels here hold
  if (rec_tm_ok(a) || (!backward && rec_tm_act_ok(a))) return {REC_TM, false, 0, 0, 0};
  const bool general = recGeneral(a);
  // two layers of 32 cells: one wavefront per (sample, layer), weights in registers
  if (a.gates != 1 && !general && (wave32(a, 2) || wave32(a, 4))) return {REC_WAVE32, false, 0, 0, 0};
  // the one-gate-per-thread kernels, weights in LDS where they fit (their static LDS, up to 46 KB, comes on top; 160 KB per workgroup)
  const size_t lds = (size_t)recLdsFloats(a, a.gates, a.nL) * sizeof(float); const bool fit = lds <= 100 * 1024;
  RecRoute r = {a.gates == 1 ? REC_RNN : (a.gates == 2 ? REC_MGU : REC_LSTM), fit, 0, 0, fit ? lds : 0};
  if (a.gates == 1 || general) return r;
  if (a.gates == 2) { if (fit && a.nL <= 2) r.NL = a.nL; return r; }
  // LSTM over the step's own state, up to 64 cells: the kernels with their own LDS layouts, each direction where ITS copy fits
  size_t fl = 0; bool al = true, same = true;
  for (int j = 0; j < a.nL; ++j) {
    const RecLayer& L = a.L[j];
    fl += backward ? (size_t)lstmBwdFloats(L.nIn, L.nC) + (size_t)a.K * lstmBwdActFloats(L.nC) : (size_t)lstmGeo(L.nIn, L.nC).floats;
    al = al && L.indW % 4 == 0 && L.nIn <= REC_MAXIN;
    // (hidden layers above the first take the block below as input; the specialised forward body relies on nIn == cells there)
    same = same && L.nC == a.L[0].nC && (j == 0 || L.nIn == a.L[0].nC);
  }
  if (al && fl * sizeof(float) <= 120 * 1024) {
    if (!backward && same && a.nL == 2 && a.L[0].nC == 32) return {REC_LSTM_LDS, true, 2, 32, fl * sizeof(float)};      // RACER_RNN.json behind other inputs
    return {REC_LSTM_LDS, true, a.nL <= 3 ? a.nL : 0, 0, fl * sizeof(float)};
  }
  if (!backward) { r.ldsw = false; r.lds = 0; }      // (the forward kernel then reads its weights through the L2; the backward one stages them where they fit)
  return r;
}
typedef void (*RecKernel)(RecArgs);
template <bool MANY> static RecKernel recForwardKernel(const RecRoute& r) {
  if (r.kind == REC_RNN) { if (r.ldsw) return rnn_forward_kernel<true, MANY>; return rnn_forward_kernel<false, MANY>; }
  if (r.kind == REC_LSTM) { if (r.ldsw) return rec_forward_kernel<true, MANY>; return rec_forward_kernel<false, MANY>; }
  if (r.kind == REC_MGU) {
    if (!r.ldsw) return mgu_forward_kernel<false, 0, MANY>;
    if (r.NL == 1) return mgu_forward_kernel<true, 1, MANY>;
    if (r.NL == 2) return mgu_forward_kernel<true, 2, MANY>;
    return mgu_forward_kernel<true, 0, MANY>;
  }
  if (r.NC == 32) return lstm_forward_lds_kernel<2, 32, MANY>;
  if (r.NL == 1) return lstm_forward_lds_kernel<1, 0, MANY>;
  if (r.NL == 2) return lstm_forward_lds_kernel<2, 0, MANY>;
  if (r.NL == 3) return lstm_forward_lds_kernel<3, 0, MANY>;
  return lstm_forward_lds_kernel<0, 0, MANY>;
}
static RecKernel recBackwardKernel(const RecRoute& r) {
  if (r.kind == REC_RNN) { if (r.ldsw) return rnn_backward_kernel<true>; return rnn_backward_kernel<false>; }
  if (r.kind == REC_LSTM) { if (r.ldsw) return rec_backward_kernel<true>; return rec_backward_kernel<false>; }
  if (r.kind == REC_MGU) {
    if (!r.ldsw) return mgu_backward_kernel<false, 0>;
    if (r.NL == 1) return mgu_backward_kernel<true, 1>;
    if (r.NL == 2) return mgu_backward_kernel<true, 2>;
    return mgu_backward_kernel<true, 0>;
  }
  if (r.NL == 1) return lstm_backward_lds_kernel<1>;
  if (r.NL == 2) return lstm_backward_lds_kernel<2>;
  if (r.NL == 3) return lstm_backward_lds_kernel<3>;
  return lstm_backward_lds_kernel<0>;
}
// the kernel of this net with its template arguments as text (the forward kernels' last one, the form for the per-agent tables, left out)
std::string rec_route_name(const RecArgs& a, bool backward) {
  const RecRoute r = recRoute(a, backward);
  const char* dir = backward ? "backward" : "forward"; const char* ldsw = r.ldsw ? "true" : "false";
  char t[96];
  switch (r.kind) {
    case REC_TM: snprintf(t, sizeof(t), "launch_rec_tm_%s", dir); break;
    case REC_WAVE32: snprintf(t, sizeof(t), "%s32_%s_wave_kernel", a.gates == 2 ? "mgu" : "lstm", dir); break;
    case REC_RNN: snprintf(t, sizeof(t), "rnn_%s_kernel<%s>", dir, ldsw); break;
    case REC_MGU: snprintf(t, sizeof(t), "mgu_%s_kernel<%s, %d>", dir, ldsw, r.NL); break;
    case REC_LSTM: snprintf(t, sizeof(t), "rec_%s_kernel<%s>", dir, ldsw); break;
    case REC_LSTM_LDS: if (backward) snprintf(t, sizeof(t), "lstm_backward_lds_kernel<%d>", r.NL); else snprintf(t, sizeof(t), "lstm_forward_lds_kernel<%d, %d>", r.NL, r.NC); break;
  }
  return t;
}
static hipError_t recLaunch(RecKernel kernel, const RecArgs& a, size_t lds, hipStream_t s) {
  if (lds > 0) { hipError_t e = ensureDynLds(reinterpret_cast<const void*>(kernel), lds); if (e != hipSuccess) return e; }
  hipLaunchKernelGGL(kernel, dim3(a.B), dim3(256), lds, s, a);
  return hipGetLastError();
}
// Acting through the workgroup-per-sample kernels, whose acting form knows the per-agent tables: one window of a.actSteps given states
// (B = 1) or, with actOff / actCnt, the windows of a.B agents, workgroup b walking agent b's.  True exactly where launch_rec_forward
// takes one of them; the route is asked for the single-agent call.
bool rec_win_act_ok(const RecArgs& a) {
  const bool many = a.actOff != nullptr && a.actCnt != nullptr;
  if (a.actStates == nullptr || (a.actOff != nullptr) != (a.actCnt != nullptr) || (many ? a.B < 1 : a.B != 1)) return false;
  if (a.actSteps < 1 || a.actSteps > a.nBPTT + 1 || a.actSteps > a.K || a.nL < 1) return false;
  if (a.gates != 1 && a.YoutRows != nullptr) return false;      // (every step's output as a row: the plain recurrent kernel alone)
  for (int j = 0; j < a.nL; ++j) if (a.L[j].nC > REC_GENC || a.L[j].nIn > REC_GENIN) return false;
  RecArgs one = a; one.B = 1; one.actOff = nullptr; one.actCnt = nullptr;
  const RecKind kind = recRoute(one, false).kind;
  return kind != REC_TM && kind != REC_WAVE32;
}
hipError_t launch_rec_forward(const RecArgs& a, hipStream_t s) {
  const RecRoute r = recRoute(a, false);
  if (r.kind == REC_TM) return launch_rec_tm_forward(a, s);
  if (r.kind == REC_WAVE32) {
    if (a.gates == 2) return launchWave32(a, [&](auto in0) { hipLaunchKernelGGL(mgu32_forward_wave_kernel<decltype(in0)::value>, dim3(a.B), dim3(128), 0, s, a); });
    return launchWave32(a, [&](auto in0) { hipLaunchKernelGGL(lstm32_forward_wave_kernel<decltype(in0)::value>, dim3(a.B), dim3(128), 0, s, a); });
  }
  // its form for the per-agent tables where they are given, else the form it had
  const bool many = a.actStates != nullptr && a.actCnt != nullptr;
  return recLaunch(many ? recForwardKernel<true>(r) : recForwardKernel<false>(r), a, r.lds, s);
}
// the one-launch step (lstm32_step_wave_kernel): the shapes of the wave-per-(sample, layer) LSTM kernels with a head of up to 32
// dense outputs and 16 action components / options
bool rec_step_fused_ok(const RecArgs& a, const HeadArgs& ha) {
  const int comps = ha.nOpt ? ha.nOpt : ha.dA;
  return !recGeneral(a) && (wave32(a, 4) || wave32(a, 2)) && a.actStates == nullptr && a.YoutRows == nullptr && a.DresRows == nullptr && a.K <= 17 &&
         ha.H == 32 && ha.nDense <= 32 && ha.nOut <= 48 && comps <= 16 && ha.ldWo <= 40;
}
hipError_t launch_rec_step_fused(const RecArgs& a, const HeadArgs& ha, const ExtraArgs* extra, hipStream_t s) {
  if (!rec_step_fused_ok(a, ha)) return hipErrorInvalidValue;
  ExtraArgs ex{}; if (extra) ex = *extra;
  unsigned long long mask = 0; for (int c = 0; c < HL_MAX_DIMA && c < 64; ++c) if (ha.bounded[c]) mask |= 1ull << c;
  const dim3 grid(a.B + (ex.role ? 1 : 0)), block(ex.role ? 256 : 128);
  if (a.gates == 2) return launchWave32(a, [&](auto in0) { hipLaunchKernelGGL(mgu32_step_wave_kernel<decltype(in0)::value>, grid, block, 0, s, a, ha, mask, ex); });
  return launchWave32(a, [&](auto in0) { hipLaunchKernelGGL(lstm32_step_wave_kernel<decltype(in0)::value>, grid, block, 0, s, a, ha, mask, ex); });
}
hipError_t launch_rec_backward(const RecArgs& a, hipStream_t s) {
  const RecRoute r = recRoute(a, true);
  if (r.kind == REC_TM) return launch_rec_tm_backward(a, s);
  if (r.kind == REC_WAVE32) {
    if (a.gates == 2) hipLaunchKernelGGL(mgu32_backward_wave_kernel, dim3(a.B), dim3(128), 0, s, a);
    else hipLaunchKernelGGL(lstm32_backward_wave_kernel, dim3(a.B), dim3(128), 0, s, a);
    return hipGetLastError();
  }
  return recLaunch(recBackwardKernel(r), a, r.lds, s);
}

}  // namespace hl

#ifdef REC_STAMPS
extern "C" int hl_debug_rec_stamps(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(hl::recStamps), sizeof(unsigned long long) * 256);
}
#endif
