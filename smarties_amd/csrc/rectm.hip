// smarties_amd/csrc/rectm.hip -- LSTM / MGU layers wider than 64 cells and plain RNN layers wider than 256, TIME-STEP-MAJOR: one launch per (layer, window step) over the whole
// minibatch, the step's gate sums as ONE product on the MFMA (round 5; VERDICT r04: "rec.hip contains no MFMA").
//
//   reference: Network/Layers/Layer_LSTM.h:77-166 (forward / backward of one step), Network/Network.h:155-193 (back-propagation over
//   the time series), Layers.h:123-188 (Layer::backward), Layers.h:347-393 (parametric residual).
//
// rec.hip's any-width kernels walk ONE sample's window per workgroup and read the layer's weights (2 MB at 2 x 256 cells) through the
// L2 for every sample and step: 2.9 ms per training step at 2 x 256 cells, batch 128, 17 steps (7 GB of L2 reads).  Here the windows
// are aligned at their first step; at global step k the rows r = b K + k of all samples that have that step form the operand of
//     gates[b][o] = bias[o] + sum_i A[r][i] W[i][o],        A[r] = [input of the step | previous output]   (the dW operand row itself)
// a [B x (nIn + nC)] x [(nIn + nC) x 4 nC] product per layer and step: the weights are read once per step, not once per sample.
//   forward   lstm_tm_prepare_kernel (window geometry per sample, the first layer's input rows; acting: lstm_tm_prepare_act_kernel for one
//             agent's window, lstm_tm_prepare_acts_kernel for many agents as the samples, lstm_tm_prepare_acts_dev_kernel
//             for their windows in the caller's device memory), then per step and layer
//             lstm_tm_fwd_kernel: workgroup = 16 samples x 16 cells, its four wavefronts the four gates (16 x 16 x K on
//             v_mfma_f32_16x16x4_f32: A tile staged in LDS with 16-byte loads, W columns as 64-byte runs from the L2); epilogue =
//             the cell (Layer_LSTM.h:77-125), the rows kept for the backward pass and the dW launch, this step's block output into the
//             next layer's input row, this step's output into the next step's recurrent input
//   backward  (the deltas of the rows a sample does not have were zeroed by the prepare launch), then ONE launch per step (last first) and layer
//             (top first), lstm_tm_bwd_kernel: [error to the block below | error to the previous step] = D[r] W^T, 16 samples x 16
//             rows of W per workgroup, the reduction over the 4 nC deltas split over the four wavefronts (both operands as 16-byte
//             loads, the reduction index permuted inside groups of 16); its epilogue forms the cell deltas (Layer_LSTM.h:127-165)
//             whose inputs the product completes
// The windows carry one row more per sample than nnBPTTseq + 1 (RecArgs::K): a truncated episode's next state is step T + 1 of its
// window like any other (forward only; its deltas are zero).  Weight gradients: the common dW launch over all rows, as before.
// The LSTM, MGU and plain RNN kernels are built from the same pieces, each written once:
//   forward   tmActiveMask / tmAnyActive (samples that have the step), tmLoadW + tmColumnProduct (a wavefront's W column x the A tile),
//             tmStageA (the A tile into LDS), tmStorePartial, tmHandOn (next step's recurrent slot, the layer above's row or Yout)
//   backward  tmDeltaProduct (a wavefront's part of D W^T), tmJoinPartials, tmFinishTile (whose cell deltas the tile completes, and the
//             hand-off between the two producers of a tile at the arrival counter -- the protocol and its reasoning stand there)
// A kernel keeps what is its own: how its wavefronts split columns and reduction, the loads it requests early, its cell.
#include <type_traits>
#include "rec_dev.h"
#include "act_win_geo.h"

namespace hl {

constexpr int TM_LDA = 4;      // padding of the staged A tile's rows (floats)

// window geometry of every sample + the first layer's input rows + zero recurrent input at the first step + zero deltas for the rows a
// sample does not have: a workgroup per (sample, window row) -- a workgroup per sample walked its eighteen rows one after the other (13 us)
__global__ __launch_bounds__(256) void lstm_tm_prepare_kernel(RecArgs a) {
  const int b = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const int t = a.bt.t[b]; const long long slot = a.bt.slot[b];
  const int T = min(a.nBPTT, t), nextRow = a.bt.nextOf[b];
  const int nSteps = T + 1 + (nextRow >= 0 ? 1 : 0);
  const long long r = (long long)b * a.K + k;
  // the backward launches tell the first of a tile's two producers from the second by the parity of an arrival counter: zeroed here, in
  // front of every window, so that a launch that never completed (device fault, failed replay) cannot leave a parity behind that would
  // make every later step pair values of different steps
  if (b == 0 && k == 0) for (int i = tid; i < a.tmCtrN; i += 256) a.tmCtr[i] = 0u;
  if (k == 0) {
    if (tid == 0) { a.tmT[b] = T; a.tmSteps[b] = nSteps; a.tmNext[b] = nextRow; }
    for (int j = 0; j < a.nL; ++j) {
      const RecLayer& L = a.L[j];
      for (int c = tid; c < L.nC; c += 256) L.A[r * L.ldA + L.nIn + c] = 0.f;
    }
  }
  if (k < nSteps) {
    const RecLayer& L0 = a.L[0];
    for (int i = tid; i < L0.nIn; i += 256) L0.A[r * L0.ldA + i] = recInputAt(a, false, b, slot, t, T, nextRow, k, i);
  }
  if (k > T) {      // rows a sample does not have (the next state's row included): zero deltas -- their stale inputs add nothing to the gradients
    for (int j = 0; j < a.nL; ++j) {
      const RecLayer& L = a.L[j];
      for (int o = tid; o < a.gates * L.nC; o += 256) L.D[r * a.gates * L.nC + o] = 0.f;
      if (L.hasRes) for (int c = tid; c < L.nC; c += 256) L.Rd[r * L.ldR + c] = 0.f;
    }
  }
}

// rollout inference of nets whose layers are wider than the per-sample kernels hold (256 cells): the agent's window as ONE sample of the
// time-step-major launches -- its geometry, the first layer's input rows from the given states, zero recurrent input at its first step
__global__ __launch_bounds__(256) void lstm_tm_prepare_act_kernel(RecArgs a) {
  const int tid = threadIdx.x, T = a.actSteps - 1;
  if (tid == 0) { a.tmT[0] = T; a.tmSteps[0] = T + 1; a.tmNext[0] = -1; }
  const RecLayer& L0 = a.L[0];
  const int dIn = L0.nIn;
  for (int e = tid; e < (T + 1) * dIn; e += 256) {
    const int k = e / dIn, i = e - k * dIn;
    L0.A[(size_t)k * L0.ldA + i] = recInputAt(a, true, 0, 0, 0, T, -1, k, i);
  }
  for (int j = 0; j < a.nL; ++j) {
    const RecLayer& L = a.L[j];
    for (int c = tid; c < L.nC; c += 256) L.A[L.nIn + c] = 0.f;
  }
}

// ... and the windows of a.B agents as the a.B samples of ONE chain of launches (hl_forward_sequences): a workgroup per (agent, window
// step), as lstm_tm_prepare_kernel.  Agent b's actCnt[b] states start at state actOff[b] of actStates (both tables and the states in mapped
// pinned memory); the last nBPTT + 1 of them are its window, those in front only feed appended observations.  The forward kernels leave
// out an agent whose window has ended (tmActiveMask) and hand its last step's block output to Yout row b (tmHandOn); a row of a longer
// window of the chunk before is never read: rows k >= tmSteps[b] feed no sum of agent b, and every row k < tmSteps[b] is written here
// (inputs) or by step k - 1 (recurrent slot) first.
__global__ __launch_bounds__(256) void lstm_tm_prepare_acts_kernel(RecArgs a) {
  const int b = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const int steps = a.actCnt[b], win = min(steps, a.nBPTT + 1), ctx = steps - win;
  const long long r = (long long)b * a.K + k;
  if (k == 0) {
    if (tid == 0) { a.tmT[b] = win - 1; a.tmSteps[b] = win; a.tmNext[b] = -1; }
    for (int j = 0; j < a.nL; ++j) {
      const RecLayer& L = a.L[j];
      for (int c = tid; c < L.nC; c += 256) L.A[r * L.ldA + L.nIn + c] = 0.f;
    }
  }
  if (k < win) {
    const RecLayer& L0 = a.L[0];
    const float* states = a.actStates + (size_t)a.actOff[b] * a.dS;
    // (behind convolutions: the agents' feature rows, step k of agent b at row b K + k, written by the launches in front)
    if (a.Xin) { for (int i = tid; i < L0.nIn; i += 256) L0.A[r * L0.ldA + i] = a.Xin[r * a.ldXin + i]; }
    else
    for (int i = tid; i < L0.nIn; i += 256) L0.A[r * L0.ldA + i] = recActInputAt(a, states, ctx, k, i);
  }
}

// ... and its twin for windows in the CALLER's device memory (hl_forward_sequences_dev): agent b's states are rows of a strided rollout
// buffer, t.nSteps[b] of them from row t.firstRow[b] on; the kernel forms the window itself (act_win_geo: the newest nBPTT + 1 + nApp
// states, one where the count is below 1) and reads, truncates and standardises it on the way into L0.A -- recActInputAt's expression on
// the same values, so the rows are the host route's bit for bit.  The host does not know the windows, so the grid and the chain behind it
// cover nBPTT + 1 steps whatever they are; rows k >= win are left as they are: the product multiplies them row by row into rows of P that
// no epilogue reads, the chain's tiles mask them (tmActiveMask).
// VEC: dS is a multiple of 4 and the states, the mean and the scale are 16-byte aligned -- every state row then starts on a 16-byte
// boundary, as every row of L0.A does.  TM_PD pieces per lane are requested before the first is used: a row of 8192 floats is 32 pieces
// of 16 bytes per lane, one dependent round trip each otherwise
constexpr int TM_PD = 4;
template <bool VEC>
__device__ __forceinline__ void tmPrepareActsDev(const RecArgs& a, const TmActDev& t) {
  using V = typename std::conditional<VEC, f32x4, float>::type;
  constexpr int W = VEC ? 4 : 1;
  const int b = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const ActWinGeo g = act_win_geo(t.nSteps[b], a.nBPTT + 1, a.nApp);
  const long long r = (long long)b * a.K + k;
  if (k == 0) {
    if (tid == 0) { a.tmT[b] = g.win - 1; a.tmSteps[b] = g.win; a.tmNext[b] = -1; }
    for (int j = 0; j < a.nL; ++j) {
      const RecLayer& L = a.L[j];
      for (int c = tid; c < L.nC; c += 256) L.A[r * L.ldA + L.nIn + c] = 0.f;
    }
  }
  if (k >= g.win) return;
  const RecLayer& L0 = a.L[0];
  const long long first = t.firstRow[b];
  const int dS = a.dS, nP = L0.nIn / W;      // (VEC: dS and with it nIn = dS (1 + nApp) are multiples of 4, a piece lies inside one state)
  float* dst = L0.A + r * L0.ldA;
  for (int p0 = tid; p0 < nP; p0 += TM_PD * 256) {
    V x[TM_PD], m[TM_PD], s[TM_PD];
#pragma unroll
    for (int u = 0; u < TM_PD; ++u) {
      const int e = min(p0 + 256 * u, nP - 1) * W, i = e % dS;
      const float* src = a.actStates + act_win_row(g, first, t.rowStride, act_win_state(g, k, e, dS)) * dS + i;
      x[u] = *reinterpret_cast<const V*>(src);
      m[u] = *reinterpret_cast<const V*>(a.rp.stMean + i);
      s[u] = *reinterpret_cast<const V*>(a.rp.stScale + i);
    }
#pragma unroll
    for (int u = 0; u < TM_PD; ++u) {
      const int p = p0 + 256 * u;
      if (p < nP) *reinterpret_cast<V*>(dst + p * W) = (x[u] - m[u]) * s[u];
    }
  }
}
__global__ __launch_bounds__(256) void lstm_tm_prepare_acts_dev_kernel(RecArgs a, TmActDev t, int vec) {
  if (vec) tmPrepareActsDev<true>(a, t); else tmPrepareActsDev<false>(a, t);
}

// ---- what the three forward kernels share --------------------------------------------------------------------------------------------
// 512 threads: eight wavefronts that split a 16-cell tile's gate columns and the reduction over [W_in; W_rec] between them (per kernel)
constexpr int TM_FNT = 512;
constexpr int TM_UN = 16;      // rows of a W column a wavefront has in flight (one batch of the forward product)
constexpr int TM_UG = 8;       // groups of 16 deltas a wavefront has in flight in the backward product

// which of the workgroup's 16 samples have window step k; read back behind the staging barrier (tmAnyActive, the epilogues)
__device__ __forceinline__ void tmActiveMask(int* sAct, const RecArgs& a, int b0, int k, int tid) {
  if (tid < 16) sAct[tid] = (b0 + tid < a.B && a.tmSteps[b0 + tid] > k) ? 1 : 0;
}
__device__ __forceinline__ bool tmAnyActive(const int* sAct) {
  bool any = false;
#pragma unroll
  for (int i = 0; i < 16; ++i) any = any || sAct[i] != 0;
  return any;
}
// the A tile: rows r = b K + k of 16 samples, Kt floats each, into sA[16][lds] in 16-byte pieces; zeros behind Kt.
//   REC_ELSEWHERE = false   the row is [input | previous output] of L.A (its pitch is a multiple of 16 floats): 16-byte loads
//   REC_ELSEWHERE = true    the recurrent part comes from rec[r ldRec + .] (MGU phase 1: A2; no alignment of its pitch is asked
//                           for by tmLayersOk): element by element
//   REC_ONLY (wide inputs)  the tile is the recurrent part alone, Kt = nC floats of rec[r ldRec + .]: the first layer's input product
//                           comes from tm_win_product_kernel (nIn need not be a multiple of 4: element by element as well)
template <bool REC_ELSEWHERE, bool REC_ONLY = false>
__device__ __forceinline__ void tmStageA(float* sA, int lds, const RecArgs& a, const RecLayer& L, const float* rec, int ldRec, int Kt, int Kt4, int b0, int k, int tid) {
  const int q4 = Kt4 >> 2;
  for (int i = tid; i < 16 * q4; i += TM_FNT) {
    const int row = i / q4, q = i - row * q4, b = min(b0 + row, a.B - 1);
    f32x4 v;
    if constexpr (REC_ELSEWHERE) {
      const long long r = (long long)b * a.K + k;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int x = 4 * q + e;
        if constexpr (REC_ONLY) v[e] = x < Kt ? rec[r * ldRec + x] : 0.f;
        else v[e] = x < L.nIn ? L.A[r * L.ldA + x] : (x < Kt ? rec[r * ldRec + (x - L.nIn)] : 0.f);
      }
    } else {
      v = *reinterpret_cast<const f32x4*>(L.A + ((size_t)b * a.K + k) * L.ldA + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) if (4 * q + e >= Kt) v[e] = 0.f;
    }
    *reinterpret_cast<f32x4*>(sA + row * lds + 4 * q) = v;
  }
}
// a batch of a wavefront's W column Wg (row pitch `pitch`): rows 4 (s + u) + lc (rows behind Kt: a valid row, the A element is zero).
// The kernels request the first batch in front of the A tile.
__device__ __forceinline__ void tmLoadW(float (&bv)[TM_UN], const float* Wg, int pitch, int s, int lc, int Kt) {
#pragma unroll
  for (int u = 0; u < TM_UN; ++u) { const int i = min(4 * (s + u) + lc, Kt - 1); bv[u] = Wg[(size_t)i * pitch]; }
}
// sum over the wavefront's slices [sBeg, sEnd) of the reduction (four rows each) of A tile x W column, on v_mfma_f32_16x16x4_f32; bv = the
// first batch; ar = sA + li lds + lc.  Element q of the result = sample 4 lc + q, cell li.  PREFETCH: the next batch flies during this
// one's MFMAs (LSTM, RNN); else it is requested in front of its own (MGU: an eighth of the reduction per wavefront, seldom a second batch)
template <bool PREFETCH>
__device__ __forceinline__ f32x4 tmColumnProduct(float (&bv)[TM_UN], const float* Wg, int pitch, const float* ar, int sBeg, int sEnd, int lc, int Kt) {
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int s0 = sBeg; s0 < sEnd; s0 += TM_UN) {
    float bn[TM_UN];
    const bool more = PREFETCH && s0 + TM_UN < sEnd;
    if (more) tmLoadW(bn, Wg, pitch, s0 + TM_UN, lc, Kt);
    if (!PREFETCH && s0 > sBeg) tmLoadW(bv, Wg, pitch, s0, lc, Kt);
#pragma unroll
    for (int u = 0; u < TM_UN; ++u) {
      const float av = s0 + u < sEnd ? ar[4 * (s0 + u)] : 0.f;
      if (u & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[u], acc1, 0, 0, 0);
      else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[u], acc0, 0, 0, 0);
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < TM_UN; ++u) bv[u] = bn[u];
    }
  }
  return acc0 + acc1;
}
// the wavefront's partial tile into sG[8][16][17]
__device__ __forceinline__ void tmStorePartial(float* sG, const f32x4& p, int wave, int lc, int li) {
#pragma unroll
  for (int q = 0; q < 4; ++q) sG[(wave * 16 + 4 * lc + q) * 17 + li] = p[q];
}
// where the output of (layer j, step k, sample b, cell c) goes, r = b K + k: the next step's recurrent slot; with the parametric residual
// (ParametricResidualLayer::forward, Layers.h:347-361; the layer's input from the staged row sArow) the layer above's input row of the
// same step, or Yout at the sample's last step T / at the next state's step T + 1.  wr, br = the residual's parameters of cell c (zero without)
__device__ __forceinline__ void tmHandOn(const RecArgs& a, const RecLayer& L, int j, int k, int b, int c, long long r, float out, const float* sArow, float wr, float br, int steps, int T) {
  float blk = out;
  if (L.hasRes && c < L.resW) blk += sArow[c] * wr + br;
  if (k + 1 < steps) L.A[(r + 1) * L.ldA + L.nIn + c] = out;          // the next step's recurrent input
  if (j + 1 < a.nL) { const RecLayer& U = a.L[j + 1]; U.A[r * U.ldA + c] = blk; }      // the layer above, same step
  else {
    if (k == T) a.Yout[(size_t)b * a.ldY + c] = blk;
    else if (k == T + 1) a.Yout[(size_t)a.tmNext[b] * a.ldY + c] = blk;
  }
}

// ---- what the three backward kernels share -------------------------------------------------------------------------------------------
// A launch is one ANTI-DIAGONAL of the (layer, step) grid -- blockIdx.z picks (j0 + z, k0 - z) -- and a workgroup forms, for 16 samples and 16
// rows i of [W_in; W_rec], e[b][i] = sum_o D[r][o] W[i][o] (Layer::backward, Layers.h:123-188); the deltas of a step a sample does not have
// are zero rows (lstm_tm_prepare_kernel).  Each of the four wavefronts reduces over its own range of n deltas (tmDeltaProduct), the four
// partial tiles meet in LDS (tmJoinPartials), and the epilogue forms the cell deltas whose inputs the product completes (tmFinishTile).

// this wavefront's part of D W^T: dq = its n deltas of sample row li, wq = the same columns of W row li (n a multiple of 4).  Both operands
// come straight from memory: whole groups of 16 as 16-byte loads, the reduction index permuted inside a group (lane group lc takes
// o = 16 G + 4 lc + e in sub-step e), TM_UG groups in flight; the rest four per lane group (element 16 nG + 4 e + lc in sub-step e).
// KEEP: the W operand times `keep` (MGU phase 1: recurrent rows take the forget deltas only)
template <bool KEEP>
__device__ __forceinline__ f32x4 tmDeltaProduct(const float* wq, const float* dq, int n, int lc, float keep = 1.f) {
  auto w = [&](float x) { if constexpr (KEEP) return x * keep; else return x; };
  const f32x4* wr = reinterpret_cast<const f32x4*>(wq) + lc;
  const f32x4* dr = reinterpret_cast<const f32x4*>(dq) + lc;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const int nG = n >> 4, rem = n & 15;
  for (int g0 = 0; g0 < nG; g0 += TM_UG) {
    f32x4 wv[TM_UG], dv[TM_UG];
#pragma unroll
    for (int u = 0; u < TM_UG; ++u) { const int G = min(g0 + u, nG - 1); wv[u] = wr[4 * G]; dv[u] = dr[4 * G]; }
#pragma unroll
    for (int u = 0; u < TM_UG; ++u) {
      if (g0 + u < nG) {      // A = deltas (rows = samples), B = W rows (columns = rows i of W)
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u][0], w(wv[u][0]), acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u][1], w(wv[u][1]), acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u][2], w(wv[u][2]), acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u][3], w(wv[u][3]), acc1, 0, 0, 0);
      }
    }
  }
  for (int e = 0; 4 * e < rem; ++e) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(dq[16 * nG + 4 * e + lc], w(wq[16 * nG + 4 * e + lc]), acc0, 0, 0, 0);
  return acc0 + acc1;
}
// the four wavefronts' partial tiles through sR[4][256]: thread tid's element (sample row tid >> 4, W row tid & 15)
__device__ __forceinline__ float tmJoinPartials(float* sR, const f32x4& p, int wave, int lc, int li, int tid) {
#pragma unroll
  for (int q = 0; q < 4; ++q) sR[wave * 256 + (4 * lc + q) * 16 + li] = p[q];
  __syncthreads();
  return (sR[tid] + sR[256 + tid]) + (sR[512 + tid] + sR[768 + tid]);
}
// The end of a backward workgroup of (layer j, step k) whose 16 rows of W start at i0.  Its tile of errors -- thread = (sample b with last
// step T, row i = i0 + tid % 16) -- is one of the two inputs of the deltas of a tile of cells (J, Kc), the same for the whole workgroup
// (layer inputs and cells come in multiples of 16):
//   rows i <  nIn (j > 0)   eBelow + residual path = the error of the block below at THIS step: the error from above of the deltas of (j - 1, k)
//   rows i >= nIn           eRec = the error handed to step k - 1: the last layer forms its deltas of (j, k - 1) at once (its error from above
//                           is the head's gradient at the sample's last step, else zero); for the other layers it is the second input of
//                           the deltas of (j, k - 1), whose first one comes from the launch (j + 1, k - 1) -- a member of the SAME diagonal.
// Delta(a, J, Kc, b, c, T, eTop, eRec) forms and stores the deltas of one cell.  Deltas formed on diagonal e are the operands of diagonal
// e - 1: 18 launches instead of 34 at two layers and 17 steps.  Launch (nL - 1, nBPTT + 1) -- a step no sample has -- starts the chain with
// the last layer's deltas of step nBPTT.
template <void (*Delta)(const RecArgs&, int, int, int, int, int, float, float)>
__device__ __forceinline__ void tmFinishTile(const RecArgs& a, int j, int k, int i0, int b, int i, int T, float eBelow, float eRec, unsigned& sArr) {
  const RecLayer& L = a.L[j];
  const int nIn = L.nIn;
  const bool below = i0 < nIn;
  const int J = below ? j - 1 : j, Kc = below ? k : k - 1, c = below ? i : i - nIn;
  const int nCJ = a.L[J].nC;
  const bool live = b < a.B && c < nCJ && T >= Kc;      // (this sample has step Kc: its rows of deltas exist)
  float v = below ? eBelow : eRec;
  if (below && L.hasRes && i < L.resW && b < a.B) v += L.Rd[((size_t)b * a.K + k) * L.ldR + i] * a.W[L.indWr + i];
  if (!below && j == a.nL - 1) {      // the last layer's deltas of the previous step: nothing else feeds them
    if (live) Delta(a, j, Kc, b, c, T, Kc == T ? a.Dres[(size_t)b * a.ldD + c] : 0.f, v);
    return;
  }
  // the other producer of these deltas -- (j - 1, k + 1) for a tile below, (j + 1, k - 1) else -- is a member of this diagonal, unless it
  // would lie behind the windows: no launch of the layer below there, these deltas have one producer
  if (below && k + 1 > a.nBPTT) {
    if (live) Delta(a, J, Kc, b, c, T, v, 0.f);
    return;
  }
  // The two producers meet at an arrival counter per (layer, 16 cells, 16 samples): the first leaves its values, the second reads them
  // and forms the deltas (the pattern of dw_wide_kernel's row quarters); the result does not depend on who arrives first.
  // Hand-off without a release / acquire pair, on purpose: the ONLY data that changes hands are these values, written by agent-scope
  // atomic stores -- which go to the coherence point themselves -- and acknowledged (vmcnt(0)) BEFORE the arrival is counted; the second
  // producer reads them back with agent-scope atomic loads.  A release here would write back this XCD's whole L2: ~15 us.  First and
  // second are told apart by the counter's parity: every counter gets exactly two arrivals per step, and lstm_tm_prepare_kernel zeroes
  // them in front of every window, so a launch that never completed cannot leave a parity behind.
  float* mine = below ? a.tmET[J] : a.tmER[J];
  const float* other = below ? a.tmER[J] : a.tmET[J];
  const size_t at = (size_t)min(b, a.B - 1) * nCJ + min(c, nCJ - 1);
  if (b < a.B && c < nCJ) __hip_atomic_store(mine + at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __builtin_amdgcn_s_waitcnt(0);          // vmcnt(0): this tile's values are at the coherence point
  __syncthreads();
  const int cTile = (below ? i0 : i0 - nIn) >> 4;
  if (threadIdx.x == 0) sArr = __hip_atomic_fetch_add(a.tmCtr + a.tmCtrOff[J] + cTile * (int)gridDim.y + (int)blockIdx.y, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if ((sArr & 1u) == 0u) return;          // the first of the two
  const float o = __hip_atomic_load(other + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (live) Delta(a, J, Kc, b, c, T, below ? v : o, below ? o : v);
}

// ---- LSTM layers (Network/Layers/Layer_LSTM.h:77-166) -------------------------------------------------------------------------------
// forward of layer j at window step k: samples with tmSteps[b] > k.  Wavefront w = gate (w & 3) x half (w >> 2) of the reduction.
// One launch = one DIAGONAL of the (layer, step) grid: blockIdx.z picks (j0 + z, k0 - z) -- layer j at step k needs layer j - 1 at step k
// and its own step k - 1, both on the diagonal in front, so a window of K steps through nL layers is K + nL - 1 launches instead of K nL
// (what they write into a shared row -- the block output of the layer below, the recurrent input of the step before -- are different columns)
// WIN (wide inputs, tm_win_lstm_fwd_kernel): the FIRST layer's tile is the recurrent part of the row alone -- its wavefronts reduce over W_rec,
// and the cell adds the row of the input product P (tm_win_product_kernel) beside the bias; the layers above are the code below as it stands.
// A flag of the kernel, as RecActWin<MANY> and tmStageA<REC_ELSEWHERE>: without it nothing of this is compiled
template <bool WIN>
__device__ __forceinline__ void tmLstmForward(const RecArgs& a, int j0, int k0) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int j = j0 + (int)blockIdx.z, k = k0 - (int)blockIdx.z;
  const RecLayer& L = a.L[j];
  if ((int)blockIdx.x * 16 >= L.nC) return;      // (the grid is as wide as the diagonal's widest layer)
  // development time stamps (-DHL_TM_STAMPS, tools/tm_stamps.py): the last layer's workgroup (0, 0) at window step 5
#ifdef HL_TM_STAMPS
#define TMSTMP(i) do { if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && j == a.nL - 1 && k == 5) a.sc->dbgT[i] = wall_clock64(); } while (0)
#else
#define TMSTMP(i) do { } while (0)
#endif
  TMSTMP(0);
  const int nIn = L.nIn, nC = L.nC, NO = 4 * nC;
  bool win = false;                      // this member of the diagonal takes its input product from P
  if constexpr (WIN) win = j == 0;
  const int Kt = win ? nC : nIn + nC, Kt4 = (Kt + 3) & ~3, lds = Kt4 + TM_LDA;
  float* sA = sm;                        // [16][lds]
  float* sG = sA + 16 * lds;             // [8][16][17]
  __shared__ int sAct[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  const int b0 = blockIdx.y * 16, c0 = blockIdx.x * 16;
  tmActiveMask(sAct, a, b0, k, tid);
  // this wavefront's W column (gate, cell li) over its half of the rows [W_in; W_rec] (WIN, first layer: of W_rec): the first batch is requested in front of the A tile
  const int gate = wave & 3, half = wave >> 2;
  const int nS = Kt4 >> 2, nSh = (nS + 1) >> 1, sBeg = half * nSh, sEnd = min(nS, sBeg + nSh);
  const float* Wg = a.W + L.indW + (win ? (size_t)nIn * NO : (size_t)0) + (size_t)gate * nC + c0 + li;
  float bv[TM_UN];
  tmLoadW(bv, Wg, NO, sBeg, lc, Kt);
  // what the cell's epilogue reads from memory -- the four biases, the state of the step before, the window's length: requested here, used
  // behind the products (a load issued there is a round trip of its own at the end of every launch of the chain)
  const int eRow = (tid >> 4) & 15, eC = c0 + (tid & 15), eB = min(b0 + eRow, a.B - 1);
  const float* Bi = a.W + L.indB;
  const long long eR = (long long)eB * a.K + k;
  const float bi0 = Bi[eC], bi1 = Bi[nC + eC], bi2 = Bi[2 * nC + eC], bi3 = Bi[3 * nC + eC];
  const float prevStE = k > 0 ? L.Y[(eR - 1) * NO + nC + eC] : 0.f;
  const int stepsE = a.tmSteps[eB], TE = a.tmT[eB];
  float wrE = 0.f, brE = 0.f;
  if (L.hasRes && eC < L.resW) { wrE = a.W[L.indWr + eC]; brE = a.W[L.indBr + eC]; }
  // (P rows of steps a sample does not have hold whatever the product made of stale inputs: read for the samples that have the step only)
  float pE0 = 0.f, pE1 = 0.f, pE2 = 0.f, pE3 = 0.f;
  if constexpr (WIN) if (win && b0 + eRow < a.B && stepsE > k) {
    const float* Pr = a.tmP + eR * NO + eC;
    pE0 = Pr[0]; pE1 = Pr[nC]; pE2 = Pr[2 * nC]; pE3 = Pr[3 * nC];
  }
  if (win) tmStageA<true, true>(sA, lds, a, L, L.A + nIn, L.ldA, Kt, Kt4, b0, k, tid);
  else
  tmStageA<false>(sA, lds, a, L, nullptr, 0, Kt, Kt4, b0, k, tid);
  TMSTMP(1);
  __syncthreads();
  TMSTMP(2);
  if (!tmAnyActive(sAct)) return;
  tmStorePartial(sG, tmColumnProduct<true>(bv, Wg, NO, sA + li * lds + lc, sBeg, sEnd, lc, Kt), wave, lc, li);
  TMSTMP(3);
  __syncthreads();
  TMSTMP(4);
  // the cell of (sample row, cell c): Layer_LSTM.h:77-125
  if (tid >= 256) return;
  const int row = tid >> 4, cc = tid & 15, b = b0 + row, c = c0 + cc;
  if (!sAct[row]) return;
  const long long r = (long long)b * a.K + k;
  auto gsum = [&](int g) { return sG[(g * 16 + row) * 17 + cc] + sG[((4 + g) * 16 + row) * 17 + cc]; };
  auto pre = [&](int g, float bi, float p) { if constexpr (WIN) return (gsum(g) + p) + bi; else return gsum(g) + bi; };      // (WIN, layers above the first: p = 0)
  const float ci = pre(0, bi0, pE0);
  const float ig = recSigm(pre(1, bi1, pE1));
  const float fg = recSigm(pre(2, bi2, pE2));
  const float og = recSigm(pre(3, bi3, pE3));
  const float st = ci * ig + prevStE * fg;
  const float co = actEval(HL_FUNC_TANH, st);
  const float out = og * co;
  L.X[r * NO + c] = ci; L.X[r * NO + nC + c] = ig; L.X[r * NO + 2 * nC + c] = fg; L.X[r * NO + 3 * nC + c] = og;
  L.Y[r * NO + c] = out; L.Y[r * NO + nC + c] = st; L.Y[r * NO + 2 * nC + c] = co;
  // (the product route stages the recurrent part alone: a first layer with a residual -- behind convolutions -- reads its input from the operand row)
  tmHandOn(a, L, j, k, b, c, r, out, win ? L.A + r * L.ldA : sA + row * lds, wrE, brE, stepsE, TE);
  TMSTMP(5);
}
__global__ __launch_bounds__(TM_FNT) void lstm_tm_fwd_kernel(RecArgs a, int j0, int k0) { tmLstmForward<false>(a, j0, k0); }
__global__ __launch_bounds__(TM_FNT) void tm_win_lstm_fwd_kernel(RecArgs a, int j0, int k0) { tmLstmForward<true>(a, j0, k0); }
// the cell's deltas of (layer j, step k, sample b, cell c), Layer_LSTM.h:127-165: eTop = error from the block above (same step), eRec = error
// handed back by step k + 1 (zero at the sample's last step)
__device__ __forceinline__ void tmDelta(const RecArgs& a, int j, int k, int b, int c, int T, float eTop, float eRec) {
  const RecLayer& L = a.L[j];
  const int nC = L.nC, NO = 4 * nC;
  const long long r = (long long)b * a.K + k;
  if (L.hasRes) L.Rd[r * L.ldR + c] = eTop;
  const float D = eTop + (k < T ? eRec : 0.f);
  const float ci = L.X[r * NO + c], ig = L.X[r * NO + nC + c], fg = L.X[r * NO + 2 * nC + c], og = L.X[r * NO + 3 * nC + c];
  const float co = L.Y[r * NO + 2 * nC + c];
  const float prevSt = k > 0 ? L.Y[(r - 1) * NO + nC + c] : 0.f;
  const float diff = (1.f - co * co) * D;
  const float sd = diff * og + (k < T ? a.tmSD[j][(size_t)b * nC + c] * L.X[(r + 1) * NO + 2 * nC + c] : 0.f);
  L.D[r * NO + c] = ig * sd;
  L.D[r * NO + nC + c] = ig * (1.f - ig) * ci * sd;
  L.D[r * NO + 2 * nC + c] = k > 0 ? fg * (1.f - fg) * prevSt * sd : 0.f;
  L.D[r * NO + 3 * nC + c] = og * (1.f - og) * D * co;
  a.tmSD[j][(size_t)b * nC + c] = sd;
}
// backward of layer j at step k, samples with T >= k - 1: wavefront w reduces over gate w's nC deltas
__global__ __launch_bounds__(256) void lstm_tm_bwd_kernel(RecArgs a, int j0, int k0) {
  __shared__ float sR[4 * 256];
  __shared__ int sT[16];
  __shared__ unsigned sArr;
  const int j = j0 + (int)blockIdx.z, k = k0 - (int)blockIdx.z;
  if (k == a.nBPTT + 1 && j != a.nL - 1) return;      // (only the last layer has a launch at the step behind the windows)
  const RecLayer& L = a.L[j];
  const int nIn = L.nIn, nC = L.nC, NO = 4 * nC;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  const int row0 = j > 0 ? 0 : nIn;      // (no error below the first layer)
  const int b0 = blockIdx.y * 16, i0 = row0 + blockIdx.x * 16;
  if (i0 >= nIn + (k > 0 ? nC : 0)) return;      // (the grid is as wide as the diagonal's widest member; no error to a step in front of the first)
  if (tid < 16) sT[tid] = b0 + tid < a.B ? a.tmT[b0 + tid] : -2;
  const int iw = min(i0 + li, nIn + nC - 1), bl = min(b0 + li, a.B - 1);
  __builtin_assume((nC & 15) == 0);      // (tmLayersOk: a gate's deltas are whole groups of 16, tmDeltaProduct's rest is empty)
  const f32x4 p = tmDeltaProduct<false>(a.W + L.indW + (size_t)iw * NO + wave * nC, L.D + ((size_t)bl * a.K + k) * NO + wave * nC, nC, lc);
  const float e = tmJoinPartials(sR, p, wave, lc, li, tid);      // (zero for a sample without step k)
  tmFinishTile<tmDelta>(a, j, k, i0, b0 + (tid >> 4), i0 + (tid & 15), sT[tid >> 4], e, e, sArr);
}

// ---- MGU layers (Network/Layers/Layer_GRU.h:64-231), the same arrangement ------------------------------------------------------------
//   forget f = sigm(b_f + W_ff in + W_fr prevOut),  state s = tanh(b_s + W_sf in + W_sr (f * prevOut)),  output = f s + (1 - f) prevOut
// The state's recurrent term needs the forget gates of ALL cells: two products per (layer, step) --
//   forward   phase 0: columns [0, nC) over [in | prevOut]       -> f, and the row A2 = f * prevOut (the dW operand of W_sr)
//             phase 1: columns [nC, 2 nC) over [in | A2]          -> s, the output, the rows of the next layer / next step
//   backward  phase 0: fp = dS W_sr^T (reduction over the state deltas)        -> dF = ((s - p) dLdO + fp p) f (1 - f)
//             phase 1: [error below | g] = [dF | dS] W_in^T  |  dF W_fr^T      -> error of the block below; error to step k - 1 =
//                      (1 - f) dLdO + f fp + g.  Its epilogue forms dLdO and dS of the cell whose inputs it completes (as the LSTM
//                      kernel does): the block below at this step, the last layer at the previous step
// W is [nIn + nC][2 nC] (forget columns first); rows kept per (sample, step): X = [f | s], Y = output, D = [dF | dS].
template <bool WIN>      // (wide inputs: tmLstmForward; both phases have an input term)
__device__ __forceinline__ void tmMguForward(const RecArgs& a, int j0, int k0, int phase) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int j = j0 + (int)blockIdx.z, k = k0 - (int)blockIdx.z;      // (a diagonal per launch: lstm_tm_fwd_kernel)
  const RecLayer& L = a.L[j];
  if ((int)blockIdx.x * 16 >= L.nC) return;
  const int nIn = L.nIn, nC = L.nC, NO = 2 * nC;
  bool win = false;
  if constexpr (WIN) win = j == 0;
  const int nInS = win ? 0 : nIn;        // input columns in front of the recurrent part of the staged row
  const int Kt = nInS + nC, Kt4 = (Kt + 3) & ~3, lds = Kt4 + TM_LDA;
  float* sA = sm;                        // [16][lds]
  float* sG = sA + 16 * lds;             // [8][16][17]
  __shared__ int sAct[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  const int b0 = blockIdx.y * 16, c0 = blockIdx.x * 16;
  tmActiveMask(sAct, a, b0, k, tid);
  // wavefront w: an eighth of the rows [W_in; W_rec] (WIN, first layer: of W_rec) of column (phase, cell li)
  const int nS = Kt4 >> 2, nSe = (nS + 7) >> 3, sBeg = wave * nSe, sEnd = min(nS, sBeg + nSe);
  const float* Wg = a.W + L.indW + (win ? (size_t)nIn * NO : (size_t)0) + (size_t)phase * nC + c0 + li;
  float bv[TM_UN];
  tmLoadW(bv, Wg, NO, sBeg, lc, Kt);
  // A tile: [in | prevOut] (phase 0) or [in | f * prevOut] (phase 1)
  if (win) tmStageA<true, true>(sA, lds, a, L, phase ? L.A2 : L.A + nIn, phase ? L.ldA2 : L.ldA, Kt, Kt4, b0, k, tid);
  else
  tmStageA<true>(sA, lds, a, L, phase ? L.A2 : L.A + nIn, phase ? L.ldA2 : L.ldA, Kt, Kt4, b0, k, tid);
  __syncthreads();
  if (!tmAnyActive(sAct)) return;
  tmStorePartial(sG, tmColumnProduct<false>(bv, Wg, NO, sA + li * lds + lc, sBeg, sEnd, lc, Kt), wave, lc, li);
  __syncthreads();
  if (tid >= 256) return;
  const int row = tid >> 4, cc = tid & 15, b = b0 + row, c = c0 + cc;
  if (!sAct[row]) return;
  float sum = a.W[L.indB + phase * nC + c];
  if constexpr (WIN) if (win) sum += a.tmP[((long long)b * a.K + k) * NO + phase * nC + c];      // (behind sAct: a row of a step this sample has)
#pragma unroll
  for (int w = 0; w < 8; ++w) sum += sG[(w * 16 + row) * 17 + cc];
  const long long r = (long long)b * a.K + k;
  const float po = sA[row * lds + nInS + c];     // phase 0: prevOut; phase 1: f * prevOut
  if (phase == 0) {
    const float f = recSigm(sum);
    L.X[r * NO + c] = f;
    L.A2[r * L.ldA2 + c] = po * f;
    return;
  }
  const float st = actEval(HL_FUNC_TANH, sum);
  L.X[r * NO + nC + c] = st;
  const float f = L.X[r * NO + c], prev = L.A[r * L.ldA + nIn + c];
  const float out = k > 0 ? f * st + (1.f - f) * prev : f * st;
  L.Y[r * NO + c] = out;
  float wr = 0.f, br = 0.f;
  if (L.hasRes && c < L.resW) { wr = a.W[L.indWr + c]; br = a.W[L.indBr + c]; }
  tmHandOn(a, L, j, k, b, c, r, out, win ? L.A + r * L.ldA : sA + row * lds, wr, br, a.tmSteps[b], a.tmT[b]);
}
__global__ __launch_bounds__(TM_FNT) void mgu_tm_fwd_kernel(RecArgs a, int j0, int k0, int phase) { tmMguForward<false>(a, j0, k0, phase); }
__global__ __launch_bounds__(TM_FNT) void tm_win_mgu_fwd_kernel(RecArgs a, int j0, int k0, int phase) { tmMguForward<true>(a, j0, k0, phase); }
// dLdO and the state delta of (layer j, step k, sample b, cell c): eTop = error from the block above, eRec = error handed back by step k + 1
__device__ __forceinline__ void tmMguOpen(const RecArgs& a, int j, int k, int b, int c, int T, float eTop, float eRec) {
  const RecLayer& L = a.L[j];
  const int nC = L.nC, NO = 2 * nC;
  const long long r = (long long)b * a.K + k;
  if (L.hasRes) L.Rd[r * L.ldR + c] = eTop;
  const float dLdO = eTop + (k < T ? eRec : 0.f);
  const float f = L.X[r * NO + c], st = L.X[r * NO + nC + c];
  a.tmSD[j][(size_t)b * nC + c] = dLdO;
  L.D[r * NO + nC + c] = dLdO * f * (1.f - st * st);
}
// (a launch is one anti-diagonal of the (layer, step) grid and one phase)
__global__ __launch_bounds__(256) void mgu_tm_bwd_kernel(RecArgs a, int j0, int k0, int phase) {
  __shared__ float sR[4 * 256];
  __shared__ int sT[16];
  __shared__ unsigned sArr;
  const int j = j0 + (int)blockIdx.z, k = k0 - (int)blockIdx.z, top = a.nL - 1;
  if (k == a.nBPTT + 1 && (j != top || phase == 0)) return;      // (behind the windows: the last layer's phase 1 only -- it starts the chain)
  const RecLayer& L = a.L[j];
  const int nIn = L.nIn, nC = L.nC, NO = 2 * nC;
  if (phase == 0 ? (int)blockIdx.x * 16 >= nC : (j > 0 ? 0 : nIn) + (int)blockIdx.x * 16 >= nIn + (k > 0 ? nC : 0)) return;      // (the grid is as wide as the diagonal's widest member)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  const int b0 = blockIdx.y * 16, row = tid >> 4, b = b0 + row;
  if (tid < 16) sT[tid] = b0 + tid < a.B ? a.tmT[b0 + tid] : -2;
  const int bl = min(b0 + li, a.B - 1);
  const float* dRow = L.D + ((size_t)bl * a.K + k) * NO;
  if (phase == 0) {
    // fp[b][c] = sum_o dS[b][o] W[nIn + c][nC + o]: the four wavefronts a quarter of the nC state deltas each (k == 0: no recurrent input, fp = 0)
    const int c0 = blockIdx.x * 16, q = nC >> 2;
    f32x4 p = {0.f, 0.f, 0.f, 0.f};
    if (k > 0) p = tmDeltaProduct<false>(a.W + L.indW + (size_t)(nIn + c0 + li) * NO + nC + wave * q, dRow + nC + wave * q, q, lc);
    const float sum = tmJoinPartials(sR, p, wave, lc, li, tid);
    const int c = c0 + (tid & 15), T = sT[row];
    if (T < k) return;
    const float fp = k > 0 ? sum : 0.f;
    const long long r = (long long)b * a.K + k;
    const float f = L.X[r * NO + c], st = L.X[r * NO + nC + c], pO = k > 0 ? L.Y[(r - 1) * NO + c] : 0.f;
    const float dLdO = a.tmSD[j][(size_t)b * nC + c];
    a.tmFP[j][(size_t)b * nC + c] = fp;
    L.D[r * NO + c] = ((st - pO) * dLdO + fp * pO) * f * (1.f - f);
    return;
  }
  // phase 1: rows i of [W_in; W_rec]: i < nIn reduce over [dF | dS] (wavefronts 0, 1 the forget half, 2, 3 the state half), i >= nIn over dF only
  const int i0 = (j > 0 ? 0 : nIn) + blockIdx.x * 16, iw = min(i0 + li, nIn + nC - 1);
  const int h = nC >> 1;                                      // deltas per wavefront: half of a gate's
  const float keep = (wave >= 2 && i0 + li >= nIn) ? 0.f : 1.f;      // (recurrent rows take the forget deltas only)
  const f32x4 p = tmDeltaProduct<true>(a.W + L.indW + (size_t)iw * NO + wave * h, dRow + wave * h, h, lc, keep);
  const float e = tmJoinPartials(sR, p, wave, lc, li, tid);      // (zero for a sample without step k)
  const int i = i0 + (tid & 15), T = sT[row];
  float eRec = 0.f;      // the error handed to step k - 1 by a recurrent tile
  if (i0 >= nIn && b < a.B && i - nIn < nC && T >= k) {
    const long long r = (long long)b * a.K + k;
    const int c = i - nIn;
    const float f = L.X[r * NO + c];
    eRec = (1.f - f) * a.tmSD[j][(size_t)b * nC + c] + f * a.tmFP[j][(size_t)b * nC + c] + e;
  }
  tmFinishTile<tmMguOpen>(a, j, k, i0, b, i, T, e, eRec, sArr);
}

// ---- plain RNN layers (nnType "RNN": BaseLayer with bRecurrent, Network/Layers/Layer_Base.h:64-113), the same arrangement ----------
//   y_t = f(b + W_in x_t + W_rec y_{t-1}):  one gate, the epilogue is the activation.  W is [nIn + nC][nC]; rows kept per (sample,
//   step): X = pre-activation, Y = output, D = delta -- the rows rec.hip's rnn_forward_kernel keeps, so the taps, the head and the dW
//   launch see nothing new.
// Tile shape of the forward kernel: a workgroup = 16 samples x TWO 16-cell tiles, its eight wavefronts = tile (w & 1) x quarter (w >> 1)
// of the reduction over [W_in; W_rec].  With one gate the LSTM kernel's "wavefront = gate" has no meaning; what a workgroup pays before
// its first MFMA is the staging of the A tile (16 rows x (nIn + nC) floats -- as many bytes as ONE tile's W columns), so the staged tile
// serves two cell tiles (half as many workgroups restage it), and the reduction is split four ways so that a wavefront's chain of
// dependent W batches stays short ((nIn + nC) / 64 loads of 16 rows: 3 at 2 x 272 cells, 8 at 2 x 1024).  Four tiles x two halves -- the
// LSTM kernel's 64 columns per workgroup -- would leave 5 x 8 workgroups per (layer, step) at 272 cells and batch 128 for 256 CUs and double
// that chain; one tile x eight eighths (the MGU kernel) restages A per 16 cells.  A layer with an odd number of tiles (272 = 17 x 16) has
// one workgroup whose second tile does not exist: its wavefronts run on clamped columns and write nothing.
// Measured with this shape (profiles/rnn_tm_timing.json): the forward chain of 2 x 272 cells, batch 128, 18 steps takes 186 us,
// of 2 x 512 cells 239 us -- 3.5 x the operations for 28 % more time, so at these sizes the dependent launches set the time and not the
// product.  The other two shapes were not built: the choice between them rests on the arithmetic above.
constexpr int RNN_TM_TILES = 2;
template <bool WIN>      // (wide inputs: tmLstmForward)
__device__ __forceinline__ void tmRnnForward(const RecArgs& a, int j0, int k0) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int j = j0 + (int)blockIdx.z, k = k0 - (int)blockIdx.z;      // (a diagonal per launch: lstm_tm_fwd_kernel)
  const RecLayer& L = a.L[j];
  if ((int)blockIdx.x * 16 * RNN_TM_TILES >= L.nC) return;           // (the grid is as wide as the diagonal's widest layer)
  const int nIn = L.nIn, nC = L.nC;
  bool win = false;
  if constexpr (WIN) win = j == 0;
  const int Kt = win ? nC : nIn + nC, Kt4 = (Kt + 3) & ~3, lds = Kt4 + TM_LDA;
  float* sA = sm;                        // [16][lds]
  float* sG = sA + 16 * lds;             // [8][16][17]
  __shared__ int sAct[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  const int b0 = blockIdx.y * 16, cBase = blockIdx.x * 16 * RNN_TM_TILES;
  tmActiveMask(sAct, a, b0, k, tid);
  // this wavefront's W column (tile, cell li) over its quarter of the rows [W_in; W_rec]: the first batch is requested in front of the A tile
  const int tile = wave & 1, quarter = wave >> 1;
  const int nS = Kt4 >> 2, nSq = (nS + 3) >> 2, sBeg = quarter * nSq, sEnd = min(nS, sBeg + nSq);
  const float* Wg = a.W + L.indW + (win ? (size_t)nIn * nC : (size_t)0) + min(cBase + 16 * tile, nC - 16) + li;      // (W's row pitch is nC: a multiple of 16)
  float bv[TM_UN];
  tmLoadW(bv, Wg, nC, sBeg, lc, Kt);
  // what the epilogue reads from memory: requested here, used behind the products (lstm_tm_fwd_kernel)
  const int eTile = tid >> 8, eRow = (tid >> 4) & 15, eC = cBase + 16 * eTile + (tid & 15), eB = min(b0 + eRow, a.B - 1);
  const bool eOk = eC < nC;
  const float biE = eOk ? a.W[L.indB + eC] : 0.f;
  const int stepsE = a.tmSteps[eB], TE = a.tmT[eB];
  float wrE = 0.f, brE = 0.f;
  if (L.hasRes && eC < L.resW) { wrE = a.W[L.indWr + eC]; brE = a.W[L.indBr + eC]; }
  float pE = 0.f;      // (read for the samples that have the step only: tmLstmForward)
  if constexpr (WIN) if (win && eOk && b0 + eRow < a.B && stepsE > k) pE = a.tmP[((long long)eB * a.K + k) * nC + eC];
  if (win) tmStageA<true, true>(sA, lds, a, L, L.A + nIn, L.ldA, Kt, Kt4, b0, k, tid);
  else
  tmStageA<false>(sA, lds, a, L, nullptr, 0, Kt, Kt4, b0, k, tid);
  __syncthreads();
  if (!tmAnyActive(sAct)) return;
  tmStorePartial(sG, tmColumnProduct<true>(bv, Wg, nC, sA + li * lds + lc, sBeg, sEnd, lc, Kt), wave, lc, li);
  __syncthreads();
  // BaseLayer::forward of (sample row, cell c): thread = (tile, row, cell)
  const int row = eRow, cc = tid & 15, b = b0 + row, c = eC;
  if (!eOk || !sAct[row]) return;
  const long long r = (long long)b * a.K + k;
  auto part = [&](int q) { return sG[((RNN_TM_TILES * q + eTile) * 16 + row) * 17 + cc]; };
  float x;
  if constexpr (WIN) x = biE + (((part(0) + part(1)) + (part(2) + part(3))) + pE); else x = biE + ((part(0) + part(1)) + (part(2) + part(3)));
  const float out = actEval(a.func, x);
  L.X[r * nC + c] = x; L.Y[r * nC + c] = out;
  tmHandOn(a, L, j, k, b, c, r, out, sA + row * lds, wrE, brE, stepsE, TE);
}
__global__ __launch_bounds__(TM_FNT) void rnn_tm_fwd_kernel(RecArgs a, int j0, int k0) { tmRnnForward<false>(a, j0, k0); }
__global__ __launch_bounds__(TM_FNT) void tm_win_rnn_fwd_kernel(RecArgs a, int j0, int k0) { tmRnnForward<true>(a, j0, k0); }
// the delta of (layer j, step k, sample b, cell c), BaseLayer::backward (Layer_Base.h:97-113): eTop = error from the block above (same step),
// eRec = error handed back by step k + 1 (zero at the sample's last step) -- as rnn_backward_kernel forms it
__device__ __forceinline__ void tmRnnDelta(const RecArgs& a, int j, int k, int b, int c, int T, float eTop, float eRec) {
  const RecLayer& L = a.L[j];
  const int nC = L.nC;
  const long long r = (long long)b * a.K + k;
  if (L.hasRes) L.Rd[r * L.ldR + c] = eTop;
  const float D = eTop + (k < T ? eRec : 0.f);
  L.D[r * nC + c] = D * actDiff(a.func, L.X[r * nC + c], L.Y[r * nC + c]);
}
// lstm_tm_bwd_kernel with one gate: the four wavefronts split the reduction over the nC deltas into quarters (nC / 4 is a multiple of 4,
// not of 16: tmDeltaProduct's rest)
__global__ __launch_bounds__(256) void rnn_tm_bwd_kernel(RecArgs a, int j0, int k0) {
  __shared__ float sR[4 * 256];
  __shared__ int sT[16];
  __shared__ unsigned sArr;
  const int j = j0 + (int)blockIdx.z, k = k0 - (int)blockIdx.z;
  if (k == a.nBPTT + 1 && j != a.nL - 1) return;      // (only the last layer has a launch at the step behind the windows)
  const RecLayer& L = a.L[j];
  const int nIn = L.nIn, nC = L.nC;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  const int row0 = j > 0 ? 0 : nIn;      // (no error below the first layer)
  const int b0 = blockIdx.y * 16, i0 = row0 + blockIdx.x * 16;
  if (i0 >= nIn + (k > 0 ? nC : 0)) return;      // (the grid is as wide as the diagonal's widest member; no error to a step in front of the first)
  if (tid < 16) sT[tid] = b0 + tid < a.B ? a.tmT[b0 + tid] : -2;
  const int iw = min(i0 + li, nIn + nC - 1), bl = min(b0 + li, a.B - 1);
  const int q = nC >> 2;                 // deltas per wavefront
  const f32x4 p = tmDeltaProduct<false>(a.W + L.indW + (size_t)iw * nC + wave * q, L.D + ((size_t)bl * a.K + k) * nC + wave * q, q, lc);
  const float e = tmJoinPartials(sR, p, wave, lc, li, tid);      // (zero for a sample without step k)
  tmFinishTile<tmRnnDelta>(a, j, k, i0, b0 + (tid >> 4), i0 + (tid & 15), sT[tid >> 4], e, e, sArr);
}

// ---- wide inputs: the first layer's input product of a whole forward pass as ONE launch -------------------------------------------------
//   P[r][o] = sum_{i < nIn} A0[r][i] W_in[i][o],   o < gates nC,   r = b K + k for b < nB, k < nK
// (training: every row of the windows; acting: the given steps of one window or of a chunk's agents).  The forward tiles stage the whole
// operand row of 16 samples in LDS, which bounds nIn + nC; here the rows the prepare launch left in HBM are read in slices of 32
// columns instead: a workgroup = 64 rows x 64 columns, wavefront w its rows 16 w .. 16 w + 15 over the four column tiles
// (v_mfma_f32_16x16x4_f32, gemm_tile.h's operand conventions: A element = (row li, k = 4 s + lc), B element = (k = 4 s + lc, column li),
// result element q = (row 4 lc + q, column li)), the next slice in registers while this one's products run.  An element of P is one chain
// of MFMAs over i = 0 .. nIn - 1 whatever its row's place in the launch: a window's rows come out the same alone and among others.
// Nothing behind nIn is read in a row of A (the recurrent part belongs to the chain), nothing behind row nIn of W (W_rec), and rows past
// nB nK are clamped on the way in and masked on the way out.  Rows of steps a sample does not have are computed from whatever their
// inputs hold and never read (the forward kernels' epilogues).
constexpr int WP_T = 64, WP_KC = 32, WP_PA = WP_KC + 4, WP_PB = 80;
__global__ __launch_bounds__(256) void tm_win_product_kernel(RecArgs a, int nB, int nK) {
  __shared__ __attribute__((aligned(16))) float sA[WP_T * WP_PA], sB[WP_KC * WP_PB];
  const RecLayer& L = a.L[0];
  const int nIn = L.nIn, NO = a.gates * L.nC, nRows = nB * nK;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  const int n0 = blockIdx.x * WP_T, m0 = blockIdx.y * WP_T;
  const float* Wb = a.W + L.indW;
  // a slice = 64 rows x 32 columns of A (thread: rows tid / 8 and + 32, four columns from 4 (tid % 8)) and 32 rows x 64 columns of W_in
  // (rows tid / 16 and + 16, four columns from 4 (tid % 16))
  const int ar0 = tid >> 3, ac = (tid & 7) * 4, wr0 = tid >> 4, wc = (tid & 15) * 4;
  const float* aRow[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int ri = min(m0 + ar0 + 32 * q, nRows - 1), b = ri / nK, k = ri - b * nK;
    aRow[q] = L.A + ((size_t)b * a.K + k) * L.ldA;
  }
  const bool wIn = n0 + wc < NO;      // (NO is a multiple of 16: a 16-byte piece is inside the row or behind it)
  f32x4 va[2], vw[2];
  auto loadSlice = [&](int i0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int x = i0 + ac, i = i0 + wr0 + 16 * q;
      va[q] = f32x4{0.f, 0.f, 0.f, 0.f}; vw[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (x + 3 < nIn) va[q] = *reinterpret_cast<const f32x4*>(aRow[q] + x);      // (the rows' pitch is a multiple of 16 floats)
      else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (x + e < nIn) va[q][e] = aRow[q][x + e];
      }
      if (wIn && i < nIn) vw[q] = *reinterpret_cast<const f32x4*>(Wb + (size_t)i * NO + n0 + wc);
    }
  };
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4] = {z4, z4, z4, z4};
  const float* ar = sA + (16 * wave + li) * WP_PA + lc;
  const float* br = sB + lc * WP_PB + li;
  loadSlice(0);
  for (int i0 = 0; i0 < nIn; i0 += WP_KC) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      *reinterpret_cast<f32x4*>(sA + (ar0 + 32 * q) * WP_PA + ac) = va[q];
      *reinterpret_cast<f32x4*>(sB + (wr0 + 16 * q) * WP_PB + wc) = vw[q];
    }
    __syncthreads();
    if (i0 + WP_KC < nIn) loadSlice(i0 + WP_KC);
#pragma unroll
    for (int s = 0; s < WP_KC / 4; ++s) {
      const float av = ar[4 * s];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, br[4 * s * WP_PB + 16 * t], acc[t], 0, 0, 0);
    }
    __syncthreads();      // (the slice's readers are through before the next one is stored)
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int ri = m0 + 16 * wave + 4 * lc + q;
    if (ri >= nRows) continue;
    const int b = ri / nK, k = ri - b * nK;
    float* Pr = a.tmP + ((size_t)b * a.K + k) * NO;
#pragma unroll
    for (int t = 0; t < 4; ++t) { const int o = n0 + 16 * t + li; if (o < NO) Pr[o] = acc[t][q]; }
  }
}

// ---- convolutions in front: the gradient into the feature rows, the mirror of the product above ---------------------------------------
//   Dres[r][i] = sum_{o < gates nC} D[r][o] W_in[i][o]  (+ Rd[r][i] w_res[i], i < resN),   D2[r][i] = Dres[r][i] act'(X[r][i], Y[r][i])
// for every window row r < M and input i < N: the GEMM_X / EPI_DX problem of the step's table (step_exec.h: buildProblems), whose record
// this kernel reads as it stands -- A = the first recurrent layer's gate deltas [M][K], B = W_in [N][ldb], C / C2 = Dres / D of the last
// convolution's rows, resIn / resW the parametric-residual path, actX / actY / func the convolution's activation.  gemm16.hip's form of
// it stages an operand row per sample; here both operands come in slices of 32 gate columns: a workgroup = 64 rows x 64 inputs, a slice =
// 64 x 32 of D and 64 x 32 of W_in (both read along the gate columns, 16 bytes per load: K and both pitches are multiples of 4), wavefront
// w its rows 16 w .. 16 w + 15 over the four input tiles, the next slice in registers while this one's products run.  An element is one
// chain of MFMAs over o = 0 .. K - 1 whatever its row's place in the launch.  Rows past M and inputs past N are clamped on the way in and
// masked on the way out; rows of steps a sample does not have hold zero deltas (lstm_tm_prepare_kernel) and come out zero.
constexpr int WX_T = 64, WX_KC = 32, WX_P = WX_KC + 4;
__global__ __launch_bounds__(256) void tm_conv_dx_kernel(GemmProblem P) {
  __shared__ __attribute__((aligned(16))) float sD[WX_T * WX_P], sW[WX_T * WX_P];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  const int n0 = blockIdx.x * WX_T, m0 = blockIdx.y * WX_T;
  // a slice: rows tid / 8 and + 32 of either operand, four gate columns from 4 (tid % 8)
  const int r0 = tid >> 3, oc = (tid & 7) * 4;
  const float* dRow[2]; const float* wRow[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    dRow[q] = P.A + (size_t)min(m0 + r0 + 32 * q, P.M - 1) * P.lda;
    wRow[q] = P.B + (size_t)min(n0 + r0 + 32 * q, P.N - 1) * P.ldb;
  }
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 vd[2], vw[2];
  auto loadSlice = [&](int o0) {
    const bool in = o0 + oc < P.K;      // (K is a multiple of 4: a 16-byte piece is inside the row or behind it)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      vd[q] = in ? *reinterpret_cast<const f32x4*>(dRow[q] + o0 + oc) : z4;
      vw[q] = in ? *reinterpret_cast<const f32x4*>(wRow[q] + o0 + oc) : z4;
    }
  };
  f32x4 acc[4] = {z4, z4, z4, z4};
  const float* ar = sD + (16 * wave + li) * WX_P + lc;      // A element = (row li of the wavefront's 16, k = 4 s + lc)
  const float* br = sW + li * WX_P + lc;                    // B element = (k = 4 s + lc, input li of tile t): W_in's row read along its columns
  loadSlice(0);
  for (int o0 = 0; o0 < P.K; o0 += WX_KC) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      *reinterpret_cast<f32x4*>(sD + (r0 + 32 * q) * WX_P + oc) = vd[q];
      *reinterpret_cast<f32x4*>(sW + (r0 + 32 * q) * WX_P + oc) = vw[q];
    }
    __syncthreads();
    if (o0 + WX_KC < P.K) loadSlice(o0 + WX_KC);
#pragma unroll
    for (int s = 0; s < WX_KC / 4; ++s) {
      const float av = ar[4 * s];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, br[16 * t * WX_P + 4 * s], acc[t], 0, 0, 0);
    }
    __syncthreads();      // (the slice's readers are through before the next one is stored)
  }
  // result element q = (row 4 lc + q, input li of tile t): EPI_DX (gemm_tile.h) on it
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int m = m0 + 16 * wave + 4 * lc + q;
    if (m >= P.M) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int n = n0 + 16 * t + li;
      if (n >= P.N) continue;
      float dres = acc[t][q];
      if (n < P.resN) dres += P.resIn[(size_t)m * P.ldRes + n] * P.resW[n];
      P.C[(size_t)m * P.ldc + n] = dres;
      P.C2[(size_t)m * P.ldc + n] = dres * actDiff(P.func, P.actX[(size_t)m * P.ldAct + n], P.actY[(size_t)m * P.ldAct + n]);
    }
  }
}
bool tm_conv_dx_ok(const GemmProblem& p) {
  auto aligned = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  return p.flavor == GEMM_X && p.epi == EPI_DX && p.M >= 1 && p.N >= 1 && p.K >= 4 && (p.K & 3) == 0 && (p.lda & 3) == 0 && (p.ldb & 3) == 0 &&
         p.lda >= p.K && p.ldb >= p.K && aligned(p.A) && aligned(p.B) && p.C && p.C2 && p.actX && p.actY && (p.resN == 0 || (p.resIn && p.resW));
}
hipError_t launch_tm_conv_dx(const GemmProblem& p, hipStream_t s) {
  if (!tm_conv_dx_ok(p)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tm_conv_dx_kernel, dim3((p.N + WX_T - 1) / WX_T, (p.M + WX_T - 1) / WX_T), dim3(256), 0, s, p);
  return hipGetLastError();
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
static bool tmGatesOk(const RecArgs& a) { return a.gates == 4 || a.gates == 2 || a.gates == 1; }
// (wide inputs -- RecArgs::tmP --: the first layer's tile is the recurrent part of the row alone)
static size_t tmFwdLds(const RecArgs& a, int j) { const RecLayer& L = a.L[j]; return (size_t)(16 * ((((a.tmP && j == 0 ? 0 : L.nIn) + L.nC + 3) & ~3) + TM_LDA) + 8 * 16 * 17) * 4; }
static bool tmLayersOk(const RecArgs& a) {
  for (int j = 0; j < a.nL; ++j) {
    const RecLayer& L = a.L[j];
    if (L.nC % 16 || L.indW % 4 || (L.ldA & 3) || (j > 0 && L.nIn != a.L[j - 1].nC)) return false;
    if (a.gates == 2 && a.tmFP[j] == nullptr) return false;
    if (tmFwdLds(a, j) > 150 * 1024) return false;
  }
  // the input product: 16-byte pieces of the operand rows, nothing wider than the bound hl_create states.  The first layer's input is the
  // raw states or (Xin, convolutions in front) the feature rows the prepare launch copies into the operand rows; a residual on it -- it
  // has one behind convolutions only -- reads its input from the operand row (the forward kernels' hand-off)
  if (a.tmP && ((a.L[0].ldA & 15) || a.L[0].nIn > TM_WIN_MAX_IN || a.L[0].nC > 1024)) return false;
  if (a.Xin != nullptr && a.tmP == nullptr) return false;      // (rows from launches in front: the product route only)
  return true;
}
// acting (one window of a.actSteps given states, or with the per-agent tables a.B windows of up to a.actSteps) through the same launches:
// used where a layer is wider than the per-sample kernels hold, or the input wider than they stage (tmP)
bool rec_tm_act_ok(const RecArgs& a) {
  const bool many = a.actOff != nullptr && a.actCnt != nullptr;
  if ((a.actOff != nullptr) != (a.actCnt != nullptr) || (many ? a.B < 1 || a.actSteps > a.nBPTT + 1 : a.B != 1)) return false;
  if (!tmGatesOk(a) || a.actStates == nullptr || a.tmSteps == nullptr || a.YoutRows != nullptr || a.actSteps < 1 || a.actSteps > a.K) return false;      // (Xin: tmLayersOk)
  bool wide = a.tmP != nullptr;
  for (int j = 0; j < a.nL; ++j) wide = wide || a.L[j].nC > 256;
  return wide && tmLayersOk(a);
}
bool rec_tm_ok(const RecArgs& a) {
  if (!tmGatesOk(a) || a.actStates != nullptr || a.tmSteps == nullptr || a.YoutRows != nullptr || a.DresRows != nullptr || a.K < a.nBPTT + 2) return false;
  return tmLayersOk(a);
}
// the forward chain: diagonal d of the (layer, step) grid = layers jLo .. jLo + nz - 1 at steps d - j, kLast = the last window step any
// sample can have; a workgroup covers `tiles` tiles of 16 cells; launch(grid, dynamic LDS bytes, jLo, k of jLo) enqueues a diagonal
template <class Launch>
static hipError_t tmForwardDiagonals(const RecArgs& a, int kLast, const void* kernel, int tiles, Launch launch) {
  size_t ldsMax = 0;
  for (int j = 0; j < a.nL; ++j) ldsMax = std::max(ldsMax, tmFwdLds(a, j));
  hipError_t e = ensureDynLds(kernel, ldsMax); if (e != hipSuccess) return e;
  for (int d = 0; d <= kLast + a.nL - 1; ++d) {
    const int jLo = std::max(0, d - kLast), jHi = std::min(a.nL - 1, d);
    int gx = 0; size_t lds = 0;
    for (int j = jLo; j <= jHi; ++j) { gx = std::max(gx, a.L[j].nC / 16); lds = std::max(lds, tmFwdLds(a, j)); }
    launch(dim3((gx + tiles - 1) / tiles, (a.B + 15) / 16, jHi - jLo + 1), lds, jLo, d - jLo);
  }
  return hipGetLastError();
}
// parts: TM_PART_*, for a caller that times them apart; one call with all of them is the pass
hipError_t launch_rec_tm_forward(const RecArgs& a, hipStream_t s, int parts) {
  const bool acting = a.actStates != nullptr;
  const int kLast = acting ? a.actSteps - 1 : a.nBPTT + 1;
  if (parts & TM_PART_PREPARE) {
    if (acting && a.actOff) hipLaunchKernelGGL(lstm_tm_prepare_acts_kernel, dim3(a.B, a.actSteps), dim3(256), 0, s, a);
    else if (acting) hipLaunchKernelGGL(lstm_tm_prepare_act_kernel, dim3(1), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(lstm_tm_prepare_kernel, dim3(a.B, a.K), dim3(256), 0, s, a);
  }
  if (a.tmP && (parts & TM_PART_PRODUCT)) {      // wide inputs: W_in's part of every row's gate sums, in front of the chain
    const int nB = acting && !a.actOff ? 1 : a.B, nK = acting ? a.actSteps : a.K;
    hipLaunchKernelGGL(tm_win_product_kernel, dim3((a.gates * a.L[0].nC + WP_T - 1) / WP_T, (nB * nK + WP_T - 1) / WP_T), dim3(256), 0, s, a, nB, nK);
  }
  if (!(parts & TM_PART_CHAIN)) return hipGetLastError();
  if (a.tmP) {      // ... and the kernels whose first layer takes it from there
    if (a.gates == 2) return tmForwardDiagonals(a, kLast, reinterpret_cast<const void*>(tm_win_mgu_fwd_kernel), 1, [&](dim3 g, size_t lds, int jLo, int k0) {
      for (int ph = 0; ph < 2; ++ph) hipLaunchKernelGGL(tm_win_mgu_fwd_kernel, g, dim3(TM_FNT), lds, s, a, jLo, k0, ph);
    });
    if (a.gates == 1) return tmForwardDiagonals(a, kLast, reinterpret_cast<const void*>(tm_win_rnn_fwd_kernel), RNN_TM_TILES, [&](dim3 g, size_t lds, int jLo, int k0) {
      hipLaunchKernelGGL(tm_win_rnn_fwd_kernel, g, dim3(TM_FNT), lds, s, a, jLo, k0);
    });
    return tmForwardDiagonals(a, kLast, reinterpret_cast<const void*>(tm_win_lstm_fwd_kernel), 1, [&](dim3 g, size_t lds, int jLo, int k0) {
      hipLaunchKernelGGL(tm_win_lstm_fwd_kernel, g, dim3(TM_FNT), lds, s, a, jLo, k0);
    });
  }
  if (a.gates == 2) return tmForwardDiagonals(a, kLast, reinterpret_cast<const void*>(mgu_tm_fwd_kernel), 1, [&](dim3 g, size_t lds, int jLo, int k0) {
    for (int ph = 0; ph < 2; ++ph) hipLaunchKernelGGL(mgu_tm_fwd_kernel, g, dim3(TM_FNT), lds, s, a, jLo, k0, ph);
  });
  if (a.gates == 1) return tmForwardDiagonals(a, kLast, reinterpret_cast<const void*>(rnn_tm_fwd_kernel), RNN_TM_TILES, [&](dim3 g, size_t lds, int jLo, int k0) {
    hipLaunchKernelGGL(rnn_tm_fwd_kernel, g, dim3(TM_FNT), lds, s, a, jLo, k0);
  });
  return tmForwardDiagonals(a, kLast, reinterpret_cast<const void*>(lstm_tm_fwd_kernel), 1, [&](dim3 g, size_t lds, int jLo, int k0) {
    hipLaunchKernelGGL(lstm_tm_fwd_kernel, g, dim3(TM_FNT), lds, s, a, jLo, k0);
  });
}
// the windows of a.B agents from the caller's device memory: the prepare launch that gathers them, then the product and the chain over
// all nBPTT + 1 steps -- after the prepare launch they read tmT / tmSteps / tmNext and the rows of L.A only
hipError_t launch_rec_tm_act_dev(const RecArgs& a, const TmActDev& t, hipStream_t s) {
  if (!a.actStates || !a.actOff || !a.actCnt || !a.tmP || a.actSteps != a.nBPTT + 1 || !t.firstRow || !t.nSteps || t.rowStride < 1) return hipErrorInvalidValue;
  auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const int vec = a.dS % 4 == 0 && aligned(a.actStates) && aligned(a.rp.stMean) && aligned(a.rp.stScale) ? 1 : 0;
  hipLaunchKernelGGL(lstm_tm_prepare_acts_dev_kernel, dim3(a.B, a.actSteps), dim3(256), 0, s, a, t, vec);
  return launch_rec_tm_forward(a, s, TM_PART_PRODUCT | TM_PART_CHAIN);
}
// anti-diagonal j + k = e of the backward chain: its members are layers jLo .. jLo + nz - 1 at steps e - j (behind the windows, k = nBPTT + 1,
// the last layer only); gx1 = grid width of the D W^T launches over the members' rows of W, gx0 = that of MGU's phase 0 over their cells
struct TmAntiDiagonal { int jLo, nz, gx0, gx1; };
static TmAntiDiagonal tmAntiDiagonal(const RecArgs& a, int e) {
  const int jLo = std::max(0, e - (a.nBPTT + 1)), jHi = std::min(a.nL - 1, e);
  TmAntiDiagonal d = {jLo, jHi - jLo + 1, 0, 0};
  for (int j = jLo; j <= jHi; ++j) {
    const int k = e - j;
    if (k == a.nBPTT + 1 && j != a.nL - 1) continue;
    const RecLayer& L = a.L[j];
    const int row0 = j > 0 ? 0 : L.nIn, nOut = L.nIn + (k > 0 ? L.nC : 0) - row0;
    if (k != a.nBPTT + 1) d.gx0 = std::max(d.gx0, L.nC / 16);
    d.gx1 = std::max(d.gx1, (nOut + 15) / 16);
  }
  return d;
}
hipError_t launch_rec_tm_backward(const RecArgs& a, hipStream_t s) {
  for (int e = a.nL - 1 + a.nBPTT + 1; e >= 0; --e) {      // (MGU: phase 0 of every member, then phase 1 of every member)
    const TmAntiDiagonal d = tmAntiDiagonal(a, e);
    const dim3 g0(d.gx0, (a.B + 15) / 16, d.nz), g1(d.gx1, (a.B + 15) / 16, d.nz);
    if (a.gates == 2 && d.gx0 > 0) hipLaunchKernelGGL(mgu_tm_bwd_kernel, g0, dim3(256), 0, s, a, d.jLo, e - d.jLo, 0);
    if (d.gx1 <= 0) continue;
    if (a.gates == 2) hipLaunchKernelGGL(mgu_tm_bwd_kernel, g1, dim3(256), 0, s, a, d.jLo, e - d.jLo, 1);
    else if (a.gates == 1) hipLaunchKernelGGL(rnn_tm_bwd_kernel, g1, dim3(256), 0, s, a, d.jLo, e - d.jLo);
    else hipLaunchKernelGGL(lstm_tm_bwd_kernel, g1, dim3(256), 0, s, a, d.jLo, e - d.jLo);
  }
  return hipGetLastError();
}

}  // namespace hl
