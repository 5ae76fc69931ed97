// smarties_amd/csrc/actrows.hip -- rollout inference of DENSE nets for MANY rows in one launch (hl_forward beyond the one-kernel route).
//
//   reference: Approximator::forward(agent) on a feed-forward net (Network/Layers/Layer_Base.h:64-113, the parametric residual of
//   Layers.h:347-361, the ParamLayer), Episode::standardizedState (Episode.h:172-183: appended observations).
//
// act_forward_kernel (misc.hip) runs one row per workgroup with VALU dot products and serves up to 64 rows of nets up to 1024 wide.
// Here a workgroup of 256 threads owns a block of 16 rows and runs the whole net for them on v_mfma_f32_16x16x4_f32:
//   * the raw rows come straight from device-mapped pinned host memory and are standardised on load (rows beyond n: zeros, never read);
//     behind convolutions the rows are act_conv_kernel's feature rows in device memory, standardised already (ActRowsArgs::stMean == nullptr);
//   * the block's activations live in ONE LDS buffer [16][ld] from layer to layer (ld = 4 mod 32: the 64 lanes of an A-operand read
//     -- row lane & 15, reduction index 4 s + (lane >> 4) -- fall on 64 different banks).  A layer's whole output is held in
//     accumulators -- size / 16 tiles spread over the four wavefronts, NG groups of 64 columns each, NG = 1 / 2 / 4 / 8 picked on the
//     host from the widest layer (2048 columns: 128 accumulator registers per lane) -- and written back IN PLACE behind a barrier,
//     so a 2048-wide layer's 16 rows (128 KB) fit without a second buffer;
//   * only weights, biases and residual parameters come from global memory.  A wavefront's B operand of reduction step s is ONE
//     16-byte load per lane and column group: lane li takes columns 4 li .. 4 li + 3 of the group's 64 (rows 4 s + (lane >> 4)), so
//     "tile" e of a group is its columns 4 li + e -- a permutation of the columns inside the group that the epilogue undoes by
//     writing 16 bytes per lane and row.  Eight such loads are in flight per lane while the previous eight feed the MFMAs;
//   * the output layer runs the same product 4 x 64 columns at a time, the values meet in LDS and go to pinned host memory as
//     doubles in row order (a block's rows are contiguous there), the ParamLayer values behind them; then the block's stamp.
// A row's sums: every output column is reduced by one wavefront over s = 0, 1, .. in order, four reduction indices per MFMA --
// the order depends neither on the row's place in its block nor on n.  It is another order than act_forward_kernel's and the
// oracle's: differences at the 1e-7 level.
#include <algorithm>
#include "act_rows_dev.h"

namespace hl {

template <int NG>
__global__ __launch_bounds__(256) void act_rows_kernel(ActRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sDyn[];      // [16][ld] activations | [16][ldO] output-layer values
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  const int ld = a.ld, row0 = blockIdx.x * AR_ROWS, rows = min(AR_ROWS, a.n - row0);
  const float* __restrict__ W = a.W;
  float* sX = sDyn;
  float* sO = sDyn + AR_ROWS * ld;
  // the block's raw rows, standardised (Episode::standardizedState, Episode.h:172-183): a thread takes a column of all 16 rows, sixteen
  // loads from host memory in flight
  {
    const float* src = a.in + (size_t)row0 * a.dIn;
    const bool raw = a.stMean != nullptr;      // (no statistics: rows standardised already -- act_conv_kernel's feature rows; (v - 0) 1 is v)
    for (int c = tid; c < a.dIn; c += 256) {
      const int k = c % a.dS;
      const float mean = raw ? a.stMean[k] : 0.f, scale = raw ? a.stScale[k] : 1.f;
      float v[AR_ROWS];
#pragma unroll
      for (int r = 0; r < AR_ROWS; ++r) v[r] = r < rows ? src[(size_t)r * a.dIn + c] : 0.f;
#pragma unroll
      for (int r = 0; r < AR_ROWS; ++r) sX[r * ld + c] = r < rows ? (v[r] - mean) * scale : 0.f;
    }
  }
  __syncthreads();
  for (int l = 0; l < a.nL; ++l) arLayer<NG>(a.L[l], W, sX, ld, wave, li, lc);
  arOutput(a, W, sX, sO, row0, rows, tid, wave, li, lc);
}

// the kernel serves this net: LDS layout and the accumulator count filled in
constexpr size_t AR_LDS_BUDGET = 160 * 1024;
bool act_rows_plan(ActRowsArgs* a) {
  if (a->nL < 1 || a->nL > HL_MAX_HIDDEN || a->dS < 1 || a->dIn < 1 || a->dIn > ACT_ROWS_MAXW || a->nDense < 1 || a->nSig < 0) return false;
  if (a->L[0].nIn != a->dIn || a->nOut != a->nDense + a->nSig || a->ldWo < a->nDense || (a->ldWo & 3)) return false;
  int maxW = a->dIn;
  for (int j = 0; j < a->nL; ++j) {
    const ActLayer& L = a->L[j];
    if (L.size < 1 || L.size > ACT_ROWS_MAXW || L.nIn < 1 || L.ldW < L.size || (L.ldW & 3) || (L.indW & 3)) return false;
    if (j > 0 && L.nIn != a->L[j - 1].size) return false;
    if (L.hasRes && L.resW > std::min(L.nIn, L.size)) return false;
    maxW = std::max(maxW, L.size);
  }
  if (a->indWo & 3) return false;
  const int gpw = (((maxW + 63) >> 6) + 3) >> 2;      // column groups per wavefront of the widest layer
  a->ng = gpw <= 1 ? 1 : gpw <= 2 ? 2 : gpw <= 4 ? 4 : 8;
  a->ld = ((maxW + 31) & ~31) + 4;
  a->ldO = (a->nDense + 3) & ~3;
  a->ldsBytes = (size_t)AR_ROWS * (a->ld + a->ldO) * sizeof(float);
  return a->ldsBytes <= AR_LDS_BUDGET;
}
template <int NG> static hipError_t actRowsLaunch(const ActRowsArgs& a, hipStream_t s) {
  hipError_t e = ensureDynLds(reinterpret_cast<const void*>(act_rows_kernel<NG>), a.ldsBytes); if (e != hipSuccess) return e;
  hipLaunchKernelGGL((act_rows_kernel<NG>), dim3(act_rows_blocks(a.n)), dim3(256), a.ldsBytes, s, a);
  return hipGetLastError();
}
int act_rows_blocks(int n) { return (n + AR_ROWS - 1) / AR_ROWS; }
hipError_t launch_act_rows(const ActRowsArgs& a, hipStream_t s) {
  if (a.n < 1 || a.ld < 1) return hipErrorInvalidValue;
  switch (a.ng) {
    case 1: return actRowsLaunch<1>(a, s);
    case 2: return actRowsLaunch<2>(a, s);
    case 4: return actRowsLaunch<4>(a, s);
    case 8: return actRowsLaunch<8>(a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace hl
