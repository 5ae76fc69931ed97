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
#include "dev_common.h"

namespace hl {

constexpr int AR_ROWS = 16;
constexpr int AR_INFLIGHT = 8;      // 16-byte weight loads in flight per lane

// acc[4 u + e][q] += sum_k X[row 4 lc + q][k] * Wl[k][(g0 + u) 64 + 4 li + e] for the wavefront's column groups g0 .. g0 + nu - 1
// (nu <= NG, wave-uniform).  Reduction indices behind nIn: the A element is zero and the weight row is the last valid one; column
// groups starting behind ldW (lanes of the last group when size is no multiple of 64): column 0 is read, the result is not used.
template <int NG>
__device__ __forceinline__ void arProduct(f32x4 (&acc)[4 * NG], const float* __restrict__ Wl, int ldW, int nIn, const float* sX, int ld,
                                          int g0, int nu, int li, int lc) {
  constexpr int U = AR_INFLIGHT / NG;      // reduction steps per batch of loads
#pragma unroll
  for (int i = 0; i < 4 * NG; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (nu <= 0) return;
  int colOff[NG];
#pragma unroll
  for (int u = 0; u < NG; ++u) { const int c = (g0 + u) * 64 + 4 * li; colOff[u] = c < ldW ? c : 0; }
  const int nS = (nIn + 3) >> 2;
  auto loadW = [&](f32x4 (&bv)[U][NG], int s0) {
#pragma unroll
    for (int w = 0; w < U; ++w) if (s0 + w < nS) {      // (a batch's steps behind the reduction's end: neither loaded nor multiplied)
      const int k = min(4 * (s0 + w) + lc, nIn - 1);
      const float* row = Wl + (size_t)k * ldW;
#pragma unroll
      for (int u = 0; u < NG; ++u) if (u < nu) bv[w][u] = *reinterpret_cast<const f32x4*>(row + colOff[u]);
    }
  };
  f32x4 bv[U][NG], bn[U][NG];
  loadW(bv, 0);
  const float* ar = sX + li * ld;
  for (int s0 = 0; s0 < nS; s0 += U) {
    const bool more = s0 + U < nS;
    if (more) loadW(bn, s0 + U);
#pragma unroll
    for (int w = 0; w < U; ++w) if (s0 + w < nS) {
      const int k = 4 * (s0 + w) + lc;
      const float av = k < nIn ? ar[k] : 0.f;
#pragma unroll
      for (int u = 0; u < NG; ++u) if (u < nu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * u + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[w][u][e], acc[4 * u + e], 0, 0, 0);
      }
    }
    if (more) {
#pragma unroll
      for (int w = 0; w < U; ++w)
#pragma unroll
        for (int u = 0; u < NG; ++u) bv[w][u] = bn[w][u];
    }
  }
}

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
  for (int l = 0; l < a.nL; ++l) {
    const ActLayer L = a.L[l];
    const int nGr = (L.size + 63) >> 6, gpw = (nGr + 3) >> 2, g0 = wave * gpw, nu = max(0, min(gpw, nGr - g0));      // (gpw <= NG: act_rows_plan)
    f32x4 acc[4 * NG];
    arProduct<NG>(acc, W + L.indW, L.ldW, L.nIn, sX, ld, g0, nu, li, lc);
    __syncthreads();      // every wavefront has read the layer's input: the outputs take its place
    const int resW = L.hasRes ? L.resW : 0;
    dispatchFunc<-1>(L.func, [&](auto F) {
      constexpr int FN = decltype(F)::value;
#pragma unroll
      for (int u = 0; u < NG; ++u) if (u < nu) {
        const int c0 = (g0 + u) * 64 + 4 * li;
        if (c0 < L.size) {
          float b[4], wr[4], br[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int c = c0 + e;
            b[e] = c < L.size ? W[L.indB + c] : 0.f;
            wr[e] = c < resW ? W[L.indWr + c] : 0.f; br[e] = c < resW ? W[L.indBr + c] : 0.f;
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            f32x4* px = reinterpret_cast<f32x4*>(sX + (4 * lc + q) * ld + c0);      // (c0 + 3 < roundUp(size, 4) <= ld)
            const f32x4 in = *px;
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              y[e] = actEvalT<FN>(acc[4 * u + e][q] + b[e]);
              if (c0 + e < resW) y[e] += in[e] * wr[e] + br[e];       // ParametricResidualLayer::forward (Layers.h:347-361)
            }
            *px = y;
          }
        }
      }
    });
    __syncthreads();
  }
  // output layer (Linear + nnOutputFunc): 4 x 64 columns per pass, a column group per wavefront
  {
    const int H = a.L[a.nL - 1].size, nGr = (a.nDense + 63) >> 6, ldO = a.ldO;
    for (int gb = 0; gb < nGr; gb += 4) {
      const int g0 = gb + wave, nu = g0 < nGr ? 1 : 0;
      f32x4 acc[4];
      arProduct<1>(acc, W + a.indWo, a.ldWo, H, sX, ld, g0, nu, li, lc);
      if (nu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = g0 * 64 + 4 * li + e;
          if (c < a.nDense) {
            const float b = W[a.indBo + c];
#pragma unroll
            for (int q = 0; q < 4; ++q) sO[(4 * lc + q) * ldO + c] = actEval(a.outFunc, acc[e][q] + b);
          }
        }
      }
    }
  }
  __syncthreads();
  // the block's output rows, contiguous in host memory: nDense doubles, then the nSig ParamLayer values
  {
    double* dst = a.out + (size_t)row0 * a.nOut;
    const int live = rows * a.nOut;
    for (int e = tid; e < live; e += 256) {
      const int r = e / a.nOut, c = e - r * a.nOut;
      dst[e] = (double)(c < a.nDense ? sO[r * a.ldO + c] : W[a.indBp + (c - a.nDense)]);
    }
  }
  __threadfence_system();
  __syncthreads();
  if (tid == 0) __hip_atomic_store(const_cast<unsigned*>(a.done) + blockIdx.x, a.tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
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
