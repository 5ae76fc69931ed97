// smarties_amd/csrc/act_rows_dev.h -- device helpers the row-block acting kernels share (actrows.hip: act_rows_kernel; actband.hip:
// act_rows_panel_kernel): the product of a block of 16 rows in LDS with a layer's weights on v_mfma_f32_16x16x4_f32, a layer's epilogue, a
// layer in place, the output layer and the block's outputs with their stamp.  The layout of the work and the order of a row's sums are
// described at the head of actrows.hip
#pragma once
#include "dev_common.h"

namespace hl {

constexpr int AR_ROWS = 16;
constexpr int AR_INFLIGHT = 8;      // 16-byte weight loads in flight per lane

// acc[4 u + e][q] += sum_k X[row 4 lc + q][k] * Wl[k][(g0 + u) 64 + 4 li + e] for the wavefront's column groups g0 .. g0 + nu - 1
// (nu <= NG, wave-uniform), k < nIn: the reduction steps s = 0, 1, .. in order on top of what acc holds.  Reduction indices behind nIn: the A
// element is zero and the weight row is the last valid one; column groups starting behind ldW (lanes of the last group when size is no
// multiple of 64): column 0 is read, the result is not used.
template <int NG>
__device__ __forceinline__ void arAccumulate(f32x4 (&acc)[4 * NG], const float* __restrict__ Wl, int ldW, int nIn, const float* sX, int ld,
                                             int g0, int nu, int li, int lc) {
  constexpr int U = AR_INFLIGHT / NG;      // reduction steps per batch of loads
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
// ... from zero
template <int NG>
__device__ __forceinline__ void arProduct(f32x4 (&acc)[4 * NG], const float* __restrict__ Wl, int ldW, int nIn, const float* sX, int ld,
                                          int g0, int nu, int li, int lc) {
#pragma unroll
  for (int i = 0; i < 4 * NG; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  arAccumulate<NG>(acc, Wl, ldW, nIn, sX, ld, g0, nu, li, lc);
}

// the column groups a wavefront takes of a layer `size` wide: g0 .. g0 + nu - 1 (at most NG: the plans)
__device__ __forceinline__ void arGroups(int size, int wave, int& g0, int& nu) {
  const int nGr = (size + 63) >> 6, gpw = (nGr + 3) >> 2;
  g0 = wave * gpw; nu = max(0, min(gpw, nGr - g0));
}

// a layer's epilogue: bias, activation, the parametric residual on the layer's input columns c < resW -- resIn(q, c0): columns c0 .. c0 + 3 of
// the input of row 4 lc + q --, the values into the activations' buffer, 16 bytes per lane and row
template <int NG, class ResIn>
__device__ __forceinline__ void arEpilogue(const f32x4 (&acc)[4 * NG], const ActLayer& L, const float* __restrict__ W, float* sX, int ld,
                                           int g0, int nu, int li, int lc, ResIn resIn) {
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
          const f32x4 in = resIn(q, c0, px);
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
}

// a layer on the block's activations in LDS, its outputs written back IN PLACE behind a barrier (the residual reads its input columns there)
template <int NG>
__device__ __forceinline__ void arLayer(const ActLayer& L, const float* __restrict__ W, float* sX, int ld, int wave, int li, int lc) {
  int g0, nu; arGroups(L.size, wave, g0, nu);      // (nu <= NG: act_rows_plan)
  f32x4 acc[4 * NG];
  arProduct<NG>(acc, W + L.indW, L.ldW, L.nIn, sX, ld, g0, nu, li, lc);
  __syncthreads();      // every wavefront has read the layer's input: the outputs take its place
  arEpilogue<NG>(acc, L, W, sX, ld, g0, nu, li, lc, [](int, int, const f32x4* px) { return *px; });
  __syncthreads();
}

// the output layer (Linear + nnOutputFunc) on the last layer's activations, 4 x 64 columns per pass, a column group per wavefront; then the
// block's output rows, contiguous in memory: nDense doubles, then the nSig ParamLayer values; then the block's stamp
__device__ __forceinline__ void arOutput(const ActRowsArgs& a, const float* __restrict__ W, const float* sX, float* sO, int row0, int rows,
                                         int tid, int wave, int li, int lc) {
  const int ld = a.ld;
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

}  // namespace hl
