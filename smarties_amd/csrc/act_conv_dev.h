// smarties_amd/csrc/act_conv_dev.h -- device helpers the conv-stack acting kernels share (actconv.hip: act_conv_kernel, act_conv_dev_kernel;
// actband.hip: act_conv_band_dev_kernel): the argument access, a layer as an implicit product on v_mfma_f32_16x16x4_f32 through an offset
// table in LDS, the tables, where a row's raw values lie, the row's load, the stack on the maps in LDS.  The layout of the work and the
// order of a row's sums are described at the head of actconv.hip
#pragma once
#include "dev_common.h"

namespace hl {

constexpr int AC_NPG = 4;      // position tiles per unit of work at most

template <bool VEC>      // K is a multiple of 4 (and the filter 16-byte aligned): a lane's four filter values of a block as one load
__device__ __forceinline__ f32x4 acFilter(const float* __restrict__ wr, int k0, int K, bool chOk) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if constexpr (VEC) { if (chOk && k0 < K) v = *reinterpret_cast<const f32x4*>(wr + k0); }
  else {
#pragma unroll
    for (int w = 0; w < 4; ++w) if (chOk && k0 + w < K) v[w] = wr[k0 + w];
  }
  return v;
}

// The kernels read their one argument through the kernel-argument segment (scalar loads of constant memory) and take the pointer as new
// at every row and every layer: a field is then loaded where it is used, not kept in a scalar register from the kernel's start on.
// (Read as a by-value parameter the fields of all layers and of both load paths stay live together: act_conv_kernel parked 13 scalar
// registers in vector lanes that way, the window kernel 19; now neither parks any.)
typedef const __attribute__((address_space(4))) ActConvArgs* AcArgs;
typedef const __attribute__((address_space(4))) ActConvLayer& AcLayerRef;
__device__ __forceinline__ AcArgs acArgs() { return (AcArgs)__builtin_amdgcn_kernarg_segment_ptr(); }
__device__ __forceinline__ AcArgs acFresh(AcArgs a) { asm volatile("" : "+s"(a)); return a; }

// the output positions [p0, pN) of one layer of one row: sIn -> out (LDS or the row's feature vector), [c][oy][ox].  sIn holds the input
// map from its row oy0 S on (the whole map: oy0 = 0; a band of the first layer: the band's first output row), at the row pitch InX and
// the channel pitch the offset table was built for
template <bool VEC>
__device__ __forceinline__ void acLayerRange(AcLayerRef L, const float* __restrict__ W, const int* sTab, const float* sIn, float* out,
                                             int wave, int li, int lc, int p0, int pN, int oy0) {
  const int K = L.K, P = L.P, KnC = L.KnC;
  const int nPT = (pN - p0 + 15) >> 4, npg = L.npg, nPG = (nPT + npg - 1) / npg, nU = ((KnC + 15) >> 4) * nPG, nB = (K + 15) >> 4;
  const int* tab = sTab + L.tabOff;
  for (int u = wave; u < nU; u += 4) {
    const int ct = u / nPG, pt0 = (u - ct * nPG) * npg, np = min(npg, nPT - pt0);      // (wave-uniform)
    int pb[AC_NPG];      // this lane's output position of tile j: the origin of its patch in the input map
#pragma unroll
    for (int j = 0; j < AC_NPG; ++j) {
      const int pos = p0 + (pt0 + j) * 16 + li, p = (j < np && pos < pN) ? pos : p0, oy = p / L.OpX, ox = p - oy * L.OpX;
      pb[j] = ((oy - oy0) * L.InX + ox) * L.S;
    }
    // the biases of this lane's outputs (channel ct 16 + 4 lc + q, position of tile j), requested in front of the reduction
    float bq[AC_NPG][4];
#pragma unroll
    for (int j = 0; j < AC_NPG; ++j) {
      const int pos = p0 + (pt0 + j) * 16 + li;
#pragma unroll
      for (int q = 0; q < 4; ++q) { const int c = ct * 16 + 4 * lc + q; bq[j][q] = (j < np && pos < pN && c < KnC) ? W[L.indB + (long long)c * P + pos] : 0.f; }
    }
    const int ch = ct * 16 + li; const bool chOk = ch < KnC;
    const float* wr = W + L.indW + (long long)(chOk ? ch : 0) * K;
    f32x4 acc[AC_NPG];
#pragma unroll
    for (int j = 0; j < AC_NPG; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 av = acFilter<VEC>(wr, 4 * lc, K, chOk);
    for (int b = 0; b < nB; ++b) {
      const int k0 = 16 * b + 4 * lc;
      const f32x4 an = b + 1 < nB ? acFilter<VEC>(wr, k0 + 16, K, chOk) : f32x4{0.f, 0.f, 0.f, 0.f};
      const int4 ko = *reinterpret_cast<const int4*>(tab + k0);      // (the table is padded to a multiple of 16 entries)
      const int kk[4] = {ko.x, ko.y, ko.z, ko.w};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const bool kin = k0 + w < K;
#pragma unroll
        for (int j = 0; j < AC_NPG; ++j) if (j < np) {
          const float x = sIn[kk[w] + pb[j]];
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[w], kin ? x : 0.f, acc[j], 0, 0, 0);
        }
      }
      av = an;
    }
#pragma unroll
    for (int j = 0; j < AC_NPG; ++j) if (j < np) {
      const int pos = p0 + (pt0 + j) * 16 + li;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = ct * 16 + 4 * lc + q;
        if (pos < pN && c < KnC) { const float x = acc[j][q] + bq[j][q]; out[c * P + pos] = x / (1 + fabsf(x)); }      // SoftSign (Functions.h)
      }
    }
  }
}
// one layer of one row on its whole input map
template <bool VEC>
__device__ __forceinline__ void acLayer(AcLayerRef L, const float* __restrict__ W, const int* sTab, const float* sIn, float* out,
                                        int wave, int li, int lc) {
  acLayerRange<VEC>(L, W, sTab, sIn, out, wave, li, lc, 0, L.P, 0);
}

// the layers' offset tables k -> ic InY InX + fy InX + fx, once per workgroup (BAND: the first layer's input is a band buffer
// [InC][bandRows][InX], so its channel pitch is bandRows InX)
template <bool BAND = false>
__device__ __forceinline__ void acTables(AcArgs a, int* sTab, int tid) {
  for (int l = 0; l < a->nL; ++l) {
    AcLayerRef L = a->L[l];
    const int fsz = L.KnY * L.KnX, Kp = (L.K + 15) & ~15, rows = (BAND && l == 0) ? a->bandRows : L.InY;
    for (int k = tid; k < Kp; k += 256) {
      int off = 0;
      if (k < L.K) { const int ic = k / fsz, f = k - ic * fsz, fy = f / L.KnX, fx = f - fy * L.KnX; off = (ic * rows + fy) * L.InX + fx; }
      sTab[L.tabOff + k] = off;
    }
  }
}

// where element c of a row's raw values lies (vec: c is a multiple of 4 and four elements are contiguous and 16-byte aligned there)
struct AcRowSrc {      // a row of [n][dIn] (act_conv_kernel)
  const float* p;
  __device__ __forceinline__ const float* at(int c, int) const { return p + c; }
};
struct AcWindowSrc {   // the newest 1 + nAppendedObs states of a strided window (act_conv_dev_kernel): block j of the row is the state max(last - j, 0)
  const float* states; long long first, stride; int last;
  __device__ __forceinline__ const float* at(int c, int dS) const {
    const int j = c / dS, k = c - j * dS;
    return states + (first + (long long)max(last - j, 0) * stride) * dS + k;
  }
};

// the raw row, standardised (Episode::standardizedState, Episode.h:172-183): image -> LDS, extras -> the feature vector's front
template <typename Src>
__device__ __forceinline__ void acLoadRow(AcArgs a, const Src& src, float* sImg, float* fr, int tid) {
  const int img = a->img, dIn = a->dIn, dS = a->dS;
  if (a->vec) {      // dIn, dS and the image are multiples of 4: 16-byte loads, four in flight per thread
    const int n4 = dIn >> 2;
    for (int i0 = 0; i0 < n4; i0 += 1024) {
      f32x4 v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) { const int i = i0 + tid + 256 * q; v[q] = i < n4 ? *reinterpret_cast<const f32x4*>(src.at(4 * i, dS)) : f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + tid + 256 * q;
        if (i < n4) {
          const int c = 4 * i, k = c % dS;
          const f32x4 mean = *reinterpret_cast<const f32x4*>(a->stMean + k), scale = *reinterpret_cast<const f32x4*>(a->stScale + k);
          const f32x4 y = (v[q] - mean) * scale;
          if (c < img) *reinterpret_cast<f32x4*>(sImg + c) = y;
          else {
#pragma unroll
            for (int e = 0; e < 4; ++e) fr[c - img + e] = y[e];
          }
        }
      }
    }
  } else {
    for (int c0 = 0; c0 < dIn; c0 += 1024) {
      float v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) { const int c = c0 + tid + 256 * q; v[q] = c < dIn ? *src.at(c, dS) : 0.f; }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + tid + 256 * q;
        if (c < dIn) {
          const int k = c % dS;
          const float y = (v[q] - a->stMean[k]) * a->stScale[k];
          if (c < img) sImg[c] = y; else fr[c - img] = y;
        }
      }
    }
  }
}

// the conv stack from layer l0 on, on the row in LDS: the maps alternate between the two buffers, the last one goes behind the extras of
// the feature vector (l0 = 0: the first layer reads the image at sImg; l0 = 1: its map has been written, act_conv_band_dev_kernel)
__device__ __forceinline__ void acRowLayers(AcArgs a, const int* sTab, float* sDyn, const float* sImg, float* fr, int wave, int li, int lc, int l0 = 0) {
  const float* __restrict__ W = a->W;
  __syncthreads();
  for (int l = l0; l < a->nL; ++l) {
    a = acFresh(a);
    AcLayerRef L = a->L[l];
    const float* sIn = l == 0 ? sImg : sDyn + a->bufOff[(l - 1) & 1];
    float* out = l == a->nL - 1 ? fr + a->extras : sDyn + a->bufOff[l & 1];
    if (L.vec) acLayer<true>(L, W, sTab, sIn, out, wave, li, lc);
    else acLayer<false>(L, W, sTab, sIn, out, wave, li, lc);
    __syncthreads();      // the map is complete; every wavefront has read its input (the next row's image may take its place)
  }
}

}  // namespace hl
