// smarties_amd/csrc/actconv.hip -- rollout inference of nets with CONVOLUTIONAL layers in front: the whole conv stack of one row per
// workgroup, every map in LDS (hl_forward's route for feed-forward nets behind convolutions; the dense layers behind run in
// act_rows_kernel, actrows.hip, on the feature rows written here).
//
//   reference: Approximator::forward(agent) through Conv2DLayer::forward (Network/Layers/Layer_Conv2D.h:117-138: SoftSign, one bias
//   per output element), the JoinLayer that puts the state variables beside the image in front of the last map (Builder.cpp:26-46,
//   Layers.h:289-299), Episode::standardizedState (Episode.h:172-183: appended observations).
//
// A workgroup of 256 threads owns a row -- one agent's stacked input of dIn raw floats -- and walks on to row blockIdx.x + k gridDim.x:
//   * the raw row comes from device-mapped pinned host memory (the chunk's staging, include/smarties_hip_act.h) and is standardised on load ((v - stMean[c % dS]) stScale[c % dS], the mapping of act_rows_kernel and
//     launch_act_standardize): the image [InC][InY][InX] goes to LDS, the extras behind it to the front of the row's feature vector in
//     device memory, where launch_extras_copy puts them in the training rows;
//   * a layer is an implicit product on v_mfma_f32_16x16x4_f32: A = 16 output channels x 4 reduction indices of the filter, read from the
//     parameter blob in the reference layout K[KnC][InC][KnY][KnX] (NOT the prepared copies of the training kernels: the route is right
//     directly behind hl_set_params / hl_restart); B = 4 reduction indices x 16 output positions, gathered from the input map in LDS
//     through the layer's offset table k -> ic InY InX + fy InX + fx (built once per workgroup) plus the position's base
//     oy S InX + ox S.  Tails -- channels beyond KnC, reduction indices beyond K, positions beyond P -- are zeros on both operands;
//   * a wavefront's unit of work is one tile of 16 channels x up to four tiles of 16 positions (four independent accumulators on one A
//     operand); the units of a layer are dealt to the four wavefronts in turn.  The reduction runs in blocks of 16 indices, lane group
//     lc taking indices 16 b + 4 lc + w in step w: a lane's four filter values of a block are contiguous (one 16-byte load where K is a
//     multiple of 4), its four table entries one 16-byte LDS read; the next block's filter values are requested before this block's
//     MFMAs;
//   * the maps alternate between two LDS buffers; the last layer's map goes behind the extras of the row's feature vector.
// A row's sums: every output element is reduced by one wavefront over the blocks b = 0, 1, .. and steps w = 0 .. 3 in order -- the order
// depends neither on the row's place nor on n.  It is another order than the training kernels' (two interleaved accumulators) and the
// oracle's: differences at the 1e-7 level.
#include <algorithm>
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

// one layer of one row: sIn -> out (LDS or the row's feature vector), [c][oy][ox]
template <bool VEC>
__device__ __forceinline__ void acLayer(AcLayerRef L, const float* __restrict__ W, const int* sTab, const float* sIn, float* out,
                                        int wave, int li, int lc) {
  const int K = L.K, P = L.P, KnC = L.KnC;
  const int nPT = (P + 15) >> 4, npg = L.npg, nPG = (nPT + npg - 1) / npg, nU = ((KnC + 15) >> 4) * nPG, nB = (K + 15) >> 4;
  const int* tab = sTab + L.tabOff;
  for (int u = wave; u < nU; u += 4) {
    const int ct = u / nPG, pt0 = (u - ct * nPG) * npg, np = min(npg, nPT - pt0);      // (wave-uniform)
    int pb[AC_NPG];      // this lane's output position of tile j: the origin of its patch in the input map
#pragma unroll
    for (int j = 0; j < AC_NPG; ++j) {
      const int pos = (pt0 + j) * 16 + li, p = (j < np && pos < P) ? pos : 0, oy = p / L.OpX, ox = p - oy * L.OpX;
      pb[j] = (oy * L.InX + ox) * L.S;
    }
    // the biases of this lane's outputs (channel ct 16 + 4 lc + q, position of tile j), requested in front of the reduction
    float bq[AC_NPG][4];
#pragma unroll
    for (int j = 0; j < AC_NPG; ++j) {
      const int pos = (pt0 + j) * 16 + li;
#pragma unroll
      for (int q = 0; q < 4; ++q) { const int c = ct * 16 + 4 * lc + q; bq[j][q] = (j < np && pos < P && c < KnC) ? W[L.indB + (long long)c * P + pos] : 0.f; }
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
      const int pos = (pt0 + j) * 16 + li;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = ct * 16 + 4 * lc + q;
        if (pos < P && c < KnC) { const float x = acc[j][q] + bq[j][q]; out[c * P + pos] = x / (1 + fabsf(x)); }      // SoftSign (Functions.h)
      }
    }
  }
}

// the layers' offset tables k -> ic InY InX + fy InX + fx, once per workgroup
__device__ __forceinline__ void acTables(AcArgs a, int* sTab, int tid) {
  for (int l = 0; l < a->nL; ++l) {
    AcLayerRef L = a->L[l];
    const int fsz = L.KnY * L.KnX, Kp = (L.K + 15) & ~15;
    for (int k = tid; k < Kp; k += 256) {
      int off = 0;
      if (k < L.K) { const int ic = k / fsz, f = k - ic * fsz, fy = f / L.KnX, fx = f - fy * L.KnX; off = (ic * L.InY + fy) * L.InX + fx; }
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

// the conv stack on the row in LDS: the maps alternate between the two buffers, the last one goes behind the extras of the feature vector
__device__ __forceinline__ void acRowLayers(AcArgs a, const int* sTab, float* sDyn, const float* sImg, float* fr, int wave, int li, int lc) {
  const float* __restrict__ W = a->W;
  __syncthreads();
  for (int l = 0; l < a->nL; ++l) {
    a = acFresh(a);
    AcLayerRef L = a->L[l];
    const float* sIn = l == 0 ? sImg : sDyn + a->bufOff[(l - 1) & 1];
    float* out = l == a->nL - 1 ? fr + a->extras : sDyn + a->bufOff[l & 1];
    if (L.vec) acLayer<true>(L, W, sTab, sIn, out, wave, li, lc);
    else acLayer<false>(L, W, sTab, sIn, out, wave, li, lc);
    __syncthreads();      // the map is complete; every wavefront has read its input (the next row's image may take its place)
  }
}

__global__ __launch_bounds__(256) void act_conv_kernel(ActConvArgs) {
  extern __shared__ __attribute__((aligned(16))) float sDyn[];      // offset tables | image | map buffer 0 | map buffer 1
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  AcArgs a = acArgs();
  int* sTab = reinterpret_cast<int*>(sDyn);
  float* sImg = sDyn + a->imgOff;
  acTables(a, sTab, tid);
  for (int row = blockIdx.x; row < a->n; row += gridDim.x) {
    a = acFresh(a);
    float* fr = a->feat + (size_t)row * a->ldF;
    acLoadRow(a, AcRowSrc{a->in + (size_t)row * a->dIn}, sImg, fr, tid);
    acRowLayers(a, sTab, sDyn, sImg, fr, wave, li, lc);
  }
}

// the same on windows of the caller's device array (hl_forward_sequences_dev): agent `row` reads its stacked row straight from the states of
// its window -- the mapping of act_stack_dev_kernel (actdev.hip) and act_stack_row (act_host.h), row arithmetic in 64 bits --, no
// [n][dIn] intermediate.  Only the loads differ: from the standardised row on the arithmetic and its order are act_conv_kernel's
__global__ __launch_bounds__(256) void act_conv_dev_kernel(ActConvArgs) {
  extern __shared__ __attribute__((aligned(16))) float sDyn[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  AcArgs a = acArgs();
  int* sTab = reinterpret_cast<int*>(sDyn);
  float* sImg = sDyn + a->imgOff;
  acTables(a, sTab, tid);
  for (int row = blockIdx.x; row < a->n; row += gridDim.x) {
    a = acFresh(a);
    float* fr = a->feat + (size_t)row * a->ldF;
    acLoadRow(a, AcWindowSrc{a->in, a->firstRow[row], a->rowStride, max(a->nSteps[row], 1) - 1}, sImg, fr, tid);
    acRowLayers(a, sTab, sDyn, sImg, fr, wave, li, lc);
  }
}

// the kernel serves this net: geometry checked (every patch inside its input map), LDS layout and the work split filled in
constexpr size_t AC_LDS_BUDGET = 160 * 1024;
bool act_conv_plan(ActConvArgs* a) {
  if (a->recurrent || a->nL < 1 || a->nL > HL_MAX_CONV || a->dS < 1 || a->dIn < 1) return false;
  long long tab = 0, prev = 0, buf[2] = {0, 0};
  for (int l = 0; l < a->nL; ++l) {
    ActConvLayer& L = a->L[l];
    if (L.InC < 1 || L.InY < 1 || L.InX < 1 || L.KnC < 1 || L.KnY < 1 || L.KnX < 1 || L.S < 1 || L.OpY < 1 || L.OpX < 1) return false;
    if ((long long)(L.OpY - 1) * L.S + L.KnY > L.InY || (long long)(L.OpX - 1) * L.S + L.KnX > L.InX) return false;      // zero padding
    const long long inSize = (long long)L.InC * L.InY * L.InX, outSize = (long long)L.KnC * L.OpY * L.OpX;
    if (inSize >= (1 << 20) || outSize >= (1 << 20)) return false;
    if (l == 0 ? inSize > a->dIn : inSize != prev) return false;
    if (L.K != L.InC * L.KnY * L.KnX || L.P != L.OpY * L.OpX || L.indW < 0 || L.indB < 0) return false;
    L.vec = (L.K & 3) == 0 && (L.indW & 3) == 0;
    L.tabOff = (int)tab; tab += (L.K + 15) & ~15;
    if (l < a->nL - 1) buf[l & 1] = std::max(buf[l & 1], (outSize + 3) & ~3LL);
    // as many position tiles per unit as still leave every wavefront one
    const int nCT = (L.KnC + 15) >> 4, nPT = (L.P + 15) >> 4;
    L.npg = 1;
    for (int g = AC_NPG; g > 1; --g) if (nCT * ((nPT + g - 1) / g) >= 4) { L.npg = g; break; }
    prev = outSize;
  }
  a->img = a->L[0].InC * a->L[0].InY * a->L[0].InX; a->extras = a->dIn - a->img;
  if (a->extras + prev > ACT_ROWS_MAXW) return false;      // the feature row is act_rows_kernel's input row
  a->nF = a->extras + (int)prev;
  a->vec = (a->dIn & 3) == 0 && (a->dS & 3) == 0 && (a->img & 3) == 0;
  a->imgOff = (int)tab;      // (a multiple of 16 ints)
  a->bufOff[0] = a->imgOff + ((a->img + 3) & ~3);
  a->bufOff[1] = a->bufOff[0] + (int)buf[0];
  a->ldsBytes = ((size_t)a->bufOff[1] + (size_t)buf[1]) * sizeof(float);
  return a->ldsBytes <= AC_LDS_BUDGET;
}
hipError_t launch_act_conv(const ActConvArgs& a, int nBlocks, hipStream_t s) {
  if (a.n < 1 || nBlocks < 1 || a.ldsBytes == 0 || a.ldF < a.nF) return hipErrorInvalidValue;
  hipError_t e = ensureDynLds(reinterpret_cast<const void*>(act_conv_kernel), a.ldsBytes); if (e != hipSuccess) return e;
  hipLaunchKernelGGL(act_conv_kernel, dim3(std::min(nBlocks, a.n)), dim3(256), a.ldsBytes, s, a);
  return hipGetLastError();
}
hipError_t launch_act_conv_dev(const ActConvArgs& a, int nBlocks, hipStream_t s) {
  if (a.n < 1 || nBlocks < 1 || a.ldsBytes == 0 || a.ldF < a.nF || !a.in || !a.feat || !a.firstRow || !a.nSteps || a.rowStride < 1) return hipErrorInvalidValue;
  hipError_t e = ensureDynLds(reinterpret_cast<const void*>(act_conv_dev_kernel), a.ldsBytes); if (e != hipSuccess) return e;
  ActConvArgs d = a;
  if (reinterpret_cast<uintptr_t>(a.in) & 15) d.vec = 0;      // (a state then starts at no 16-byte boundary: the scalar loads, the same values)
  hipLaunchKernelGGL(act_conv_dev_kernel, dim3(std::min(nBlocks, a.n)), dim3(256), a.ldsBytes, s, d);
  return hipGetLastError();
}

}  // namespace hl
