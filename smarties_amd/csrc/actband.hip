// smarties_amd/csrc/actband.hip -- acting from DEVICE memory beyond the resident plans of actconv.hip and actrows.hip (learner_dev.h: the nets
// whose image does not fit a workgroup's LDS beside the maps, the nets whose feature or input row is wider than ACT_ROWS_MAXW, the
// Nature-DQN stack of Network/Builder.cpp:189-194 being both).  Rows in device memory can be streamed: a second read costs L2 traffic, not
// the bus.  Both kernels differ from their resident twins in the FIRST layer only and share every other line with them (act_conv_dev.h,
// act_rows_dev.h); the plans are host arithmetic of their own (act_plan.h).
//
// act_conv_band_dev_kernel: act_conv_dev_kernel with the first layer in nb bands of bandR output rows.  Band b -- output rows
//   [b R, min((b + 1) R, OpY)) -- loads the (r - 1) S + KnY input rows its r output rows read, of every channel, from the agent's window
//   (AcWindowSrc, standardised on load) into an LDS buffer [InC][bandRows][InX]; the first layer's offset table is built for that channel
//   pitch and a position's base is taken relative to the band's first input row; the band's part of the first map goes where the whole
//   map goes in the resident kernel.  Consecutive bands read the KnY - S rows they share again.  A barrier between a band's loads and its
//   products, and between its products and the next band's loads.
//     LDS: the row pitch of the band buffer is the image's InX, so the 16 lanes of a gather (positions ox S apart) and its four lane
//     groups (filter offsets inside one block of 16 indices) meet the banks exactly as they do on the resident image; only the channel
//     pitch differs, which a gather sees where a block of 16 reduction indices straddles two channels.  The loads of a band are issued
//     four per thread before the first is used, as acLoadRow issues a row's.
//   Sums: an output element is one wavefront's reduction over the blocks b = 0, 1, .. and steps w = 0 .. 3 in order, whichever band and
//   tile its position falls into: the results equal act_conv_dev_kernel's bit for bit on any net both run.
//
// act_rows_panel_kernel: act_rows_kernel with the first layer's input row -- up to ACT_DEV_MAX_ROW wide, never resident -- staged in panels
//   of pn columns into an LDS buffer [16][pn + 4] (pn a multiple of 32: the pitch is 4 mod 32 as the activations' is, and a panel ends on
//   a whole batch of reduction steps), standardised on load where the rows are raw.  The first layer's accumulators persist across the
//   panels; its parametric residual reads the input columns c < resW from the rows in device memory (standardised with the load's
//   expression) instead of from LDS.  Sums: the MFMAs into every accumulator run over s = 0, 1, .. as in act_rows_kernel, so the results
//   equal its bit for bit on any net both run.
#include <algorithm>
#include "act_conv_dev.h"
#include "act_rows_dev.h"

namespace hl {

// the state variables behind the image of the agent's row, standardised, to the front of its feature vector
__device__ __forceinline__ void acLoadExtras(AcArgs a, const AcWindowSrc& src, float* fr, int tid) {
  const int img = a->img, dIn = a->dIn, dS = a->dS;
  for (int c = img + tid; c < dIn; c += 256) { const int k = c % dS; fr[c - img] = (*src.at(c, dS) - a->stMean[k]) * a->stScale[k]; }
}

// input rows [iy0, iy0 + rows) of every channel of the agent's image, standardised, into the band buffer [InC][bandRows][InX]
__device__ __forceinline__ void acLoadBand(AcArgs a, const AcWindowSrc& src, float* sBand, int iy0, int rows, int tid) {
  AcLayerRef L = a->L[0];
  const int InC = L.InC, chan = L.InY * L.InX, seg = rows * L.InX, pitch = a->bandRows * L.InX, c0 = iy0 * L.InX, dS = a->dS;
  if (a->bandVec) {      // dS, the channels and the band's slice of a channel are multiples of 4 floats: 16-byte loads, four in flight per thread
    const int seg4 = seg >> 2;
    for (int ic = 0; ic < InC; ++ic) {
      const int cb = ic * chan + c0;
      float* dst = sBand + ic * pitch;
      for (int i0 = 0; i0 < seg4; i0 += 1024) {
        f32x4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int i = i0 + tid + 256 * q; v[q] = i < seg4 ? *reinterpret_cast<const f32x4*>(src.at(cb + 4 * i, dS)) : f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = i0 + tid + 256 * q;
          if (i < seg4) {
            const int k = (cb + 4 * i) % dS;
            const f32x4 mean = *reinterpret_cast<const f32x4*>(a->stMean + k), scale = *reinterpret_cast<const f32x4*>(a->stScale + k);
            *reinterpret_cast<f32x4*>(dst + 4 * i) = (v[q] - mean) * scale;
          }
        }
      }
    }
  } else {
    for (int ic = 0; ic < InC; ++ic) {
      const int cb = ic * chan + c0;
      float* dst = sBand + ic * pitch;
      for (int e0 = 0; e0 < seg; e0 += 1024) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int e = e0 + tid + 256 * q; v[q] = e < seg ? *src.at(cb + e, dS) : 0.f; }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e = e0 + tid + 256 * q;
          if (e < seg) { const int k = (cb + e) % dS; dst[e] = (v[q] - a->stMean[k]) * a->stScale[k]; }
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void act_conv_band_dev_kernel(ActConvArgs) {
  extern __shared__ __attribute__((aligned(16))) float sDyn[];      // offset tables | band buffer | map buffer 0 | map buffer 1
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  AcArgs a = acArgs();
  int* sTab = reinterpret_cast<int*>(sDyn);
  float* sBand = sDyn + a->bandOff;
  acTables<true>(a, sTab, tid);
  for (int row = blockIdx.x; row < a->n; row += gridDim.x) {
    a = acFresh(a);
    float* fr = a->feat + (size_t)row * a->ldF;
    const AcWindowSrc src{a->in, a->firstRow[row], a->rowStride, max(a->nSteps[row], 1) - 1};
    acLoadExtras(a, src, fr, tid);
    float* out0 = a->nL == 1 ? fr + a->extras : sDyn + a->bufOff[0];
    for (int b = 0; b < a->nb; ++b) {
      a = acFresh(a);
      AcLayerRef L = a->L[0];
      const int oy0 = b * a->bandR, oy1 = min(oy0 + a->bandR, L.OpY);
      acLoadBand(a, src, sBand, oy0 * L.S, (oy1 - oy0 - 1) * L.S + L.KnY, tid);
      __syncthreads();      // the band is in LDS (and, first band, the offset tables)
      if (L.vec) acLayerRange<true>(L, a->W, sTab, sBand, out0, wave, li, lc, oy0 * L.OpX, oy1 * L.OpX, oy0);
      else acLayerRange<false>(L, a->W, sTab, sBand, out0, wave, li, lc, oy0 * L.OpX, oy1 * L.OpX, oy0);
      __syncthreads();      // every wavefront has read the band: the next one (the next row's first) may take its place
    }
    acRowLayers(a, sTab, sDyn, sBand, fr, wave, li, lc, 1);
  }
}

hipError_t launch_act_conv_band_dev(const ActConvArgs& a, int nBlocks, hipStream_t s) {
  if (a.n < 1 || nBlocks < 1 || a.ldsBytes == 0 || a.ldF < a.nF || !a.in || !a.feat || !a.firstRow || !a.nSteps || a.rowStride < 1) return hipErrorInvalidValue;
  if (a.nb < 1 || a.bandR < 1 || a.bandRows < 1 || (long long)a.nb * a.bandR < a.L[0].OpY) return hipErrorInvalidValue;      // (no plan of act_conv_band_plan)
  hipError_t e = ensureDynLds(reinterpret_cast<const void*>(act_conv_band_dev_kernel), a.ldsBytes); if (e != hipSuccess) return e;
  ActConvArgs d = a;
  if (reinterpret_cast<uintptr_t>(a.in) & 15) d.bandVec = 0;      // (a state then starts at no 16-byte boundary: the scalar loads, the same values)
  hipLaunchKernelGGL(act_conv_band_dev_kernel, dim3(std::min(nBlocks, a.n)), dim3(256), a.ldsBytes, s, d);
  return hipGetLastError();
}

typedef const __attribute__((address_space(4))) ActRowsArgs* ArArgs;

template <int NG>
__global__ __launch_bounds__(256) void act_rows_panel_kernel(ActRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sDyn[];      // [16][ld] activations | [16][ldO] output-layer values | [16][pn + 4] panel
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  const int row0 = blockIdx.x * AR_ROWS;
  float* sX = sDyn;
  {
    // the first layer: its input row panel by panel, the accumulators kept.  (The loop reads its fields through the kernel-argument
    // segment, the pointer taken as new per panel, and forms its pointers there: a field is then loaded where it is used, not kept in a
    // scalar register across the products -- act_conv_dev.h; kept from the kernel's start on, NG = 8 parked scalars in vector lanes)
    ArArgs ka = (ArArgs)__builtin_amdgcn_kernarg_segment_ptr();
    int g0, nu; arGroups(ka->L[0].size, wave, g0, nu);      // (nu <= NG: act_rows_panel_plan)
    f32x4 acc[4 * NG];
#pragma unroll
    for (int i = 0; i < 4 * NG; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < ka->dIn; k0 += ka->pn) {
      asm volatile("" : "+s"(ka));
      const int dIn = ka->dIn, pn = ka->pn, ldP = pn + 4, w = min(pn, dIn - k0), rows = min(AR_ROWS, ka->n - row0);
      float* sP = sDyn + ka->panOff;
      {
        // the panel's columns of the block's rows, standardised (Episode::standardizedState, Episode.h:172-183): a thread takes a column
        // of all 16 rows, sixteen loads in flight (rows beyond n: zeros)
        const float* src = ka->in + (size_t)row0 * dIn + k0;
        const bool raw = ka->stMean != nullptr;      // (no statistics: rows standardised already -- the conv stack's feature rows; (v - 0) 1 is v)
        for (int c = tid; c < w; c += 256) {
          const int k = (k0 + c) % ka->dS;
          const float mean = raw ? ka->stMean[k] : 0.f, scale = raw ? ka->stScale[k] : 1.f;
          float v[AR_ROWS];
          const float* p = src + c;      // (walked row by row in vector registers, not through sixteen scalar row offsets)
#pragma unroll
          for (int r = 0; r < AR_ROWS; ++r) { v[r] = r < rows ? *p : 0.f; p += dIn; asm volatile("" : "+v"(p)); }
#pragma unroll
          for (int r = 0; r < AR_ROWS; ++r) sP[r * ldP + c] = r < rows ? (v[r] - mean) * scale : 0.f;
        }
      }
      __syncthreads();
      asm volatile("" : "+s"(ka));
      arAccumulate<NG>(acc, ka->W + ka->L[0].indW + (size_t)k0 * ka->L[0].ldW, ka->L[0].ldW, w, sP, ldP, g0, nu, li, lc);
      __syncthreads();      // every wavefront has read the panel: the next one takes its place
    }
    // the residual's input columns come from the rows in device memory, standardised as the panels were
    const ActLayer L = a.L[0];
    const int resW = L.hasRes ? L.resW : 0, dS = a.dS, dIn = a.dIn, rows = min(AR_ROWS, a.n - row0);
    const float* stMean = a.stMean; const float* stScale = a.stScale; const float* src = a.in + (size_t)row0 * dIn;
    const bool raw = stMean != nullptr;
    arEpilogue<NG>(acc, L, a.W, sX, a.ld, g0, nu, li, lc, [=](int q, int c0, const f32x4*) {
      f32x4 in = {0.f, 0.f, 0.f, 0.f};
      const int r = 4 * lc + q;
      if (r < rows) {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (c0 + e < resW) {
          const int k = (c0 + e) % dS;
          in[e] = (src[(size_t)r * dIn + c0 + e] - (raw ? stMean[k] : 0.f)) * (raw ? stScale[k] : 1.f);
        }
      }
      return in;
    });
    __syncthreads();
  }
  const float* __restrict__ W = a.W;
  for (int l = 1; l < a.nL; ++l) arLayer<NG>(a.L[l], W, sX, a.ld, wave, li, lc);
  arOutput(a, W, sX, sDyn + AR_ROWS * a.ld, row0, min(AR_ROWS, a.n - row0), tid, wave, li, lc);
}

template <int NG> static hipError_t actRowsPanelLaunch(const ActRowsArgs& a, hipStream_t s) {
  hipError_t e = ensureDynLds(reinterpret_cast<const void*>(act_rows_panel_kernel<NG>), a.ldsBytes); if (e != hipSuccess) return e;
  hipLaunchKernelGGL((act_rows_panel_kernel<NG>), dim3(act_rows_blocks(a.n)), dim3(256), a.ldsBytes, s, a);
  return hipGetLastError();
}
hipError_t launch_act_rows_panel(const ActRowsArgs& a, hipStream_t s) {
  if (a.n < 1 || a.ld < 1 || a.pn < 32 || (a.pn & 31) || a.panOff < AR_ROWS * (a.ld + a.ldO)) return hipErrorInvalidValue;      // (no plan of act_rows_panel_plan)
  if (a.ldsBytes < (size_t)(a.panOff + AR_ROWS * (a.pn + 4)) * sizeof(float)) return hipErrorInvalidValue;
  switch (a.ng) {
    case 1: return actRowsPanelLaunch<1>(a, s);
    case 2: return actRowsPanelLaunch<2>(a, s);
    case 4: return actRowsPanelLaunch<4>(a, s);
    case 8: return actRowsPanelLaunch<8>(a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace hl
