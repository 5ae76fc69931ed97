// smarties_amd/csrc/convg.hip -- convolutional layers of GENERAL geometry: zero padding, a stride per axis (1 .. 8, any value), up to 256
// channels in and out.  conv.hip's kernels gather their patch elements straight from global memory through an offset table without bounds
// (a padded tap would read the neighbouring row or sample) and keep the whole filter of a channel tile in LDS (64 channels at most); the
// layers they serve keep them.  Here every pass is ONE correlation with zero fill,
//
//     out[r][u][v] = sum_{ch, a, b}  A[r][(ch, a, b)]  src[ch][u SY + a - PY][v SX + b - PX]        (src = 0 outside its image)
//
// computed by workgroups that own a BAND of outputs of one sample (RB rows x XB columns, at most 128 positions = 8 tiles of 16) and 64 rows r:
//   * the window of the band -- (RB - 1) SY + TA source rows, (XB - 1) SX + TB columns, a CHUNK of reduction channels -- is staged in LDS with
//     zeros written for every element outside the image: padding is resolved there, the MFMA loop carries no bounds test;
//   * window columns are stored de-interleaved by their residue modulo SX (column w -> slot (w mod SX) WQ + w / SX): the 16 lanes of a tile row
//     -- consecutive outputs v, source columns SX apart -- read CONSECUTIVE LDS words for a given tap, whatever SX (2, 3, 4, 8: no pitch gives
//     that for the plain layout: 16 lanes 8 words apart share 4 of 32 banks); the row pitch is odd, so tiles that span two band rows do not
//     pile up either.  B operand = window[origin(u, v) + table(ch, a, b)], origin = u SY pitch + v, table = ch plane + a pitch + slot(b);
//   * the A slice of the chunk (64 rows x chunk channels x taps, pitch = 4 mod 32) lies beside it; the reduction runs chunk by chunk, k inside
//     a chunk in table order, the accumulators (4 row tiles x 2 position tiles per wavefront) stay in registers: a fixed order, bit-reproducible;
//   * rows beyond 64 go over blockIdx.z.
//
//   forward  A = the filter rows (ConvGeo::Wf), src = the input image; epilogue = conv.hip's: + bias per output element, X and Y = softsign(X)
//            in the reference's [c][oy][ox] layout, 64-byte runs per channel.
//   dX       gather form by RESIDUE CLASS (ry, rx) = ((iy + Py) mod Sy, (ix + Px) mod Sx) of the input position: only the taps fy = ry + ty Sy,
//            fx = rx + tx Sx reach it, from output (jy - ty, jx - tx) with jy = (iy + Py) / Sy.  Per class that is a stride-1 correlation of the
//            deltas with the class's own tap list (T = ceil((Kn - r) / S) per axis: classes differ, a class may have none) and its own slice of
//            the transposed filter, ConvGeo::Wg, written by convg_prep_kernel in front of the launch.  Neither the filter nor the image need be a
//            multiple of the stride (conv.hip: convStrided demands both).  Deltas are staged zero-filled beyond [0, OpY) x [0, OpX): no test on the
//            quotients.  Epilogue: x act'(X) of the layer below -> its D.  No atomics.
//   dW       dK[c][k] = sum_{(b, p)} D[b][c][p] in_padded[(b, p) -> k]: a workgroup owns 128 patch elements k x 64 channels c and a chunk of
//            samples; per (sample, band) it stages the same zero-filled window (the input channels its k touch) and the band's deltas, A = deltas,
//            B = window[origin(p) + table(k)].  One partial per chunk -> ConvGeo::part, summed in chunk order by conv_reduce_adam_kernel
//            (conv.hip, unchanged; the bias gradient stays a RED_COL problem of the common launch).
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; tools/resource_usage.py prints them): no scratch, no VGPR and no SGPR
// spills in any kernel.  Dynamic LDS is the band plan's (convg_plan: at most 144 KB), 0 bytes static.
//   convg_kernel<forward>   VGPR 48   AGPR 32   SGPR 106   scratch 0   6 waves / SIMD
//   convg_kernel<dX>        VGPR 46   AGPR 32   SGPR 106   scratch 0   6 waves / SIMD
//   convg_dw_kernel         VGPR 46   AGPR 32   SGPR 106   scratch 0   6 waves / SIMD
//   convg_prep_kernel       VGPR 15   AGPR 0    SGPR 42    scratch 0
// (the staging loop is unrolled twice, not four times, and the filter gradient walks its (sample, band) pairs in one loop: either of the
// other forms costs convg_dw_kernel one or two spilled scalar registers)
#include "convg_band.h"      // cgPad4, CgBand, cgBand, cgSlot, the budget and the band size: shared with actconvg.hip

namespace hl {

__device__ __forceinline__ float cgSoftsign(float x) { return x / (1 + fabsf(x)); }
__device__ __forceinline__ float cgSoftsignDiff(float x) { const float d = 1 + fabsf(x); return 1 / (d * d); }

// one axis of a residue class of the input gradient: T taps, class coordinates j = lo .. lo + n - 1 (input coordinate j S + r - Pd)
struct CgAxis { int T, lo, n; };
__host__ __device__ inline CgAxis cgAxis(int r, int S, int Pd, int Kn, int In) {
  CgAxis c; c.T = r < Kn ? (Kn - r + S - 1) / S : 0; c.lo = Pd > r ? (Pd - r + S - 1) / S : 0;
  const int top = In - 1 + Pd - r; c.n = top < 0 ? 0 : top / S - c.lo + 1; if (c.n < 0) c.n = 0;
  return c;
}
__host__ __device__ inline int cgTapsMax(int Kn, int S) { return (Kn + S - 1) / S; }
__host__ __device__ inline int cgLdg(const ConvGeo& g) { return cgPad4(g.KnC * cgTapsMax(g.KnY, g.Sy) * cgTapsMax(g.KnX, g.Sx)) + 4; }      // pitch of a Wg row
// floats of dynamic LDS: window of `nc` channels | 64 operand rows of `red` reduction elements (+ 4: pitch = 4 mod 32 where red is a
// multiple of 32) | a table of `red` offsets
__host__ __device__ inline size_t cgLdsFloats(const CgBand& bd, int nc, int red) { return (size_t)cgPad4(nc * bd.plane) + (size_t)64 * (cgPad4(red) + 4) + cgPad4(red); }
constexpr int CONVG_DW_K = 128;          // patch elements of a filter-gradient workgroup: 8 tiles of 16, two per wavefront

bool convg_needed(int sx, int sy, int px, int py, int inC, int knC) {
  return px != 0 || py != 0 || sx != sy || (sx & (sx - 1)) != 0 || inC > 64 || knC > 64;
}
long long convg_prep_floats(const ConvGeo& g) { return (long long)g.Sy * g.Sx * ((g.InC + 15) & ~15) * cgLdg(g); }

// band of at most CONVG_BAND_POS outputs and the reduction channels beside it within the budget.  chunked: the largest channel chunk that
// fits (forward, dX); else exactly C channels and a table of the band's positions (dW)
static bool cgFit(int NU, int NV, int SY, int SX, int TA, int TB, int C, bool chunked, short (&out)[3]) {
  int XB = NV < CONVG_BAND_POS ? NV : CONVG_BAND_POS, RB = CONVG_BAND_POS / XB;
  if (RB > NU) RB = NU;
  if (RB < 1) RB = 1;
  for (;;) {
    const CgBand bd = cgBand(RB, XB, SY, SX, TA, TB);
    if (chunked) {
      for (int icc = C; icc >= 1; --icc)
        if (cgLdsFloats(bd, icc, icc * TA * TB) * 4 <= CONVG_LDS_BUDGET) { out[0] = (short)RB; out[1] = (short)XB; out[2] = (short)icc; return true; }
    } else if (cgLdsFloats(bd, C, RB * XB) * 4 <= CONVG_LDS_BUDGET) { out[0] = (short)RB; out[1] = (short)XB; out[2] = (short)C; return true; }
    if (RB > 1) RB = (RB + 1) / 2; else if (XB > 16) XB = (XB + 1) / 2; else return false;
  }
}
bool convg_plan(ConvGeo* g, int rows) {
  const int fsz = g->KnY * g->KnX;
  if (!cgFit(g->OpY, g->OpX, g->Sy, g->Sx, g->KnY, g->KnX, g->InC, true, g->gF)) return false;
  if (!cgFit((g->InY + g->Sy - 1) / g->Sy, (g->InX + g->Sx - 1) / g->Sx, 1, 1, cgTapsMax(g->KnY, g->Sy), cgTapsMax(g->KnX, g->Sx), g->KnC, true, g->gX)) return false;
  int nIc = (CONVG_DW_K - 1) / fsz + 2; if (nIc > g->InC) nIc = g->InC;      // input channels that 128 consecutive patch elements touch
  if (!cgFit(g->OpY, g->OpX, g->Sy, g->Sx, g->KnY, g->KnX, nIc, false, g->gW)) return false;
  // filter gradient: a few hundred workgroups over (128 patch elements, 64 channels, chunk of samples)
  const int groups = ((g->K + CONVG_DW_K - 1) / CONVG_DW_K) * ((g->KnC + 63) / 64);
  int want = 512 / groups; if (want < 1) want = 1; if (want > rows) want = rows;
  g->gSamples = (rows + want - 1) / want; g->nChunks = (rows + g->gSamples - 1) / g->gSamples; g->chunkRows = g->gSamples * g->P;
  return true;
}

// ---------------------------------------------------------------------------------------------------------------
// Wg[class][ic][(c, a, b)] = K[c][ic][ry + (TA - 1 - a) Sy][rx + (TB - 1 - b) Sx], zero padded: the A rows of the class's correlation
// (row a of the staged deltas is output row jy - (TA - 1 - a)).  In front of the input gradient, once per step: the weights are those of
// the step's forward pass
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void convg_prep_kernel(ConvArgs a, int l) {
  const ConvGeo& g = a.L[l];
  const int rows = (g.InC + 15) & ~15, ldg = cgLdg(g);
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)g.Sy * g.Sx * rows * ldg) return;
  const int cls = (int)(i / ((long long)rows * ldg)), rem = (int)(i - (long long)cls * rows * ldg), ic = rem / ldg, kk = rem - ic * ldg;
  const int ry = cls / g.Sx, rx = cls - ry * g.Sx;
  const int TA = cgAxis(ry, g.Sy, g.Py, g.KnY, g.InY).T, TB = cgAxis(rx, g.Sx, g.Px, g.KnX, g.InX).T, nT = TA * TB;
  float w = 0.f;
  if (ic < g.InC && kk < g.KnC * nT) {
    const int c = kk / nT, f = kk - c * nT, aa = f / TB, bb = f - aa * TB;
    const int fy = ry + (TA - 1 - aa) * g.Sy, fx = rx + (TB - 1 - bb) * g.Sx;
    w = a.W[g.indW + (((size_t)c * g.InC + ic) * g.KnY + fy) * g.KnX + fx];
  }
  g.Wg[i] = w;
}
hipError_t launch_convg_prep(const ConvArgs& a, int l, hipStream_t s) {
  const long long n = convg_prep_floats(a.L[l]);
  hipLaunchKernelGGL(convg_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, l);
  return hipGetLastError();
}

// channels [ch0, ch0 + ncc) of the image src[ch][srcY][srcX], rows y0 .. y0 + WR, columns x0 .. x0 + WW -> the window, zeros outside the image
__device__ __forceinline__ void cgStageWindow(float* sWin, const float* __restrict__ src, int srcY, int srcX, int ch0, int ncc, int y0, int x0, const CgBand& bd, int SX) {
  const int perCh = bd.WR * bd.WW, total = ncc * perCh;
#pragma unroll 2
  for (int i = threadIdx.x; i < total; i += 256) {
    const int ch = i / perCh, r = i - ch * perCh, wr = r / bd.WW, wx = r - wr * bd.WW;
    const int sy = y0 + wr, sx = x0 + wx;
    float v = 0.f;
    if ((unsigned)sy < (unsigned)srcY && (unsigned)sx < (unsigned)srcX) v = src[((size_t)(ch0 + ch) * srcY + sy) * srcX + sx];
    sWin[ch * bd.plane + wr * bd.pitch + cgSlot(wx, SX, bd.WQ)] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// forward (DX = 0; grid: bands x rows x groups of 64 output channels) and input gradient (DX = 1; grid: bands of the largest class x
// samples x (class, group of 64 input channels))
// ---------------------------------------------------------------------------------------------------------------
template <int DX>
__global__ __launch_bounds__(256) void convg_kernel(ConvArgs a, int l) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const ConvGeo g = a.L[l];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  const int row = blockIdx.y;
  if (!DX && row >= a.sc->nRows[a.parity]) return;
  // the correlation of this workgroup
  int C, SrcY, SrcX, NU, NV, NVmax, SY, SX, PY, PX, TA, TB, M, ldA, rg, ry = 0, rx = 0, jy0 = 0, jx0 = 0;
  const float* A; const float* src;
  if (!DX) {
    C = g.InC; SrcY = g.InY; SrcX = g.InX; NU = g.OpY; NV = NVmax = g.OpX; SY = g.Sy; SX = g.Sx; PY = g.Py; PX = g.Px; TA = g.KnY; TB = g.KnX;
    M = g.KnC; ldA = cgPad4(g.K) + 4; A = g.Wf; rg = blockIdx.z; src = g.in + (size_t)row * g.ldIn;
  } else {
    const int nIg = (g.InC + 63) / 64, cls = (int)blockIdx.z / nIg;
    rg = (int)blockIdx.z - cls * nIg; ry = cls / g.Sx; rx = cls - ry * g.Sx;
    const CgAxis cy = cgAxis(ry, g.Sy, g.Py, g.KnY, g.InY), cx = cgAxis(rx, g.Sx, g.Px, g.KnX, g.InX);
    C = g.KnC; SrcY = g.OpY; SrcX = g.OpX; NU = cy.n; NV = cx.n; NVmax = (g.InX + g.Sx - 1) / g.Sx; SY = SX = 1; TA = cy.T; TB = cx.T;
    PY = cy.T - 1 - cy.lo; PX = cx.T - 1 - cx.lo; jy0 = cy.lo; jx0 = cx.lo;
    M = g.InC; ldA = cgLdg(g); A = g.Wg + (size_t)cls * ((g.InC + 15) & ~15) * ldA; src = g.D + (size_t)row * g.ldOut;
  }
  const int RB = DX ? g.gX[0] : g.gF[0], XB = DX ? g.gX[1] : g.gF[1], ICC = DX ? g.gX[2] : g.gF[2];
  const int nSeg = (NVmax + XB - 1) / XB, rb = (int)blockIdx.x / nSeg, seg = (int)blockIdx.x - rb * nSeg;
  const int u0 = rb * RB, v0 = seg * XB;
  if (u0 >= NU || v0 >= NV) return;                                   // (a smaller class: uniform over the workgroup, in front of every barrier)
  const int nU = min(RB, NU - u0), nV = min(XB, NV - v0), nPos = nU * nV, nT = TA * TB;
  const CgBand bd = cgBand(RB, XB, SY, SX, TA, TB);
  const int redMax = cgPad4(ICC * nT), ldAs = redMax + 4;
  float* sWin = reinterpret_cast<float*>(smem);                        // [ICC][WR][pitch]
  float* sA = sWin + cgPad4(ICC * bd.plane);                           // [64][ldAs]
  int* kOff = reinterpret_cast<int*>(sA + (size_t)64 * ldAs);          // [redMax]
  const int nCt = min(4, ((M + 15) >> 4) - rg * 4);                    // row tiles of this group
  // this wavefront's position tiles wave, wave + 4: origin of the lane's position in the window
  int org[2], ul[2], vl[2]; bool ok[2], tOn[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = (wave + 4 * j) * 16 + li;
    tOn[j] = (wave + 4 * j) * 16 < nPos; ok[j] = p < nPos;
    const int pc = ok[j] ? p : 0;
    ul[j] = pc / nV; vl[j] = pc - ul[j] * nV;
    org[j] = ul[j] * SY * bd.pitch + vl[j];
  }
  f32x4 acc[4][2];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) { acc[ct][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[ct][1] = acc[ct][0]; }
  const float* aRow = sA + li * ldAs + lc;
  for (int ch0 = 0; ch0 < C; ch0 += ICC) {
    const int ncc = min(ICC, C - ch0), Kc = ncc * nT, KcP = cgPad4(Kc);
    if (ch0) __syncthreads();                                          // the chunk before has been read
    cgStageWindow(sWin, src, SrcY, SrcX, ch0, ncc, u0 * SY - PY, v0 * SX - PX, bd, SX);
    for (int i = tid; i < nCt * 16 * KcP; i += 256) {
      const int r = i / KcP, kk = i - r * KcP, rowG = rg * 64 + r;
      sA[r * ldAs + kk] = (rowG < M && kk < Kc) ? A[(size_t)rowG * ldA + ch0 * nT + kk] : 0.f;
    }
    for (int kk = tid; kk < KcP; kk += 256) {
      int off = 0;                                                     // (padding: a zero operand row element times a staged value)
      if (kk < Kc) { const int ch = kk / nT, f = kk - ch * nT, aa = f / TB, bb = f - aa * TB; off = ch * bd.plane + aa * bd.pitch + cgSlot(bb, SX, bd.WQ); }
      kOff[kk] = off;
    }
    __syncthreads();
#pragma unroll 2
    for (int s = 0; s < (KcP >> 2); ++s) {
      const int off = kOff[4 * s + lc];
      const float b0 = sWin[org[0] + off], b1 = sWin[org[1] + off];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        if (ct < nCt) {
          const float av = aRow[ct * 16 * ldAs + 4 * s];
          if (tOn[0]) acc[ct][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc[ct][0], 0, 0, 0);
          if (tOn[1]) acc[ct][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc[ct][1], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (!ok[j]) continue;
    if (!DX) {
      const int P = g.P, pp = (u0 + ul[j]) * g.OpX + v0 + vl[j];
      const float* Bl = a.W + g.indB;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ch = (rg * 4 + ct) * 16 + lc * 4 + q;
          if (ct < nCt && ch < g.KnC) {
            const float x = acc[ct][j][q] + Bl[(size_t)ch * P + pp];
            const size_t o = (size_t)row * g.ldOut + (size_t)ch * P + pp;
            g.X[o] = x; g.Y[o] = cgSoftsign(x);
          }
        }
      }
    } else {
      const ConvGeo& gp = a.L[l - 1];                                  // the layer whose outputs are this layer's inputs
      const int iy = (jy0 + u0 + ul[j]) * g.Sy + ry - g.Py, ix = (jx0 + v0 + vl[j]) * g.Sx + rx - g.Px, Pin = g.InY * g.InX;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ic = (rg * 4 + ct) * 16 + lc * 4 + q;
          if (ct < nCt && ic < g.InC) {
            const size_t o = (size_t)row * gp.ldOut + (size_t)ic * Pin + (size_t)iy * g.InX + ix;
            gp.D[o] = acc[ct][j][q] * cgSoftsignDiff(gp.X[o]);
          }
        }
      }
    }
  }
}
template <int DX> static hipError_t launchConvgT(const ConvArgs& a, int l, int rows, hipStream_t s) {
  const ConvGeo& g = a.L[l];
  const short* pl = DX ? g.gX : g.gF;
  const int NU = DX ? (g.InY + g.Sy - 1) / g.Sy : g.OpY, NV = DX ? (g.InX + g.Sx - 1) / g.Sx : g.OpX;
  const int TA = DX ? cgTapsMax(g.KnY, g.Sy) : g.KnY, TB = DX ? cgTapsMax(g.KnX, g.Sx) : g.KnX;
  if (!g.gen || pl[0] < 1 || pl[1] < 1 || pl[2] < 1 || rows < 1) return hipErrorInvalidValue;
  const CgBand bd = cgBand(pl[0], pl[1], DX ? 1 : g.Sy, DX ? 1 : g.Sx, TA, TB);
  const size_t lds = cgLdsFloats(bd, pl[2], pl[2] * TA * TB) * 4;
  const unsigned bands = (unsigned)(((NU + pl[0] - 1) / pl[0]) * ((NV + pl[1] - 1) / pl[1]));
  const unsigned z = DX ? (unsigned)(g.Sy * g.Sx * ((g.InC + 63) / 64)) : (unsigned)((g.KnC + 63) / 64);
  hipError_t e = ensureDynLds(reinterpret_cast<const void*>(convg_kernel<DX>), lds); if (e != hipSuccess) return e;
  hipLaunchKernelGGL(convg_kernel<DX>, dim3(bands, (unsigned)rows, z), dim3(256), lds, s, a, l);
  return hipGetLastError();
}
hipError_t launch_convg_forward(const ConvArgs& a, int l, int maxRows, hipStream_t s) { return launchConvgT<0>(a, l, maxRows, s); }
hipError_t launch_convg_dx(const ConvArgs& a, int l, hipStream_t s) {
  if (l < 1 || !a.L[l].Wg) return hipErrorInvalidValue;
  return launchConvgT<1>(a, l, a.B, s);
}

// ---------------------------------------------------------------------------------------------------------------
// filter gradient.  grid: groups of 128 patch elements x chunks of samples x groups of 64 channels
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void convg_dw_kernel(ConvArgs a, int l) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const ConvGeo& g = a.L[l];      // (read where needed: a copy of the record costs scalar registers the loops need)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  const int RB = g.gW[0], XB = g.gW[1], NIC = g.gW[2], K = g.K, fsz = g.KnY * g.KnX, P = g.P, SY = g.Sy, SX = g.Sx;
  const int k0 = (int)blockIdx.x * CONVG_DW_K, chunk = blockIdx.y, c0 = (int)blockIdx.z * 64;
  const int icLo = k0 / fsz, icHi = min(g.InC - 1, (k0 + CONVG_DW_K - 1) / fsz), nIc = icHi - icLo + 1;      // (<= NIC: convg_plan)
  const CgBand bd = cgBand(RB, XB, SY, SX, g.KnY, g.KnX);
  const int posMax = cgPad4(RB * XB), ldD = posMax + 4;
  float* sWin = reinterpret_cast<float*>(smem);                        // [NIC][WR][pitch]
  float* sD = sWin + cgPad4(NIC * bd.plane);                           // [64][ldD]   the band's deltas, zero padded
  int* sPos = reinterpret_cast<int*>(sD + (size_t)64 * ldD);           // [posMax]    window origin of position p
  const int nCt = min(4, ((g.KnC + 15) >> 4) - (int)blockIdx.z * 4);
  // this wavefront's patch-element tiles wave, wave + 4; the lane's element k of each -> its window offset
  int ko[2];      // (an element beyond K reads element 0 of the window: computed, never stored)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = k0 + (wave + 4 * j) * 16 + li;
    ko[j] = 0;
    if (k < K) { const int ic = k / fsz, f = k - ic * fsz, aa = f / g.KnX, bb = f - aa * g.KnX; ko[j] = (ic - icLo) * bd.plane + aa * bd.pitch + cgSlot(bb, SX, bd.WQ); }
  }
  f32x4 acc[4][2];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) { acc[ct][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[ct][1] = acc[ct][0]; }
  const int nSeg = (g.OpX + XB - 1) / XB, nBands = ((g.OpY + RB - 1) / RB) * nSeg;
  const int b0 = chunk * g.gSamples, b1 = min(a.B, b0 + g.gSamples);
  const float* dRow = sD + li * ldD + lc;
  for (int it = b0 * nBands; it < b1 * nBands; ++it) {      // (sample, band) pairs of the chunk, one loop: fewer scalars live across the stages
    {
      const int b = it / nBands, band = it - b * nBands;
      const float* img = g.in + (size_t)b * g.ldIn; const float* Db = g.D + (size_t)b * g.ldOut;
      const int rb = band / nSeg, seg = band - rb * nSeg, u0 = rb * RB, v0 = seg * XB;
      const int nU = min(RB, g.OpY - u0), nV = min(XB, g.OpX - v0), nPos = nU * nV, nPos4 = cgPad4(nPos);
      __syncthreads();                                                 // the band before has been read
      cgStageWindow(sWin, img, g.InY, g.InX, icLo, nIc, u0 * SY - g.Py, v0 * SX - g.Px, bd, SX);
      for (int i = tid; i < nCt * 16 * nPos4; i += 256) {
        const int c = i / nPos4, p = i - c * nPos4, ch = c0 + c;
        float v = 0.f;
        if (p < nPos && ch < g.KnC) { const int u = p / nV, w = p - u * nV; v = Db[(size_t)ch * P + (u0 + u) * g.OpX + v0 + w]; }
        sD[c * ldD + p] = v;
      }
      for (int p = tid; p < nPos4; p += 256) { const int pc = p < nPos ? p : 0, u = pc / nV, w = pc - u * nV; sPos[p] = u * SY * bd.pitch + w; }
      __syncthreads();
      for (int s = 0; s < (nPos4 >> 2); ++s) {
        const int po = sPos[4 * s + lc];
        const float p0 = sWin[po + ko[0]], p1 = sWin[po + ko[1]];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          if (ct < nCt) {
            const float dv = dRow[ct * 16 * ldD + 4 * s];
            acc[ct][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv, p0, acc[ct][0], 0, 0, 0);
            acc[ct][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv, p1, acc[ct][1], 0, 0, 0);
          }
        }
      }
    }
  }
  float* part = g.part + (size_t)chunk * g.KnC * K;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = k0 + (wave + 4 * j) * 16 + li;
    if (k >= K) continue;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ch = c0 + ct * 16 + lc * 4 + q;
        if (ct < nCt && ch < g.KnC) part[(size_t)ch * K + k] = acc[ct][j][q];
      }
    }
  }
}
hipError_t launch_convg_dw(const ConvArgs& a, int l, hipStream_t s) {
  const ConvGeo& g = a.L[l];
  if (!g.gen || g.gW[0] < 1 || g.gW[1] < 1 || g.gW[2] < 1 || g.gSamples < 1 || g.nChunks != (a.B + g.gSamples - 1) / g.gSamples) return hipErrorInvalidValue;
  const CgBand bd = cgBand(g.gW[0], g.gW[1], g.Sy, g.Sx, g.KnY, g.KnX);
  const size_t lds = cgLdsFloats(bd, g.gW[2], g.gW[0] * g.gW[1]) * 4;
  hipError_t e = ensureDynLds(reinterpret_cast<const void*>(convg_dw_kernel), lds); if (e != hipSuccess) return e;
  hipLaunchKernelGGL(convg_dw_kernel, dim3((unsigned)((g.K + CONVG_DW_K - 1) / CONVG_DW_K), (unsigned)g.nChunks, (unsigned)((g.KnC + 63) / 64)), dim3(256), lds, s, a, l);
  return hipGetLastError();
}

}  // namespace hl
