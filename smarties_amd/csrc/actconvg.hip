// smarties_amd/csrc/actconvg.hip -- acting from device memory for conv stacks of GENERAL geometry (zero padding, a stride per axis, up to
// 256 channels: the layers convg.hip trains).  The acting kernels of actconv.hip / actband.hip keep every map of an agent in LDS, know one
// stride and gather through an offset table without bounds; a same-padded stack keeps its image size (32 channels of 84 x 84: 903 KB per
// map), so here the maps live in device scratch of the acting source and every layer of the stack is ONE launch for all agents of a chunk:
//
//     out[c][u][v] = softsign(bias[c][u][v] + sum_{ch, a, b} K[c][ch][a][b] src[ch][u SY + a - PY][v SX + b - PX])      (src = 0 outside its image)
//
// No padding and a power-of-two stride are special cases: every layer of a stack with one general layer runs here.
//
// Grid: bands of outputs x agents x groups of 16 TC output channels.  A workgroup of four wavefronts owns a band of RB rows x XB columns
// (at most 128 positions = 8 tiles of 16) of one agent:
//   * the band's window -- (RB - 1) SY + KnY rows, (XB - 1) SX + KnX columns of a CHUNK of ICC input channels -- is staged in LDS with zeros
//     for every element outside the image (the MFMA loop carries no bounds test), its columns de-interleaved by their residue modulo SX
//     (convg_band.h: consecutive outputs read consecutive LDS words whatever SX).  Staging goes BY WINDOW ROW: 2^sh lanes (the smallest
//     power of two that covers a row, 64 at most) take a (channel, row) pair, 64 / 2^sh pairs per wavefront at a time; channel and row
//     advance by increments, a column's slot comes from a table in LDS built once per workgroup: no division per staged element.
//       - the first layer reads the agent's window of the caller's [rows][dimS] array itself (AcWindowSrc's addressing: element c of the
//         stacked row is component c % dimS of the state c / dimS steps before the newest, steps before the first given state repeat
//         it, 64-bit row arithmetic): ONE division per (channel, row) pair finds the row's first element, the lanes walk on by
//         comparison.  Values are standardised on load.  Its launch also writes the agent's extras to the front of the feature row;
//       - layers behind it read the previous map from scratch in quads aligned to 16 bytes in MEMORY (the window's left edge is
//         x0 = v0 SX - PX: no alignment of its own): one 16-byte load where the quad lies inside the image row, scalar loads of the
//         same values at the row's ends and where the scratch pointer is not aligned.  Staging moves values, it computes nothing;
//   * the A operand is read straight from the source's blob in the reference layout K[c][ic][fy][fx] -- a filter row IS the (ch, a, b)
//     ordered operand row; the slice of the chunk (16 TC rows, pitch = 4 mod 32) lies beside the window.  No prepared copy is read
//     (ConvGeo::Wf reflects the live weights only; the snapshot source has none);
//   * the reduction runs chunk by chunk, k inside a chunk in (ch, a, b) order, accumulators in registers across the chunks: the order of
//     every sum is fixed and depends on the layer's plan only -- the same bits whatever n, the agent's place or the chunking of agents;
//   * epilogue: + bias per output element, SoftSign, Y only, [c][oy][ox]: into the other scratch map, the last layer's behind the extras
//     of the agent's feature row.
//
// Tile shape (ActConvgLayer::TC x TP, chosen per layer by act_convg_plan): TC = 1, 2 or 4 channel tiles x TP = 2 position tiles per
// wavefront.  The issue that asked for this kernel suggested more position tiles per wavefront for layers of few channels.  Within a
// band of 8 position tiles and four wavefronts every split gives a wavefront the same 2 nCt MFMAs per reduction step, and 2 x 2
// already needs the fewest LDS reads per MFMA; accumulators that idle cost registers, not cycles.  What a narrow layer does waste with
// convg_kernel's fixed 4 x 2 is the LDS of 64 operand rows and the branches around absent tiles: TC is a template parameter, the operand
// slice has 16 TC rows, and the plan spends the LDS on a larger channel chunk (fewer barriers) within a budget of 72 KB where a band
// fits it -- two workgroups per compute unit, one staging while the other multiplies -- and convg.hip's 144 KB otherwise.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; tools/resource_usage.py prints them): no scratch, no VGPR and no SGPR
// spills.  Dynamic LDS is the plan's (at most 144 KB), 0 bytes static.
//   act_convg_dev_kernel<1, first>    VGPR 32   AGPR 8    SGPR 98    scratch 0   8 waves / SIMD
//   act_convg_dev_kernel<1, behind>   VGPR 40   AGPR 8    SGPR 90    scratch 0   8 waves / SIMD
//   act_convg_dev_kernel<2, first>    VGPR 32   AGPR 16   SGPR 102   scratch 0   7 waves / SIMD
//   act_convg_dev_kernel<2, behind>   VGPR 38   AGPR 16   SGPR 94    scratch 0   8 waves / SIMD
//   act_convg_dev_kernel<4, first>    VGPR 47   AGPR 32   SGPR 104   scratch 0   6 waves / SIMD
//   act_convg_dev_kernel<4, behind>   VGPR 47   AGPR 32   SGPR 96    scratch 0   6 waves / SIMD
// (the first layer's loads and the loads from the previous map are two instantiations, and the layer's record is read through a
// reference: with both paths in one body and the record copied the kernel parked 4 to 9 scalar registers in vector lanes)
#include <algorithm>
#include "convg_band.h"

namespace hl {

constexpr size_t ACG_LDS_PREFER = 72 * 1024;      // two workgroups per compute unit
constexpr int ACG_MAX_MAP = 1 << 24;              // floats of a map: int offsets inside an agent's map

// floats of dynamic LDS: window of icc channels | 16 TC operand rows of icc nT reduction elements (+ 4: pitch = 4 mod 32 where that is a
// multiple of 32) | the table of their window offsets | the table of the window columns' slots
__host__ __device__ inline size_t acgLdsFloats(const CgBand& bd, int icc, int nT, int TC) {
  const int red = cgPad4(icc * nT);
  return (size_t)cgPad4(icc * bd.plane) + (size_t)16 * TC * (red + 4) + red + cgPad4(bd.WW);
}
// lanes per row, as a shift: the smallest power of two from 4 on that covers n elements, 64 at most
__device__ __forceinline__ int acgShift(int n) { int sh = 6; while (sh > 2 && (1 << (sh - 1)) >= n) --sh; return sh; }
// the (channel, row) pairs of a window, walked by groups of 2^sh lanes: pair `p` of this group, then every `step`-th
struct AcgPairs {
  int ch, wr, step, WR;
  __device__ __forceinline__ AcgPairs(int p, int step_, int WR_) : ch(0), wr(p), step(step_), WR(WR_) { norm(); }
  __device__ __forceinline__ void norm() { while (wr >= WR) { wr -= WR; ++ch; } }
  __device__ __forceinline__ void next() { wr += step; norm(); }
};

// FIRST: the layer reads the agents' windows of the caller's states (l = 0); else the previous map
template <int TC, bool FIRST>
__global__ __launch_bounds__(256) void act_convg_dev_kernel(ActConvgArgs a, int l) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const ActConvgLayer& g = a.L[l];      // (read where needed: a copy of the record costs scalar registers the loops need)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lc = lane >> 4;
  const int agent = blockIdx.y, c0 = (int)blockIdx.z * 16 * TC;
  const int SY = g.Sy, SX = g.Sx, TA = g.KnY, TB = g.KnX, nT = TA * TB, C = g.InC, SrcY = g.InY, SrcX = g.InX;
  const int RB = g.RB, XB = g.XB, ICC = g.ICC;
  const int nSeg = (g.OpX + XB - 1) / XB, rb = (int)blockIdx.x / nSeg, seg = (int)blockIdx.x - rb * nSeg, u0 = rb * RB, v0 = seg * XB;
  const int nU = min(RB, g.OpY - u0), nV = min(XB, g.OpX - v0), nPos = nU * nV;
  const CgBand bd = cgBand(RB, XB, SY, SX, TA, TB);
  const int redMax = cgPad4(ICC * nT), ldAs = redMax + 4;
  float* sWin = reinterpret_cast<float*>(smem);                        // [ICC][WR][pitch]
  float* sA = sWin + cgPad4(ICC * bd.plane);                           // [16 TC][ldAs]
  int* kOff = reinterpret_cast<int*>(sA + (size_t)16 * TC * ldAs);     // [redMax]
  int* sSlot = kOff + redMax;                                          // [WW]
  const int y0 = u0 * SY - g.Py, x0 = v0 * SX - g.Px;
  const int nCt = min(TC, ((g.KnC + 15) >> 4) - (int)blockIdx.z * TC); // channel tiles of this group
  // the agent's window (first layer) / its map of the layer before
  constexpr bool first = FIRST;
  const long long row0 = first ? a.firstRow[agent] : 0;
  const int last = first ? max(a.nSteps[agent], 1) - 1 : 0, dS = a.dS;
  const float* mp = first ? nullptr : a.src + (size_t)agent * a.mapLd;
  const bool vec = !first && (reinterpret_cast<uintptr_t>(a.src) & 15) == 0;      // (mapLd is a multiple of 4 floats)
  // the extras, standardised, to the front of the feature row: one workgroup per agent
  if (first && blockIdx.x == 0 && blockIdx.z == 0) {
    const int jE = a.img / dS, kE = a.img - jE * dS;
    for (int e = tid; e < a.extras; e += 256) {
      int j = jE, k = kE + e;
      while (k >= dS) { k -= dS; ++j; }
      const float v = a.in[(size_t)(row0 + (long long)max(last - j, 0) * a.rowStride) * dS + k];
      a.feat[(size_t)agent * a.ldF + e] = (v - a.stMean[k]) * a.stScale[k];
    }
  }
  for (int wx = tid; wx < bd.WW; wx += 256) sSlot[wx] = cgSlot(wx, SX, bd.WQ);
  for (int kk = tid; kk < redMax; kk += 256) {
    int off = 0;                                                       // (padding: a zero operand element times a staged value)
    if (kk < ICC * nT) { const int ch = kk / nT, f = kk - ch * nT, aa = f / TB, bb = f - aa * TB; off = ch * bd.plane + aa * bd.pitch + cgSlot(bb, SX, bd.WQ); }
    kOff[kk] = off;
  }
  // this wavefront's position tiles wave, wave + 4: origin of the lane's position in the window
  int org[2], pp[2]; bool ok[2], tOn[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = (wave + 4 * j) * 16 + li;
    tOn[j] = (wave + 4 * j) * 16 < nPos; ok[j] = p < nPos;
    const int pc = ok[j] ? p : 0, ul = pc / nV, vl = pc - ul * nV;
    org[j] = ul * SY * bd.pitch + vl; pp[j] = (u0 + ul) * g.OpX + v0 + vl;
  }
  f32x4 acc[TC][2];
#pragma unroll
  for (int ct = 0; ct < TC; ++ct) { acc[ct][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[ct][1] = acc[ct][0]; }
  const float* aRow = sA + li * ldAs + lc;
  // groups of 2^sh lanes per window row: elements (first layer) or memory-aligned quads (behind it)
  const int sh = acgShift(first ? bd.WW : (bd.WW + 6) >> 2), grp = lane >> sh, ql = lane & ((1 << sh) - 1), nGrp = 64 >> sh;
  __syncthreads();                                                     // the tables
  for (int ch0 = 0; ch0 < C; ch0 += ICC) {
    const int ncc = min(ICC, C - ch0), Kc = ncc * nT, KcP = cgPad4(Kc);
    if (ch0) __syncthreads();                                          // the chunk before has been read
    if (ncc != ICC) for (int kk = Kc + tid; kk < KcP; kk += 256) kOff[kk] = 0;
    for (AcgPairs pr(wave * nGrp + grp, 4 * nGrp, bd.WR); pr.ch < ncc; pr.next()) {
      float* drow = sWin + pr.ch * bd.plane + pr.wr * bd.pitch;
      const int sy = y0 + pr.wr;
      if ((unsigned)sy >= (unsigned)SrcY) { for (int wx = ql; wx < bd.WW; wx += 1 << sh) drow[sSlot[wx]] = 0.f; continue; }
      const int rowOff = ((ch0 + pr.ch) * SrcY + sy) * SrcX;             // the image row's first element in the stacked row / the map
      if (first) {
        const int j0 = rowOff / dS, k0 = rowOff - j0 * dS;             // (once per pair)
        for (int wx = ql; wx < bd.WW; wx += 1 << sh) {
          const int sx = x0 + wx;
          float v = 0.f;
          if ((unsigned)sx < (unsigned)SrcX) {
            int j = j0, k = k0 + sx;
            while (k >= dS) { k -= dS; ++j; }
            v = (a.in[(size_t)(row0 + (long long)max(last - j, 0) * a.rowStride) * dS + k] - a.stMean[k]) * a.stScale[k];
          }
          drow[sSlot[wx]] = v;
        }
      } else {
        const float* prow = mp + rowOff;
        const int s0 = x0 - ((x0 + (rowOff & 3)) & 3), nQ = (x0 + bd.WW - s0 + 3) >> 2;      // prow + s0 lies on a 16-byte boundary
        for (int q = ql; q < nQ; q += 1 << sh) {
          const int sx = s0 + 4 * q;
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (vec && sx >= 0 && sx + 3 < SrcX) v = *reinterpret_cast<const f32x4*>(prow + sx);
          else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if ((unsigned)(sx + e) < (unsigned)SrcX) v[e] = prow[sx + e];
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) { const int wx = sx + e - x0; if ((unsigned)wx < (unsigned)bd.WW) drow[sSlot[wx]] = v[e]; }
        }
      }
    }
    {   // the operand slice: rows of the blob's filter, a group of lanes per row
      const int shA = acgShift(KcP), nGA = 64 >> shA;
      for (int r = wave * nGA + (lane >> shA); r < nCt * 16; r += 4 * nGA) {
        const bool chOk = c0 + r < g.KnC;
        const float* wr = a.W + g.indW + (size_t)(chOk ? c0 + r : 0) * g.K + (size_t)ch0 * nT;
        for (int kk = lane & ((1 << shA) - 1); kk < KcP; kk += 1 << shA) sA[r * ldAs + kk] = (chOk && kk < Kc) ? wr[kk] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll 2
    for (int s = 0; s < (KcP >> 2); ++s) {
      const int off = kOff[4 * s + lc];
      const float b0 = sWin[org[0] + off], b1 = sWin[org[1] + off];
#pragma unroll
      for (int ct = 0; ct < TC; ++ct) {
        if (ct < nCt) {
          const float av = aRow[ct * 16 * ldAs + 4 * s];
          if (tOn[0]) acc[ct][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc[ct][0], 0, 0, 0);
          if (tOn[1]) acc[ct][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc[ct][1], 0, 0, 0);
        }
      }
    }
  }
  float* out = l == a.nL - 1 ? a.feat + (size_t)agent * a.ldF + a.extras : a.dst + (size_t)agent * a.mapLd;
  const float* Bl = a.W + g.indB;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (!ok[j]) continue;
#pragma unroll
    for (int ct = 0; ct < TC; ++ct) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ch = c0 + ct * 16 + lc * 4 + q;
        if (ct < nCt && ch < g.KnC) {
          const float x = acc[ct][j][q] + Bl[(size_t)ch * g.P + pp[j]];
          out[(size_t)ch * g.P + pp[j]] = x / (1 + fabsf(x));          // SoftSign (Functions.h)
        }
      }
    }
  }
}

// a band of at most CONVG_BAND_POS outputs (convg.hip's shrinking order) and the largest chunk of reduction channels beside it within `budget`
static bool acgFit(ActConvgLayer& L, size_t budget) {
  int XB = std::min(L.OpX, CONVG_BAND_POS), RB = std::max(1, std::min(CONVG_BAND_POS / XB, L.OpY));
  for (;;) {
    const CgBand bd = cgBand(RB, XB, L.Sy, L.Sx, L.KnY, L.KnX);
    for (int icc = L.InC; icc >= 1; --icc) {
      const size_t bytes = acgLdsFloats(bd, icc, L.KnY * L.KnX, L.TC) * sizeof(float);
      if (bytes <= budget) { L.RB = RB; L.XB = XB; L.ICC = icc; L.ldsBytes = bytes; return true; }
    }
    if (RB > 1) RB = (RB + 1) / 2; else if (XB > 16) XB = (XB + 1) / 2; else return false;
  }
}
bool act_convg_plan(ActConvgArgs* a) {
  if (a->nL < 1 || a->nL > HL_MAX_CONV || a->dS < 1 || a->dIn < 1) return false;
  long long prev = 0, mapLd = 0;
  for (int l = 0; l < a->nL; ++l) {
    ActConvgLayer& L = a->L[l];
    if (L.InC < 1 || L.InY < 1 || L.InX < 1 || L.KnC < 1 || L.KnY < 1 || L.KnX < 1 || L.OpY < 1 || L.OpX < 1) return false;
    if (L.Sy < 1 || L.Sy > 8 || L.Sx < 1 || L.Sx > 8 || L.Py < 0 || L.Py >= L.KnY || L.Px < 0 || L.Px >= L.KnX) return false;
    if ((long long)(L.OpY - 1) * L.Sy + L.KnY > L.InY + 2 * L.Py || (long long)(L.OpX - 1) * L.Sx + L.KnX > L.InX + 2 * L.Px) return false;
    const long long inSize = (long long)L.InC * L.InY * L.InX, outSize = (long long)L.KnC * L.OpY * L.OpX;
    if (inSize >= ACG_MAX_MAP || outSize >= ACG_MAX_MAP) return false;
    if (l == 0 ? inSize > a->dIn : inSize != prev) return false;
    if (L.K != L.InC * L.KnY * L.KnX || L.P != L.OpY * L.OpX || L.indW < 0 || L.indB < 0) return false;
    const int nCt = (L.KnC + 15) >> 4;
    L.TC = nCt >= 3 ? 4 : nCt; L.TP = 2;
    if (!acgFit(L, ACG_LDS_PREFER) && !acgFit(L, CONVG_LDS_BUDGET)) return false;
    if (l < a->nL - 1) mapLd = std::max(mapLd, (outSize + 3) & ~3LL);
    prev = outSize;
  }
  a->img = a->L[0].InC * a->L[0].InY * a->L[0].InX; a->extras = a->dIn - a->img;
  if (a->extras + prev > ACT_DEV_MAX_ROW) return false;
  a->nF = a->extras + (int)prev; a->mapLd = mapLd;
  return true;
}

template <int TC, bool FIRST> static hipError_t acgLaunchT(const ActConvgArgs& a, int l, dim3 grid, hipStream_t s) {
  hipError_t e = ensureDynLds(reinterpret_cast<const void*>(act_convg_dev_kernel<TC, FIRST>), a.L[l].ldsBytes); if (e != hipSuccess) return e;
  hipLaunchKernelGGL((act_convg_dev_kernel<TC, FIRST>), grid, dim3(256), a.L[l].ldsBytes, s, a, l);
  return hipGetLastError();
}
template <int TC> static hipError_t acgLaunch(const ActConvgArgs& a, int l, dim3 grid, hipStream_t s) {
  return l == 0 ? acgLaunchT<TC, true>(a, l, grid, s) : acgLaunchT<TC, false>(a, l, grid, s);
}
hipError_t launch_act_convg_dev(const ActConvgArgs& a, int l, hipStream_t s) {
  if (l < 0 || l >= a.nL || a.n < 1 || a.n > 65535 || !a.W || !a.feat || a.ldF < a.nF) return hipErrorInvalidValue;
  const ActConvgLayer& L = a.L[l];
  if (L.RB < 1 || L.XB < 1 || L.ICC < 1 || L.TP != 2 || L.ldsBytes == 0 || L.ldsBytes > CONVG_LDS_BUDGET) return hipErrorInvalidValue;
  if (l == 0 && (!a.in || !a.firstRow || !a.nSteps || a.rowStride < 1 || !a.stMean || !a.stScale)) return hipErrorInvalidValue;
  if ((l > 0 && !a.src) || (l < a.nL - 1 && !a.dst) || (a.nL > 1 && (a.mapLd < 4 || (a.mapLd & 3)))) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(((L.OpY + L.RB - 1) / L.RB) * ((L.OpX + L.XB - 1) / L.XB)), (unsigned)a.n, (unsigned)((L.KnC + 16 * L.TC - 1) / (16 * L.TC)));
  switch (L.TC) {
  case 1: return acgLaunch<1>(a, l, grid, s);
  case 2: return acgLaunch<2>(a, l, grid, s);
  case 4: return acgLaunch<4>(a, l, grid, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace hl
