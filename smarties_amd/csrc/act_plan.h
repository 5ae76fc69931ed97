// smarties_amd/csrc/act_plan.h -- the LDS plans of the acting kernels of actband.hip (the device calls of learner_dev.h beyond the resident plans
// act_conv_plan and act_rows_plan): the first conv layer's image in bands of output rows, the first dense layer's input row in panels.
// Host arithmetic on the argument records of kernels.h only, no device call: tests/cpp/act_plan_check.cpp runs it on the CPU
#pragma once
#include <algorithm>
#include <cstddef>
#include "kernels.h"

namespace hl {

constexpr size_t ACT_PLAN_LDS_BUDGET = 160 * 1024;      // (the budget of act_conv_plan and act_rows_plan)
constexpr int ACT_PLAN_NPG = 4;                         // position tiles per unit of work at most (AC_NPG of act_conv_dev.h)
constexpr int ACT_PANEL_MAX = 1024;                     // widest panel; panels are multiples of 32 columns (a batch of arProduct's reduction steps)

// the geometry act_conv_plan checks and the fields it fills that no LDS layout depends on, with feature rows up to ACT_DEV_MAX_ROW;
// tab / buf: floats of the offset tables and of the two map buffers
inline bool act_conv_geometry(ActConvArgs* a, long long* tab, long long (&buf)[2]) {
  if (a->recurrent || a->nL < 1 || a->nL > HL_MAX_CONV || a->dS < 1 || a->dIn < 1) return false;
  long long prev = 0;
  *tab = 0; buf[0] = buf[1] = 0;
  for (int l = 0; l < a->nL; ++l) {
    ActConvLayer& L = a->L[l];
    if (L.InC < 1 || L.InY < 1 || L.InX < 1 || L.KnC < 1 || L.KnY < 1 || L.KnX < 1 || L.S < 1 || L.OpY < 1 || L.OpX < 1) return false;
    if ((long long)(L.OpY - 1) * L.S + L.KnY > L.InY || (long long)(L.OpX - 1) * L.S + L.KnX > L.InX) return false;      // zero padding
    const long long inSize = (long long)L.InC * L.InY * L.InX, outSize = (long long)L.KnC * L.OpY * L.OpX;
    if (inSize >= (1 << 20) || outSize >= (1 << 20)) return false;
    if (l == 0 ? inSize > a->dIn : inSize != prev) return false;
    if (L.K != L.InC * L.KnY * L.KnX || L.P != L.OpY * L.OpX || L.indW < 0 || L.indB < 0) return false;
    L.vec = (L.K & 3) == 0 && (L.indW & 3) == 0;
    L.tabOff = (int)*tab; *tab += (L.K + 15) & ~15;
    if (l < a->nL - 1) buf[l & 1] = std::max(buf[l & 1], (outSize + 3) & ~3LL);
    const int nCT = (L.KnC + 15) >> 4, nPT = (L.P + 15) >> 4;
    L.npg = 1;
    for (int g = ACT_PLAN_NPG; g > 1; --g) if (nCT * ((nPT + g - 1) / g) >= 4) { L.npg = g; break; }
    prev = outSize;
  }
  a->img = a->L[0].InC * a->L[0].InY * a->L[0].InX; a->extras = a->dIn - a->img;
  if (a->extras + prev > ACT_DEV_MAX_ROW) return false;
  a->nF = a->extras + (int)prev;
  a->vec = (a->dIn & 3) == 0 && (a->dS & 3) == 0 && (a->img & 3) == 0;
  return true;
}

// act_conv_plan's layout -- offset tables | image | map buffer 0 | map buffer 1 -- for a net whose feature row is beyond ACT_ROWS_MAXW
// (act_conv_dev_kernel in front of act_rows_panel_kernel)
inline bool act_conv_wide_plan(ActConvArgs* a) {
  long long tab, buf[2];
  if (!act_conv_geometry(a, &tab, buf)) return false;
  a->nb = a->bandR = a->bandRows = a->bandOff = a->bandVec = 0;
  a->imgOff = (int)tab;
  a->bufOff[0] = a->imgOff + ((a->img + 3) & ~3);
  a->bufOff[1] = a->bufOff[0] + (int)buf[0];
  a->ldsBytes = ((size_t)a->bufOff[1] + (size_t)buf[1]) * sizeof(float);
  return a->ldsBytes <= ACT_PLAN_LDS_BUDGET;
}

// band b of a banded first layer: output rows [oy0, oy1), which read the input rows [iy0, iy0 + rows) of every channel
struct ActBand { int oy0, oy1, iy0, rows; };
inline ActBand act_conv_band(const ActConvArgs& a, int b) {
  const ActConvLayer& L = a.L[0];
  ActBand d{};
  d.oy0 = b * a.bandR; d.oy1 = std::min(d.oy0 + a.bandR, L.OpY);
  d.iy0 = d.oy0 * L.S; d.rows = (d.oy1 - d.oy0 - 1) * L.S + L.KnY;
  return d;
}

// act_conv_band_dev_kernel serves this net: offset tables | band buffer [InC][bandRows][InX] | map buffer 0 | map buffer 1 within the budget.
// The smallest band count from 2 on that fits; forceNb > 0: that count (at most OpY), whatever fewer bands would fit.
// false: the geometry, a feature row beyond ACT_DEV_MAX_ROW, or a map that exceeds the LDS at any band count
inline bool act_conv_band_plan(ActConvArgs* a, int forceNb = 0) {
  long long tab, buf[2];
  if (!act_conv_geometry(a, &tab, buf)) return false;
  const ActConvLayer& L = a->L[0];
  for (int want = forceNb > 0 ? std::min(forceNb, L.OpY) : 2; want <= L.OpY; ++want) {
    const int R = (L.OpY + want - 1) / want, nb = (L.OpY + R - 1) / R;      // (bands of R rows: no more of them than hold a row)
    const int rows = (R - 1) * L.S + L.KnY;
    const long long band = ((long long)L.InC * rows * L.InX + 3) & ~3LL;
    const size_t bytes = (size_t)(tab + band + buf[0] + buf[1]) * sizeof(float);
    if (bytes <= ACT_PLAN_LDS_BUDGET) {
      a->nb = nb; a->bandR = R; a->bandRows = rows;
      a->bandOff = (int)tab; a->imgOff = (int)tab;
      a->bufOff[0] = a->bandOff + (int)band;
      a->bufOff[1] = a->bufOff[0] + (int)buf[0];
      a->ldsBytes = bytes;
      // 16-byte loads: states, channels and every band's slice of a channel start and end on multiples of 4 floats
      bool vec = (a->dS & 3) == 0 && ((L.InY * L.InX) & 3) == 0 && ((rows * L.InX) & 3) == 0;
      for (int b = 0; b < nb && vec; ++b) { const ActBand d = act_conv_band(*a, b); vec = ((d.iy0 * L.InX) & 3) == 0 && ((d.rows * L.InX) & 3) == 0; }
      a->bandVec = vec ? 1 : 0;
      return true;
    }
    if (forceNb > 0) return false;
  }
  return false;
}

// act_rows_panel_kernel serves this net: [16][ld] activations of the layers | [16][ldO] output values | [16][pn + 4] panel of the first layer's
// input row within the budget.  The widest panel up to ACT_PANEL_MAX that fits; forcePn > 0: that width.
// false: an input row beyond ACT_DEV_MAX_ROW, a layer beyond ACT_ROWS_MAXW, no room for a panel of 32 columns
inline bool act_rows_panel_plan(ActRowsArgs* a, int forcePn = 0) {
  if (a->nL < 1 || a->nL > HL_MAX_HIDDEN || a->dS < 1 || a->dIn < 1 || a->dIn > ACT_DEV_MAX_ROW || a->nDense < 1 || a->nSig < 0) return false;
  if (a->L[0].nIn != a->dIn || a->nOut != a->nDense + a->nSig || a->ldWo < a->nDense || (a->ldWo & 3)) return false;
  if (forcePn < 0 || (forcePn & 31) || forcePn > ACT_PANEL_MAX) return false;
  int maxW = 0;
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
  a->panOff = 16 * (a->ld + a->ldO);
  const long long room = (long long)(ACT_PLAN_LDS_BUDGET / sizeof(float)) / 16 - a->ld - a->ldO - 4;      // columns of a panel row
  const int pn = forcePn > 0 ? forcePn : (int)std::min<long long>(ACT_PANEL_MAX, room) & ~31;
  if (pn < 32 || pn > room) return false;
  a->pn = pn;
  a->ldsBytes = (size_t)16 * (a->ld + a->ldO + pn + 4) * sizeof(float);
  return true;
}

}  // namespace hl
