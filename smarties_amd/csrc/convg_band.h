// smarties_amd/csrc/convg_band.h -- the band arithmetic the kernels of general conv geometry share (convg.hip: training; actconvg.hip:
// acting from device memory): the LDS window of a band of outputs and where a window column lies in it.  Host and device, no state
#pragma once
#include "dev_common.h"

namespace hl {

__host__ __device__ inline int cgPad4(int k) { return (k + 3) & ~3; }

// the LDS window of a band: WR rows of WW columns per channel, columns de-interleaved by SX into SX runs of WQ slots, odd row pitch
struct CgBand { int WR, WW, WQ, pitch, plane; };
__host__ __device__ inline CgBand cgBand(int RB, int XB, int SY, int SX, int TA, int TB) {
  CgBand b; b.WR = (RB - 1) * SY + TA; b.WW = (XB - 1) * SX + TB; b.WQ = (b.WW + SX - 1) / SX; b.pitch = (SX * b.WQ) | 1; b.plane = b.WR * b.pitch;
  return b;
}
__host__ __device__ inline int cgSlot(int b, int SX, int WQ) { return (b % SX) * WQ + b / SX; }      // window column b (of output column 0) -> slot
constexpr size_t CONVG_LDS_BUDGET = 144 * 1024;
constexpr int CONVG_BAND_POS = 128;      // positions of a band: 8 tiles of 16, two per wavefront

}  // namespace hl
