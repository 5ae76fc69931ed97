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
#include "act_conv_dev.h"

namespace hl {

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
