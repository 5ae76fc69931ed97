// smarties_amd/csrc/fused.hip -- forward + V-RACER head + input-gradient back-propagation of the
// two-hidden-layer MLP as ONE kernel (the cfg-NS class of networks: dS <= 32, two hidden blocks of
// equal width H in {16,32,64,128,256}, dA <= 7).
//
// Why: a gradient step is a chain of dependent kernels, each costing a dispatch gap (~1.6 us), a
// cold L2 (every kernel boundary invalidates it) and a prologue.  fwd0 -> fwd1 -> head -> dX were
// four such kernels for ~40 MFLOP.  Here a 16-row PANEL of the minibatch is owned by a group of
// HT = H/16 workgroups (one 16-column tile each, all on one XCD because workgroups are dealt
// round-robin to the 8 XCDs and the group shares blockIdx % 8); inside the group only ONE exchange
// is needed:
//
//   every WG:  h1 = f(S W0 + b0) for the whole panel (17x256 weights: recomputed, not exchanged)
//              its tile of x2 = h1 W1 + b1, y3 = f(x2) + w*h1 + b and f'(x2), and its SHARE of the output layer,
//              the 16 x 8 partial y3[:, tile] Wout[rows of the tile] (the layer is linear in the columns)
//              -> global (plain stores through the XCD's L2; agent-scope write-through stores if the probe says so)
//   -- group barrier: a counter per panel, one arrive per WG (no returned value: the target comes from a read of the
//      counter issued with the first loads), no L2 flush / invalidate --
//   every WG:  sums the HT partials of the panel's outputs in one fixed association (one round trip of small L2 hits; y3 is
//              not read back), V-RACER head for the 16 samples (fp64, one (sample, action dim) per lane) while the waves
//              that have no part in the head stage f'(x2) of the panel, delta_y3 = delta_out Wout^T,
//              delta_x2 = delta_y3 f'(x2) for the whole panel, its tile of
//              delta_h1 = delta_x2 W1^T (+ residual path), delta_x1 = delta_h1 f'(x1)
//
// The weight-gradient GEMMs need all rows and stay a second kernel (gemm16.hip, role DW).
// Reference functions: BaseLayer::forward / ParametricResidualLayer::forward (Layer_Base.h:64-95,
// Layers.h:347-361), RACER::Train (Learners/RACER_train.cpp:14-67), Continuous_policy
// (Math/Continuous_policy.h:68-378, 569-738), MiniBatch::setMseDklImpw / setValues
// (MiniBatch.h:161-175), Layer::backward (Layers.h:123-160, 363-393).
#include "tail_dev.h"

namespace hl {

#define FLDR 258            // leading dimension of 16-row LDS tiles (== 2 mod 32: conflict-free MFMA operand reads)
#define FLDS 34             // leading dimension of the 16 x dS state tile
#define FMAXK4 8            // dS <= 32: at most 8 MFMA k-steps in the first layer
#ifndef FUSED_NT
#define FUSED_NT 512        // threads per workgroup of the fused kernel
#endif
// chained h1 -> x2 (512 threads, H >= 64): how many wavefronts chain (4: waves 4-7, the others run the fp64 head terms beside them;
// 8: all of them, H >= 128) and where those head terms sit (0: beside / behind the chain, 1: under the wait of the panel barrier).
// The shipped values are the ones measured fastest (docs/EXPERIMENTS.md); the others build for comparison.  With 4 every weight keeps
// the bits of the panel form; with 8 the K split is finer (redSum<8>).
#ifndef FUSED_CHAINW
#define FUSED_CHAINW 8
#endif
#ifndef FUSED_PRE_LATE
#define FUSED_PRE_LATE 1
#endif
// h1 product: 1 = straight-line code per k-step count with every operand read up front (h1Product), 0 = the loop that reads the
// operands of step s + 1 under the MFMAs of step s (the compiler serialises it: one full LDS wait per step).  Same bits either way.
#ifndef FUSED_H1_PRE
#define FUSED_H1_PRE 1
#endif
// 1: what the first batch of loads needs is taken as ONE batch of scalar loads in front of everything else (see the kernel)
#ifndef FUSED_ARGS_FIRST
#define FUSED_ARGS_FIRST 1
#endif
#define FTLD 17             // leading dimension of the own-tile scratch of the chained form (x1 at 0, h1 at 16 * FTLD + 16)

// development time stamps of workgroup (panel 0, tile 1), 100 MHz clock: -DHL_FSTAMPS (its own flag: the tail stamps of
// -DHL_TAIL_STAMPS use the same slots of DevScalars::dbgT)
#if defined(HL_FSTAMPS)
#ifndef HL_FSTAMP_PANEL
#define HL_FSTAMP_PANEL 0      // (another panel: a workgroup in the crowd of a larger batch)
#endif
#define FSTAMP(i) do { if (threadIdx.x == 0 && panel == HL_FSTAMP_PANEL && n == 1) a.sc->dbgT[i] = wall_clock64(); } while (0)
// the same for thread t: the first lane of the wavefront that chains this tile (slots 14 - 16 of the chained form)
#define FSTAMPT(t, i) do { if (threadIdx.x == (t) && panel == HL_FSTAMP_PANEL && n == 1) a.sc->dbgT[i] = wall_clock64(); } while (0)
#else
#define FSTAMP(i) do { } while (0)
#define FSTAMPT(t, i) do { } while (0)
#endif

// (-DHL_FSTAMPS) when does the LAST workgroup of each kind finish?  dbgT[20] ordinary panels, [21] panels with next-state rows (they
// start with a dependent load of the row count), [22] the sampler rider, [23] the far-policy / beta rider -- maxima of a monotonic clock:
// after a call they belong to its last launch, like the entry stamp dbgT[31]
#if defined(HL_FSTAMPS)
#define FEND(i) do { __syncthreads(); if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned long long*>(&a.sc->dbgT[i]), (unsigned long long)wall_clock64()); } while (0)
#else
#define FEND(i) do { } while (0)
#endif

// development: stop after phase n (tools/ktime4.py; library built with HL_EXTRA_FLAGS=-DHL_DEV) -- compiled out otherwise
#ifdef HL_DEV
#define FVARIANT_STOP(n) do { if (a.variant == (n)) return; } while (0)
#else
#define FVARIANT_STOP(n) do { } while (0)
#endif

// LDS carve-up (floats).  R1: h1 panel (chained form: unused until then), later the W1 row tile of the dX contraction.  R2: W0
// (k-major, leading dimension H+16).  R3: W1 column tile, later f'(x2) -> delta_x2 panel.
__host__ __device__ inline int fusedR2Floats(int dSp, int H) { return dSp * (H + 16); }
__host__ __device__ inline int fusedR3Floats(int H) { const int a = H * 16, b = 16 * FLDR; return a > b ? a : b; }
__host__ __device__ inline size_t fusedLdsBytes(int dS, int H) {
  const int dSp = (dS + 3) & ~3;
  const size_t fl = (size_t)16 * FLDR + fusedR2Floats(dSp, H) + fusedR3Floats(H) + (size_t)H * 8 /*Wout*/ + 16 * FLDS +
                    2048 /*red*/ + 3 * (size_t)H /*b0, wres, bres*/ + 512 /*sO*/ + 128 /*sDo*/ + 2 * (16 * FTLD + 16) /*own tile scratch: x1, h1*/ + 32 /*bo, bp*/ + 4 /*beta hand-off*/;
  const size_t bytes = fl * 4;
  return bytes > TAIL_LDS_BYTES ? bytes : TAIL_LDS_BYTES;
}

// C[16x16] partial of one wave: sum over its k range of A[i][k] * B[k][j]; operands read from LDS
// through the two index functors, ALL of them before the first MFMA (one exposed LDS latency)
template <int NK, class FA, class FB>
__device__ __forceinline__ f32x4 waveMma(FA fa, FB fb) {
  float av[NK], bv[NK];
#pragma unroll
  for (int s = 0; s < NK; ++s) { av[s] = fa(s); bv[s] = fb(s); }
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < NK; ++s) {
    if (s & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc1, 0, 0, 0);
    else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc0, 0, 0, 0);
  }
  return acc0 + acc1;
}

// The first layer's product S W0 over a run-time count of k-steps (dSp / 4 = 1..8) as straight-line code per count: every operand
// of the product is requested before its first MFMA (one exposed LDS latency, like waveMma), where a loop over the count waits for
// the LDS in every step.  One operand is shared by the NTL tiles of the wavefront (fs(s)), the other is the tile's own (ft(s, t));
// TILE_A says which of the two is the A operand.  Step order and the accumulator of every step are those of the loop: for s, for t.
// No padding to a fixed count: a step with zero operands could turn a -0 into +0.
template <int NQ, int NTL, bool TILE_A, class FS, class FT>
__device__ __forceinline__ void h1Steps(f32x4* acc, FS fs, FT ft) {
  float sv[NQ], tv[NQ][NTL];
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    sv[s] = fs(s);
#pragma unroll
    for (int t = 0; t < NTL; ++t) tv[s][t] = ft(s, t);
  }
  __builtin_amdgcn_sched_barrier(0);      // (the scheduler would otherwise sink half of the reads between the MFMAs to save registers)
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
#pragma unroll
    for (int t = 0; t < NTL; ++t) {
      if constexpr (TILE_A) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(tv[s][t], sv[s], acc[t], 0, 0, 0);
      else acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(sv[s], tv[s][t], acc[t], 0, 0, 0);
    }
  }
}
template <int NTL, bool TILE_A, class FS, class FT>
__device__ __forceinline__ void h1Product(int nk4, f32x4* acc, FS fs, FT ft) {      // nk4 is wave-uniform: a scalar branch
  switch (nk4) {
    case 1: h1Steps<1, NTL, TILE_A>(acc, fs, ft); break;
    case 2: h1Steps<2, NTL, TILE_A>(acc, fs, ft); break;
    case 3: h1Steps<3, NTL, TILE_A>(acc, fs, ft); break;
    case 4: h1Steps<4, NTL, TILE_A>(acc, fs, ft); break;
    case 5: h1Steps<5, NTL, TILE_A>(acc, fs, ft); break;
    case 6: h1Steps<6, NTL, TILE_A>(acc, fs, ft); break;
    case 7: h1Steps<7, NTL, TILE_A>(acc, fs, ft); break;
    case 8: h1Steps<8, NTL, TILE_A>(acc, fs, ft); break;
    default: break;
  }
}

// NT threads per workgroup (256 or 512): threads 0..255 own one output element / one (sample, action
// component) each; with 512 the panel-wide phases and the K-split contractions are spread over 8 waves
// sum of the K-split partial tiles (fixed association: pairs, then pairs of pairs)
template <int NP> __device__ __forceinline__ float redSum(const float* red, int tid) {
  if constexpr (NP == 8) return ((red[tid] + red[256 + tid]) + (red[512 + tid] + red[768 + tid])) + ((red[1024 + tid] + red[1280 + tid]) + (red[1536 + tid] + red[1792 + tid]));
  else return (red[tid] + red[256 + tid]) + (red[512 + tid] + red[768 + tid]);
}

// sum of N values held in registers, same association as redSum (pairs, then pairs of pairs, ...)
template <int N> __device__ __forceinline__ float treeSum(const float* v) {
  if constexpr (N == 1) return v[0];
  else return treeSum<N / 2>(v) + treeSum<N / 2>(v + N / 2);
}

template <int H, int CF, int NT>
__global__ __launch_bounds__(NT, NT / 128) void fused_fwd_head_dx_kernel(FusedArgs a, ExtraArgs extra) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // blocks 0..7: riders (tail work of the neighbouring steps); 8 of them keep blockIdx % 8 == XCD
  if (blockIdx.x < 8) {
    if (threadIdx.x >= 256) return;            // the tail code is written for 256 threads
    // the sampler runs in block 0; with PH_PUBLISH its gather is spread over blocks 1..7
    if (blockIdx.x == 0) { if (extra.role == 1) { samplePhases(extra.samp, extra.phases, smem); FEND(22); } }      // (the bookkeeping never rides here: its register needs exceed this kernel's 128)
    else if (blockIdx.x == 1 && (a.deferBeta || extra.post.mode == POST_ENCODE)) { farBetaPhase(extra.post, smem); if (threadIdx.x == 0) a.sc->dbgT[23] = wall_clock64(); }      // what the bookkeeping of the step before left over
    else if (extra.role == 1 && (extra.phases & PH_PUBLISH)) gatherHelper(extra.samp, blockIdx.x - 1, 7, smem);
    return;
  }
  constexpr int HT = H / 16, H4 = H / 4, LDW0 = H + 16;
  constexpr int NW = NT / 64;                    // waves per workgroup
  constexpr int KWAVES = (H / 4 >= NW) ? NW : 4; // waves sharing the reduction of the K-split contractions
  constexpr int KW = H / KWAVES;                 // reduction length per wave
  constexpr int NK = KW / 4;                     // MFMA steps per wave
  constexpr int TPW = HT >= NW ? HT / NW : 1;    // h1 column tiles per wave
  constexpr int QP = (16 * H4 + NT - 1) / NT;    // float4 per thread of a 16 x H panel
  constexpr int QC = (H * 4 + NT - 1) / NT;      // float4 per thread of the H x 16 column tile
  constexpr int QO = (H * 2 + NT - 1) / NT;      // float4 per thread of Wout [H][8]
  constexpr int Q0 = (32 * H4 + NT - 1) / NT;    // float4 per thread of W0 (dS <= 32)
  constexpr int QS = 512 / NT;                   // state-tile elements per thread
  // chained form: the wavefronts that contract x2 compute the h1 tiles of their own K range with swapped operands, so that the
  // accumulators of the first product are the A operand of the second (no h1 panel in LDS, no barrier between the two)
  constexpr bool CHAIN = (NW == 8 && H >= 64);
  constexpr int CW = (FUSED_CHAINW == 8 && H >= 128) ? 8 : 4;      // chaining wavefronts
  constexpr int CT = CHAIN ? H / (16 * CW) : 1;                    // h1 tiles per chaining wavefront
  constexpr int CTID = CW == 8 ? 0 : 256;                          // (stamps) first lane of the wavefront that chains tile 1
  constexpr int TLD = CHAIN ? FTLD : 16;                           // own-tile scratch: leading dimension, offset of the h1 tile
  constexpr int TY1 = 16 * FTLD + 16;
#if defined(HL_FSTAMPS)
  if (threadIdx.x == 0 && blockIdx.x == 8 + 8) a.sc->dbgT[31] = wall_clock64();   // (panel 0, tile 1): kernel entry
#endif
#ifdef HL_TAIL_STAMPS
  if (threadIdx.x == 0 && blockIdx.x == 8 + 8) a.sc->dbgT[31] = wall_clock64();
#endif
#ifdef HL_STEP_STAMPS
  if (threadIdx.x == 0 && blockIdx.x == 8 + 8) a.sc->dbgStep[a.sc->nGradSteps & 63] = wall_clock64();      // tools/step_stamps.py
#endif
  // what the first batch of loads needs (weights, states, vectors, the panel counter).  FUSED_ARGS_FIRST: held in scalar registers
  // at this point, so that they come as ONE batch of scalar loads with one wait; otherwise the compiler fetches the arguments batch
  // by batch in program order, each batch with a wait of its own, and this one comes last
  const DevScalars* sc = a.sc;
  const float* W = a.W; const float* X0 = a.X0; unsigned* panelCtr = a.panelCtr;
  long long iW0 = a.indW0, iW1 = a.indW1, iWo = a.indWo, iB0 = a.indB0, iB1 = a.indB1, iWr = a.indWr, iBr = a.indBr, iBo = a.indBo, iBp = a.indBp;
  int ldW0 = a.ldW0, ldW1 = a.ldW1, ldX0 = a.ldX0, dSa = a.dS, Ba = a.B, parity = a.parity;
#if FUSED_ARGS_FIRST
  // (inputs only: the compiler still knows where the values come from -- global pointers, kernel arguments)
  asm volatile("" :: "s"(W), "s"(iW0), "s"(iW1), "s"(iWo), "s"(iB0), "s"(iB1), "s"(iWr), "s"(iBr), "s"(iBo), "s"(iBp),
               "s"(X0), "s"(panelCtr), "s"(sc), "s"(ldW0), "s"(ldW1), "s"(ldX0), "s"(dSa), "s"(Ba), "s"(parity),
               "s"(a.bt.nextSrc), "s"(a.bt.slot), "s"(a.bt.eid));
#endif
  const int dS = dSa, dSp = (dS + 3) & ~3, B = Ba, dA = a.dA, nDense = a.nDense;
  // arguments used inside the hot loops, pinned in VGPRs: under SGPR pressure the compiler would
  // otherwise re-load them from the kernarg segment at every use (~1 us per epilogue)
  const int func = __builtin_amdgcn_readfirstlane(a.func);
  int resN = a.resN, ldA0 = a.ldA0, ldA1 = a.ldA1;
  float* gR2 = a.R2; float* gX2 = a.X2; float* gD2 = a.D2; float* gDres2 = a.Dres2;
#define FUSED_PIN_ARGS() do { asm volatile("" : "+v"(resN), "+v"(ldA0), "+v"(ldA1)); asm volatile("" : "+v"(gR2), "+v"(gX2), "+v"(gD2), "+v"(gDres2)); } while (0)
#if !FUSED_ARGS_FIRST
  FUSED_PIN_ARGS();
#endif
  const int bid = blockIdx.x - 8, xcd = bid & 7, gi = bid >> 3;
  const int panel = (gi / HT) * 8 + xcd, n = gi % HT;
  const int m0 = panel * 16, n0 = n * 16;
  // panels made of sampled rows only never wait for the row count of this minibatch
  int nRows = B;
  if (m0 + 16 > B) { nRows = sc->nRows[parity]; if (m0 >= nRows) return; }
  FSTAMP(0);

  float* sY1 = reinterpret_cast<float*>(smem);                 // [16][FLDR]
  float* sR2 = sY1 + 16 * FLDR;
  float* sR3 = sR2 + fusedR2Floats(dSp, H);
  float* sWo = sR3 + fusedR3Floats(H);                         // [H][8]
  float* sS = sWo + H * 8;                                     // [16][FLDS]
  float* red = sS + 16 * FLDS;                                 // [8][256]
  float* sB0 = red + 2048;                                     // [H]
  float* sWr = sB0 + H;                                        // [H] residual w
  float* sBr = sWr + H;                                        // [H] residual b
  double* sO = reinterpret_cast<double*>(sBr + H);             // [16][16]  (offset is a multiple of 8 bytes)
  float* sDo = reinterpret_cast<float*>(sO + 256);             // [16][8]
  float* sT = sDo + 128;                                       // own-tile scratch: x1 [16][16]; chained form: x1 and h1, [16][FTLD] each
  float* sBo = sT + 2 * (16 * FTLD + 16);                      // [16] output bias, [16] ParamLayer bias
  float* sBp = sBo + 16;
  double* sBeta = reinterpret_cast<double*>(sBp + 16);          // [0] beta of this step, [1] != 0: it has arrived (deferBeta)

  const int tid = threadIdx.x, lane = tid & 63;
  __builtin_assume(tid >= 0 && tid < NT);      // lets the `tid + NT * q < count` guards of full chunks fold away
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: scalar branches on it
  const int li = lane & 15, lc = lane >> 4;
  const bool eth = tid < 256;                                  // element thread: owns output element / (sample, dim) (em, en)
  const int em = (tid >> 4) & 15, en = tid & 15;
  const float* W0 = W + iW0; const float* W1 = W + iW1; const float* Wo = W + iWo;

  // ---- every load that does not depend on the exchange, issued up front --------------------------
  const int row = m0 + em;
  const bool rowValid = eth && row < nRows, isNext = rowValid && row >= B;
  int bSrc = 0; long long slot = 0;
  if (rowValid) { bSrc = isNext ? a.bt.nextSrc[row - B] : row; slot = a.bt.slot[bSrc]; }   // oldest loads: the gathers hang off them
  int eidv = 0;
  if (rowValid && !isNext) eidv = a.bt.eid[row];
  float sv[QS];
#pragma unroll
  for (int q = 0; q < QS; ++q) {
    const int idx = tid + NT * q, r = idx >> 5, c = idx & 31;
    sv[q] = (c < dS && m0 + r < nRows) ? X0[(size_t)(m0 + r) * ldX0 + c] : 0.f;
  }
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 w0v[Q0], w1c[QC], w1r[QP], wov[QO];
  const int nW0 = dSp * H4;
#pragma unroll
  for (int q = 0; q < Q0; ++q) {
    // no guards: rows >= dS read row dS-1 again (finite weights) and meet state columns that are zero, so they add
    // exactly 0; a guarded load would make the compiler wait for it at the join, ahead of all the loads below
    const int f = tid + NT * q, k = f / H4, c4 = f % H4;
    w0v[q] = *reinterpret_cast<const f32x4*>(W0 + (size_t)(k < dS ? k : dS - 1) * ldW0 + 4 * c4);
  }
#pragma unroll
  for (int q = 0; q < QC; ++q) {
    const int f = tid + NT * q; w1c[q] = z4;
    if (f < H * 4) { const int k = f >> 2, c = n0 + (f & 3) * 4; w1c[q] = *reinterpret_cast<const f32x4*>(W1 + (size_t)k * ldW1 + c); }
  }
#pragma unroll
  for (int q = 0; q < QO; ++q) { const int f = tid + NT * q; wov[q] = f < H * 2 ? *reinterpret_cast<const f32x4*>(Wo + (size_t)f * 4) : z4; }
  const float b0v = tid < H ? W[iB0 + tid] : 0.f;
  const float wrv = tid < H ? W[iWr + tid] : 0.f, brv = tid < H ? W[iBr + tid] : 0.f;
  const float b1e = eth ? W[iB1 + n0 + en] : 0.f;
  const float bov = tid < nDense ? W[iBo + tid] : 0.f, bpv = tid < dA ? W[iBp + tid] : 0.f;
  double beta = sc->beta; const double Cmax = sc->Cmax, Cinv = sc->Cinv;
  const long long betaWant = sc->nGradSteps;      // (deferBeta: the rider in block 1 publishes beta under this number)
  // the panel's arrive counter as it stands before this workgroup's own arrival: it advances by HT per launch (the whole group of a
  // panel runs or leaves), so any such value lies in [base, base + HT - 1] and gives the barrier's target without a returning atomic
  unsigned ctr0 = 0;
  if constexpr (HT > 1) ctr0 = __hip_atomic_load(panelCtr + panel * 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#if FUSED_ARGS_FIRST
  FUSED_PIN_ARGS();      // behind the first batch: the arguments of the later phases
#endif
  // ---- stage: states, W0 (k-major), W1 column tile (k-major), Wout, vectors ------------------------
#pragma unroll
  for (int q = 0; q < QS; ++q) { const int idx = tid + NT * q, r = idx >> 5, c = idx & 31; sS[r * FLDS + c] = sv[q]; }
#pragma unroll
  for (int q = 0; q < Q0; ++q) {
    const int f = tid + NT * q;
    if (f < nW0) { const int k = f / H4, c4 = f % H4; *reinterpret_cast<f32x4*>(sR2 + k * LDW0 + 4 * c4) = w0v[q]; }
  }
#pragma unroll
  for (int q = 0; q < QC; ++q) { const int f = tid + NT * q; if (f < H * 4) *reinterpret_cast<f32x4*>(sR3 + (size_t)f * 4) = w1c[q]; }
#pragma unroll
  for (int q = 0; q < QO; ++q) { const int f = tid + NT * q; if (f < H * 2) *reinterpret_cast<f32x4*>(sWo + (size_t)f * 4) = wov[q]; }
  if (tid < H) { sB0[tid] = b0v; sWr[tid] = wrv; sBr[tid] = brv; }
  if (tid < 16) { sBo[tid] = bov; sBp[tid] = bpv; }
  __syncthreads();
  FSTAMP(1);
  FVARIANT_STOP(1);
  // the W1 row tile is needed only by the dX contraction: fetched now, behind the critical first batch
#pragma unroll
  for (int q = 0; q < QP; ++q) {
    const int f = tid + NT * q; w1r[q] = z4;
    if (f < 16 * H4) { const int r = f / H4, c4 = f % H4; w1r[q] = *reinterpret_cast<const f32x4*>(W1 + (size_t)(n0 + r) * a.ldW1 + 4 * c4); }
  }
  // publishing workgroup of the sample: the aggregates of the sampled episode travel with it to the
  // bookkeeping pass, which then needs no dependent gather (the store happens at the very end)
  // (issued here, behind the first batch and its barrier: they hang off `slot` / `eid`, and a dependent load in the
  // prologue makes everything after it wait for a second HBM round trip)
  const bool aggOwner = ((em & (HT - 1)) == n) && rowValid && !isNext && en < AGG_N;

  // the replay rows of the head (issued now, consumed after the exchange): one (sample, dim) per thread
  double act = 0, bMean = 0, bStd = 1; float misc = 0.f;
  if (rowValid && !isNext && en < dA) {
    act = a.rp.A[(size_t)slot * dA + en];
    bMean = a.rp.MU[(size_t)slot * 2 * dA + en]; bStd = a.rp.MU[(size_t)slot * 2 * dA + dA + en];
  }
  if (rowValid) {   // lanes 0..5: RET, DQ, DKL, IMPW, V, ADV of the sampled step; next rows: lanes 6, 7: V, ADV of t+1
    const float* arr = nullptr; long long sl = slot;
    if (!isNext) arr = en == 0 ? a.rp.RET : en == 1 ? a.rp.DQ : en == 2 ? a.rp.DKL : en == 3 ? a.rp.IMPW : en == 4 ? a.rp.V : en == 5 ? a.rp.ADV : nullptr;
    else { arr = en == 6 ? a.rp.V : en == 7 ? a.rp.ADV : nullptr; sl = slot + 1; }
    if (arr) misc = arr[sl];
  }

  float aggv = 0.f;
  if constexpr (CHAIN) {      // (nothing between here and the x2 barrier for the element threads to wait behind)
    asm volatile("" : "+v"(eidv));
    if (aggOwner) aggv = en < AGG_USED ? a.rp.epAgg[(size_t)eidv * AGG_N + en] : (en == AGG_LEN ? (float)a.rp.epN[eidv] : 0.f);
  }

  // ---- head terms that do not depend on the network outputs of this step (the policy stdev comes
  // from the ParamLayer bias alone).  With 8 waves the element threads (waves 0-3) compute them
  // while waves 4-7 run the x2 contraction; with 4 waves they follow the exchange stores. ------------
  const bool live = rowValid && !isNext;
  const double MAXM = 8.31776613503286;
  double stdev = 1, invStd = 1, dPos = 0, bInv = 1, invVarMu = 1, u2 = 0, lq = 0, CmuCpi = 1;
  bool bnd = false;
  auto headPrecompute = [&]() {
    asm volatile("" : "+v"(act), "+v"(bMean), "+v"(bStd));   // keep the fp64 work (and its wait on the gathers) here
    if (live && en < dA) {
      bnd = ((a.boundedMask >> en) & 1ull) != 0;
      const double pp = (double)sBp[en];
      const double rt = sqrt(1 + pp * pp);
      stdev = (pp + rt) / 2; invStd = 1 / stdev; dPos = (1 + pp / rt) / 2;
      bInv = 1 / bStd; invVarMu = 1 / (bStd * bStd);
      u2 = (act - bMean) * bInv;
      const double qq = stdev * bInv;
      lq = log(qq); CmuCpi = qq * qq;
    }
  };

  float x1o = 0.f, y1o = 0.f;
  if constexpr (!CHAIN) {
  // ---- h1 = f(S W0 + b0), whole panel: wave w computes column tiles w, w+4, ... --------------------
  if (wave < HT) {
    f32x4 acc[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) acc[t] = z4;
    const int nk4 = dSp >> 2;
    float bb[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) bb[t] = sB0[(wave + NW * t) * 16 + li];      // (depends on nothing: requested with the operands)
#if FUSED_H1_PRE
    h1Product<TPW, false>(nk4, acc, [&](int s) { return sS[li * FLDS + 4 * s + lc]; },
                          [&](int s, int t) { return sR2[(4 * s + lc) * LDW0 + (wave + NW * t) * 16 + li]; });
#else
    // operands of step s+1 are read while the MFMAs of step s run
    float av = sS[li * FLDS + lc], bv[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) bv[t] = sR2[lc * LDW0 + (wave + NW * t) * 16 + li];
    for (int s = 0; s < nk4; ++s) {
      const int kn = s + 1 < nk4 ? 4 * (s + 1) + lc : lc;
      const float avn = sS[li * FLDS + kn];
      float bvn[TPW];
#pragma unroll
      for (int t = 0; t < TPW; ++t) bvn[t] = sR2[kn * LDW0 + (wave + NW * t) * 16 + li];
#pragma unroll
      for (int t = 0; t < TPW; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[t], acc[t], 0, 0, 0);
      av = avn;
#pragma unroll
      for (int t = 0; t < TPW; ++t) bv[t] = bvn[t];
    }
#endif
    FSTAMP(14);
    dispatchFunc<CF>(func, [&](auto F) {
      constexpr int FN = decltype(F)::value;
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int nt = wave + NW * t;
        const int c = nt * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = lc * 4 + r;
          const float x = acc[t][r] + bb[t];
          sY1[i * FLDR + c] = actEvalT<FN>(x);
          if (nt == n) sT[i * 16 + li] = x;
        }
      }
    });
  }
  FSTAMP(15);
  __syncthreads();
  x1o = sT[em * 16 + en]; y1o = sY1[em * FLDR + n0 + en];
  FSTAMP(2);
  FVARIANT_STOP(2);
  if (eth && row < B) a.Y1[(size_t)row * ldA0 + n0 + en] = y1o;     // A operand of the dW1 contraction
  asm volatile("" : "+v"(eidv));      // keeps the index arithmetic (and the wait for the load) from being hoisted into the prologue
  if (aggOwner) aggv = en < AGG_USED ? a.rp.epAgg[(size_t)eidv * AGG_N + en] : (en == AGG_LEN ? (float)a.rp.epN[eidv] : 0.f);
  }
  constexpr bool SPLITW = (NW == 8 && H >= 16);      // waves 4-7 contract, waves 0-3 do the fp64 terms
  constexpr int XW = CHAIN ? CW : (SPLITW ? 4 : KWAVES);      // waves sharing the x2 contraction
  constexpr int XKW = H / XW, XNK = XKW / 4;

  if constexpr (CHAIN) {
    // ---- h1 tiles of this wave's K range, then straight on to its share of x2 = h1 W1 + b1.  The first product runs with the
    // operands exchanged, x1^T = W0^T S^T: lane (li, lc) supplies W0[4s + lc][column of row li] as A and S[li][4s + lc] as B and
    // gets acc[r] = x1[sample li][row 4 lc + r of the tile] back -- the sample it supplies as A of the second product.  Row i of
    // the tile is column c0 + (i >> 2) + 4 (i & 3), so acc[r] is column c0 + 4 r + lc: step (tile, r) of the second product
    // contracts k = c0 + 4 r + lc, lc = 0..3, against W1[k][n0 + li] -- the k grouping, the step order and the accumulator of
    // every step are those of waveMma over the h1 panel, and so are the bits of x2 ----------------------------------------------
    const int cw = CW == 8 ? wave : wave - 4;
    if (cw >= 0) {
      const int cb = cw * XKW;                         // first h1 column = first k of this wave
      const int pc = (li >> 2) + 4 * (li & 3);
      // B operands of the second product, requested before the first MFMA: R3 is staged
      float w1b[CT][4];
#pragma unroll
      for (int t = 0; t < CT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) w1b[t][r] = sR3[(cb + 16 * t + 4 * r + lc) * 16 + li];
      }
      f32x4 acc[CT];
#pragma unroll
      for (int t = 0; t < CT; ++t) acc[t] = z4;
      const int nk4 = dSp >> 2;
      // the bias of the h1 tiles depends on nothing: requested with the operands, consumed behind the product
      float bb[CT][4];
#pragma unroll
      for (int t = 0; t < CT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) bb[t][r] = sB0[cb + 16 * t + 4 * r + lc];
      }
#if FUSED_H1_PRE
      h1Product<CT, true>(nk4, acc, [&](int s) { return sS[li * FLDS + 4 * s + lc]; },
                          [&](int s, int t) { return sR2[(4 * s + lc) * LDW0 + cb + 16 * t + pc]; });
#else
      // operands of step s+1 are read while the MFMAs of step s run
      float bv = sS[li * FLDS + lc], av[CT];
#pragma unroll
      for (int t = 0; t < CT; ++t) av[t] = sR2[lc * LDW0 + cb + 16 * t + pc];
      for (int s = 0; s < nk4; ++s) {
        const int kn = s + 1 < nk4 ? 4 * (s + 1) + lc : lc;
        const float bvn = sS[li * FLDS + kn];
        float avn[CT];
#pragma unroll
        for (int t = 0; t < CT; ++t) avn[t] = sR2[kn * LDW0 + cb + 16 * t + pc];
#pragma unroll
        for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], bv, acc[t], 0, 0, 0);
        bv = bvn;
#pragma unroll
        for (int t = 0; t < CT; ++t) av[t] = avn[t];
      }
#endif
      FSTAMPT(CTID, 14);
      // bias and activation in place; the workgroup's own column tile also goes to LDS, x1 and h1, for the element threads
      // (residual path, A operand of dW1, f'(x1))
      dispatchFunc<CF>(func, [&](auto F) {
        constexpr int FN = decltype(F)::value;
#pragma unroll
        for (int t = 0; t < CT; ++t) {
          const bool own = cb + 16 * t == n0;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float x = acc[t][r] + bb[t][r], y = actEvalT<FN>(x);
            acc[t][r] = y;
            if (own) { sT[li * TLD + 4 * r + lc] = x; sT[TY1 + li * TLD + 4 * r + lc] = y; }
          }
        }
      });
      FSTAMPT(CTID, 15);
      f32x4 xa0 = z4, xa1 = z4;
#pragma unroll
      for (int t = 0; t < CT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (r & 1) xa1 = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[t][r], w1b[t][r], xa1, 0, 0, 0);
          else xa0 = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[t][r], w1b[t][r], xa0, 0, 0, 0);
        }
      }
      const f32x4 xacc = xa0 + xa1;
#pragma unroll
      for (int r = 0; r < 4; ++r) red[cw * 256 + (lc * 4 + r) * 16 + li] = xacc[r];
      FSTAMPT(CTID, 16);
      if (CW == 8 && !FUSED_PRE_LATE) headPrecompute();
    } else if (!FUSED_PRE_LATE) headPrecompute();
    FSTAMP(2);
    FVARIANT_STOP(2);
  } else {
  // ---- own tile of x2 = h1 W1 + b1: K split over XW waves ------------------------------------------------
    const int xw = SPLITW ? wave - 4 : wave;
    if (xw >= 0 && xw < XW) {
      const int k0 = xw * XKW + lc;
      const f32x4 acc = waveMma<XNK>([&](int s) { return sY1[li * FLDR + k0 + 4 * s]; }, [&](int s) { return sR3[(k0 + 4 * s) * 16 + li]; });
#pragma unroll
      for (int r = 0; r < 4; ++r) red[xw * 256 + (lc * 4 + r) * 16 + li] = acc[r];
    } else if (SPLITW) headPrecompute();
  }
  __syncthreads();
  FSTAMP(3);
  if constexpr (CHAIN) {
    x1o = sT[em * TLD + en]; y1o = sT[TY1 + em * TLD + en];
    if (eth && row < B) a.Y1[(size_t)row * ldA0 + n0 + en] = y1o;     // A operand of the dW1 contraction
  }
  float y3 = 0.f;      // (padding rows: zero, they add nothing to the partial outputs)
  if (rowValid) {
    const float v = redSum<XW>(red, tid);
    const float x2 = v + b1e;
    float y2 = 0.f, f2 = 0.f;
    dispatchFunc<CF>(func, [&](auto F) { constexpr int FN = decltype(F)::value; y2 = actEvalT<FN>(x2); f2 = actDiffT<FN>(x2, y2); });
    y3 = (n0 + en < resN) ? resOut(y2, y1o, sWr[n0 + en], sBr[n0 + en]) : y2;
    // plain stores: the consumers are the workgroups of this panel, which share this XCD's L2 (the vector L1 is
    // write-through); other XCDs see y3 after the kernel boundary.  Agent-scope (write-through) stores made the
    // acknowledgement wait below ~1 us longer.
    if (a.xcdSafe) {      // (the probe found workgroups of a panel on different XCDs: through the coherence point)
      __hip_atomic_store(gR2 + (size_t)row * ldA1 + n0 + en, y3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(gX2 + (size_t)row * ldA1 + n0 + en, f2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      gR2[(size_t)row * ldA1 + n0 + en] = y3;                // also the A operand of dWout
      gX2[(size_t)row * ldA1 + n0 + en] = f2;                // f'(x2)
    }
  }
  // ---- this tile's share of the output layer, O[16][8] += y3[:, tile n] Wout[rows of tile n]: the layer is linear in the
  // columns, so the 16 x 8 partial travels with the exchange and nobody reads the y3 panel back.  Lane en multiplies its y3 with
  // row n0 + en of Wout; the sum over the 16 lanes of a sample is the rotation butterfly of sum16 (every lane gets it) ----
  float pOwn = 0.f;     // lane en < 8: partial O[em][en] of this tile
  if (wave < 4) {
    const f32x4 wa = *reinterpret_cast<const f32x4*>(sWo + (n0 + en) * 8), wb = *reinterpret_cast<const f32x4*>(sWo + (n0 + en) * 8 + 4);
    float p[8] = {y3 * wa[0], y3 * wa[1], y3 * wa[2], y3 * wa[3], y3 * wb[0], y3 * wb[1], y3 * wb[2], y3 * wb[3]};
#pragma unroll
    for (int o = 0; o < 8; ++o) { p[o] += rowRorF<8>(p[o]); p[o] += rowRorF<4>(p[o]); p[o] += rowRorF<2>(p[o]); p[o] += rowRorF<1>(p[o]); }
    pOwn = p[0];
#pragma unroll
    for (int o = 1; o < 8; ++o) pOwn = (en & 7) == o ? p[o] : pOwn;
    if (HT > 1 && rowValid && en < 8) {      // same kind of store as y3 / f'(x2)
      float* po = a.Opart + ((size_t)panel * HT + n) * 128 + em * 8 + en;
      if (a.xcdSafe) __hip_atomic_store(po, pOwn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else *po = pOwn;
    }
  }
  FSTAMP(4);
  if (!SPLITW) headPrecompute();
  // ---- group barrier: all HT tiles of this panel are in memory ------------------------------------------
  FSTAMP(5);
  __builtin_amdgcn_s_waitcnt(0);          // vmcnt(0): the stores are acknowledged by the L2
  __syncthreads();
  FVARIANT_STOP(3);
  FSTAMP(6);
  // (safe mode: the agent-scope stores above are write-through and acknowledged -- vmcnt(0) -- before the arrival below; the
  // agent-scope loads behind the barrier bypass this XCD's L2: no cache-wide release / acquire, which costs ~20 us each here)
  // (one L2 round trip: the target comes from the early read `ctr0`, the arrival returns nothing, polling starts at once; the
  // counter wraps soundly: HT is a power of two and the comparison is a signed difference)
  if (HT > 1 && tid == 0) __hip_atomic_fetch_add(a.panelCtr + panel * 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // h1 is dead (own tile kept in registers; chained form: it never was there): R1 takes the W1 row tile of the dX contraction while the peers arrive
  float* sF2 = sR3; float* sBx = sY1;
#pragma unroll
  for (int q = 0; q < QP; ++q) {
    const int f = tid + NT * q;
    if (f < 16 * H4) {
      const int r = f / H4, c = 4 * (f % H4);
      float2* d = reinterpret_cast<float2*>(sBx + r * FLDR + c);
      d[0] = make_float2(w1r[q][0], w1r[q][1]); d[1] = make_float2(w1r[q][2], w1r[q][3]);
    }
  }
  if (CHAIN && FUSED_PRE_LATE) { headPrecompute(); FSTAMP(17); }      // (the gathers are in: vmcnt(0) above)
  if (HT > 1 && tid == 0) {
    unsigned* ctr = a.panelCtr + panel * 32;
    const unsigned barTarget = (ctr0 / (unsigned)HT + 1u) * (unsigned)HT;
    int spins = 0;
    while ((int)(__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - barTarget) < 0) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > (1 << 22)) { a.sc->errFlag = 77; break; }   // never hang the GPU on a lost workgroup
    }
  }
  // beta of this step may still be on its way (POST_DEFER: the count it hangs off is taken by the rider in block 1 while the
  // panels run): one look now, so that the load's latency is hidden behind the loads of the partial outputs; the wait proper sits
  // in front of the head
  if (a.deferBeta && tid == 0) {
    double got = 0; double ok = 0;
    if (__hip_atomic_load(&a.sc->betaSeq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == betaWant) {
      got = __hip_atomic_load(&a.sc->beta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); ok = 1;
    }
    sBeta[0] = got; sBeta[1] = ok;
  }
  __syncthreads();

  FSTAMP(7);
  FVARIANT_STOP(4);
  // ---- the HT partials of O[em][en]: one round trip of HT small loads per element thread (lanes en >= 8 repeat the addresses of
  // en - 8: no guard, no extra lines) ----------------------------------------------------------------------------------------
  float pv[HT];
  if constexpr (HT > 1) {
#pragma unroll
    for (int t = 0; t < HT; ++t) pv[t] = 0.f;
    if (wave < 4) {
      const float* pp = a.Opart + (size_t)panel * HT * 128 + em * 8 + (en & 7);
      if (a.xcdSafe) {
#pragma unroll
        for (int t = 0; t < HT; ++t) pv[t] = __hip_atomic_load(pp + t * 128, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
#pragma unroll
        for (int t = 0; t < HT; ++t) pv[t] = pp[t * 128];
      }
    }
  } else pv[0] = pOwn;      // no peers: the one partial never leaves its registers
  // ---- f'(x2) of the panel is needed by the dX contraction only: loaded behind the partials and staged by the waves that have
  // no part in the head (waves 4-7 of 8; with 4 waves, by all of them after the head) ------------------------------------------
  constexpr int SNT = NW == 8 ? 256 : NT;           // staging threads
  constexpr int QF = (16 * H4 + SNT - 1) / SNT;     // float4 per staging thread of a 16 x H panel
  const int stid = NW == 8 ? tid - 256 : tid;
  f32x4 fv[QF];
#pragma unroll
  for (int q = 0; q < QF; ++q) fv[q] = z4;
  if (stid >= 0) {
    if (a.xcdSafe) {
#pragma unroll
      for (int q = 0; q < QF; ++q) {
        const int f = stid + SNT * q, r = f / H4, c4 = f % H4;
        if (f < 16 * H4 && m0 + r < nRows) {
          const float* pf = gX2 + (size_t)(m0 + r) * ldA1 + 4 * c4;
#pragma unroll
          for (int u = 0; u < 4; ++u) fv[q][u] = __hip_atomic_load(pf + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < QF; ++q) {
        const int f = stid + SNT * q, r = f / H4, c4 = f % H4;
        if (f < 16 * H4 && m0 + r < nRows) fv[q] = *reinterpret_cast<const f32x4*>(gX2 + (size_t)(m0 + r) * ldA1 + 4 * c4);
      }
    }
  }
  auto stageF2 = [&]() {
#pragma unroll
    for (int q = 0; q < QF; ++q) {
      const int f = stid + SNT * q;
      if (f < 16 * H4) {
        const int r = f / H4, c = 4 * (f % H4);
        float2* df = reinterpret_cast<float2*>(sF2 + r * FLDR + c);
        df[0] = make_float2(fv[q][0], fv[q][1]); df[1] = make_float2(fv[q][2], fv[q][3]);
      }
    }
  };
  if (a.deferBeta) {
    if (sBeta[1] == 0) {      // (the same value in every thread: written before the barrier above, not after it)
      if (tid == 0) {
        int spins = 0;
        while (__hip_atomic_load(&a.sc->betaSeq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != betaWant) {
          __builtin_amdgcn_s_sleep(1);
          if (++spins > (1 << 22)) { a.sc->errFlag = 79; break; }
        }
        sBeta[0] = __hip_atomic_load(&a.sc->beta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
    }
    beta = sBeta[0];
  }
#ifdef HL_TAIL_STAMPS
  if (tid == 0 && blockIdx.x == 8 + 8) { a.sc->dbgT[13] = wall_clock64(); a.sc->dbgT[3] = sBeta[1] != 0 ? 1 : 0; }      // beta in hand; was it there at the first look
#endif
  FSTAMP(8);
  FVARIANT_STOP(5);
  if (NW == 8 && stid >= 0) stageF2();      // (waves 4-7, while waves 0-3 run the head; the barrier that closes the head covers it)
  // network outputs of sample em stay in registers: lane en holds O[em][en] (dense part); the
  // ParamLayer part (Linear) is its bias
  const float Oen = eth ? ((rowValid && en < 8) ? treeSum<HT>(pv) : 0.f) + sBo[en] : 0.f;
#if defined(HL_FSTAMPS)
  asm volatile("" :: "v"(Oen));
#endif
  FSTAMP(9);
  const double O0 = (double)bcast0F(Oen, en);
  const double mean = (double)rowRorF<15>(Oen);                           // O[em][1 + en]: lane i reads lane i+1

  // ---- V-RACER head: thread = (sample em, action component en), fp64 --------------------------------------
  FVARIANT_STOP(6);
  // every workgroup of the group holds the head results of all 16 samples: workgroup n publishes
  // the samples em with em % HT == n, so no single workgroup carries all the stores
  const bool writer = ((em & (HT - 1)) == n);
  if (eth) {
    float g0f = 0.f, gMf = 0.f;
    if (rowValid && isNext) {     // RACER_train.cpp:23-27: V(s_{t+1}) of a truncated episode end
      const float oV = rowRorF<10>(misc), oA = rowRorF<9>(misc);      // lane 0 reads lanes 6 and 7
      if (writer && en == 0) {
        const float Vn = (float)scaleNet2V(O0);
        a.bt.oldNextV[bSrc] = oV; a.bt.oldNextADV[bSrc] = oA;
        a.rp.V[slot + 1] = Vn; a.rp.ADV[slot + 1] = 0.f; a.bt.nextV[bSrc] = Vn;
        a.bt.O[(size_t)row * a.nOut] = O0;
      }
    }
    double lw = 0, kl = 0;
    if (live && en < dA) {
      // log pi(a) - log mu(a) and D_KL(pi || mu) share one logarithm (see head.hip)
      const double m = bnd ? (mean > MAXM ? MAXM : (mean < -MAXM ? -MAXM : mean)) : mean;
      const double u1 = (act - m) * invStd;
      lw = (u2 * u2 - u1 * u1) / 2 - lq;
      const double dm = (mean - bMean) * bInv;
      kl = (CmuCpi - 1 + dm * dm - 2 * lq) / 2;
    }
    const double logW = sum16(lw), DKL = sum16(kl);
    const double RHO = exp(logW > 7 ? 7 : (logW < -7 ? -7 : logW));
    const float Wf = (float)RHO, Cf = (float)Cmax, iCf = (float)Cinv;
    const bool far = (Cf > 1.f) && (Wf > Cf || Wf < iCf);          // Episode.h:28-33 (Fval)
    const double V = scaleNet2V(O0);
    const double Qret = (double)bcast0F(misc, en);
    const double A_RET = Qret - V, dQ = A_RET;                       // Zero_advantage
    const double Ver = fmin(1.0, RHO) * dQ;
    const double g0 = far ? 0.0 : Ver * beta * scaleVdiff(O0);
    const double coef = A_RET * fmin(Cmax, RHO);
    if (live && en < dA) {
      const double dMean = mean - bMean;
      const double penalM = -1 * (dMean * invVarMu);
      const double penalS = dPos * -1 * ((invVarMu - invStd * invStd) * stdev);
      double polM = 0, polS = 0;
      if (!far) {
        if (bnd) {
          const double dLogPdMean = (act - mean) * invStd * invStd;
          const double m = mean > MAXM ? MAXM : (mean < -MAXM ? -MAXM : mean);
          const double u = (act - m) * invStd;
          polS = dPos * coef * ((u * u - 1) * invStd);
          if (mean >= MAXM && coef * dLogPdMean > 0) polM = 0;
          else if (mean <= -MAXM && coef * dLogPdMean < 0) polM = 0;
          else polM = coef * dLogPdMean;
        } else {
          const double u = (act - mean) * invStd;
          polM = coef * (u * invStd);
          polS = dPos * coef * ((u * u - 1) * invStd);
        }
      }
      const double gM = beta * polM + (1 - beta) * penalM;
      const double gS = beta * polS + (1 - beta) * penalS;
      gMf = (float)gM;                                             // Activation::addOutputDelta: nnReal += Real
      if (writer) {
        a.bt.gParam[(size_t)bSrc * dA + en] = (float)gS;
        a.bt.G[(size_t)bSrc * a.nOut + 1 + en] = (double)gMf;
        a.bt.G[(size_t)bSrc * a.nOut + nDense + en] = (double)(float)gS;
      }
    }
    if (live) g0f = (float)g0;
    // output-layer deltas of the panel (zero for next / padding rows)
    const float gPrev = rowRorF<1>(gMf);                               // component en-1 of the same sample
    if (en < 8) sDo[em * 8 + en] = en == 0 ? g0f : (en <= dA ? gPrev : 0.f);
    if (live && writer) {
      // lane 0 (the one that stores them) reads lanes 1..5
      const float oDQ = rowRorF<15>(misc), oDKL = rowRorF<14>(misc), oW = rowRorF<13>(misc);
      const float oV = rowRorF<12>(misc), oADV = rowRorF<11>(misc);
      if (en == 0) {
        a.bt.pEid[bSrc] = a.bt.eid[bSrc]; a.bt.pNextOf[bSrc] = a.bt.nextOf[bSrc];
        a.bt.G[(size_t)bSrc * a.nOut] = (double)g0f;
        a.bt.rho[bSrc] = RHO; a.bt.dkl[bSrc] = DKL; a.bt.far[bSrc] = far ? 1 : 0;
        // write-backs (Fval casts, MiniBatch.h:161-175); old values kept for the aggregate updates
        const float E = (float)dQ, D = (float)DKL, Wn = (float)RHO, Vf = (float)V;
        a.bt.oldDQ[bSrc] = oDQ; a.bt.oldDKL[bSrc] = oDKL; a.bt.oldW[bSrc] = oW; a.bt.oldV[bSrc] = oV; a.bt.oldADV[bSrc] = oADV;
        a.bt.newDQ[bSrc] = E; a.bt.newDKL[bSrc] = D; a.bt.newW[bSrc] = Wn; a.bt.newV[bSrc] = Vf;
        a.rp.DQ[slot] = E; a.rp.DKL[slot] = D; a.rp.IMPW[slot] = Wn; a.rp.V[slot] = Vf; a.rp.ADV[slot] = 0.f;
        a.bt.dq[bSrc] = (double)E;
      }
      if (en < nDense) a.bt.O[(size_t)row * a.nOut + en] = (double)Oen;
      if (en < dA) a.bt.O[(size_t)row * a.nOut + nDense + en] = (double)sBp[en];
    }
  }
  if (NW != 8) stageF2();
  __syncthreads();
  FSTAMP(10);
  FVARIANT_STOP(7);
  if (eth && writer && row < B && en < nDense) a.dOut[(size_t)row * a.ldDo + en] = sDo[em * 8 + en];

  // ---- delta_y3 = delta_out Wout^T and delta_x2 = delta_y3 f'(x2) are formed directly as the A operand
  // of the dX contraction (8 fused multiply-adds per element; no panel-wide pass, no extra barrier);
  // the element threads compute the same expression for their own element, which goes to global memory ----
  auto deltaY3 = [&](int rowL, int c) {      // sum_o delta_out[rowL][o] * Wout[c][o], fixed association
    const f32x4 wa = *reinterpret_cast<const f32x4*>(sWo + c * 8), wb = *reinterpret_cast<const f32x4*>(sWo + c * 8 + 4);
    const f32x4 da = *reinterpret_cast<const f32x4*>(sDo + rowL * 8), db = *reinterpret_cast<const f32x4*>(sDo + rowL * 8 + 4);
    float s = wa[0] * da[0];
    s = fmaf(wa[1], da[1], s); s = fmaf(wa[2], da[2], s); s = fmaf(wa[3], da[3], s);
    s = fmaf(wb[0], db[0], s); s = fmaf(wb[1], db[1], s); s = fmaf(wb[2], db[2], s); s = fmaf(wb[3], db[3], s);
    return s;
  };
  float dy3own = 0.f;
  if (eth && rowValid) {
    const int c = n0 + en;
    dy3own = deltaY3(em, c);
    if (row < B) { gDres2[(size_t)row * ldA1 + c] = dy3own; gD2[(size_t)row * ldA1 + c] = dy3own * sF2[em * FLDR + c]; }
  }
  FSTAMP(11);
  FVARIANT_STOP(8);

  // ---- own tile of delta_h1 = delta_x2 W1^T (+ residual path), delta_x1 = delta_h1 f'(x1) ----------------------
  if (wave < KWAVES) {
    const int k0 = wave * KW + lc;
    const f32x4 acc = waveMma<NK>([&](int s) { const int c = k0 + 4 * s; return deltaY3(li, c) * sF2[li * FLDR + c]; },
                                  [&](int s) { return sBx[li * FLDR + k0 + 4 * s]; });
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave * 256 + (lc * 4 + r) * 16 + li] = acc[r];
  }
  __syncthreads();
  FSTAMP(12);
  if (((em & (HT - 1)) == n) && rowValid && !isNext && en < AGG_N) a.bt.aggIn[(size_t)bSrc * AGG_N + en] = aggv;
  if (eth && row < B) {
    const float v = redSum<KWAVES>(red, tid);
    float dres = v;
    if (n0 + en < resN) dres += dy3own * sWr[n0 + en];
    a.Dres1[(size_t)row * ldA0 + n0 + en] = dres;
    float f1 = 1.f;
    dispatchFunc<CF>(func, [&](auto F) { f1 = actDiffT<decltype(F)::value>(x1o, y1o); });
    a.D1[(size_t)row * ldA0 + n0 + en] = dres * f1;
  }
  FSTAMP(13);
  FEND(m0 + 16 > a.B ? 21 : 20);
}

template <int H, int CF>
static hipError_t launchFusedT(const FusedArgs& a, int maxRows, const ExtraArgs& ex, hipStream_t s) {
  const int HT = H / 16, panels = (maxRows + 15) / 16, pg = (panels + 7) / 8;
  const size_t lds = fusedLdsBytes(a.dS, H);
  { hipError_t e = ensureDynLds(reinterpret_cast<const void*>(fused_fwd_head_dx_kernel<H, CF, FUSED_NT>), lds); if (e != hipSuccess) return e; }
  hipLaunchKernelGGL((fused_fwd_head_dx_kernel<H, CF, FUSED_NT>), dim3(8 + 8 * HT * pg), dim3(FUSED_NT), lds, s, a, ex);
  return hipGetLastError();
}
// SoftSign (the reference's default for the shipped settings) and Tanh get their own instantiation;
// every other activation takes the generic one (run-time dispatch inside the epilogues)
template <int H>
static hipError_t launchFusedH(const FusedArgs& a, int maxRows, const ExtraArgs& ex, hipStream_t s) {
  if (a.func == HL_FUNC_SOFTSIGN) return launchFusedT<H, HL_FUNC_SOFTSIGN>(a, maxRows, ex, s);
  if (a.func == HL_FUNC_TANH) return launchFusedT<H, HL_FUNC_TANH>(a, maxRows, ex, s);
  return launchFusedT<H, -1>(a, maxRows, ex, s);
}

hipError_t launch_fused(const FusedArgs& a, int maxRows, const ExtraArgs* extra, hipStream_t s) {
  ExtraArgs ex{}; if (extra) ex = *extra;
  switch (a.H) {
    case 16: return launchFusedH<16>(a, maxRows, ex, s);
    case 32: return launchFusedH<32>(a, maxRows, ex, s);
    case 64: return launchFusedH<64>(a, maxRows, ex, s);
    case 128: return launchFusedH<128>(a, maxRows, ex, s);
    case 256: return launchFusedH<256>(a, maxRows, ex, s);
    default: return hipErrorInvalidValue;
  }
}

size_t fused_lds_bytes(int dS, int H) { return fusedLdsBytes(dS, H); }
int fused_threads() { return FUSED_NT; }

// The panel exchange of the fused kernel passes y3 / f'(x2) between the workgroups of a panel with plain stores and loads,
// which is only sound while those workgroups share one XCD's L2 -- i.e. while workgroup b runs on XCD b % 8, an observed
// property of the dispatcher, not a promise of the runtime.  hl_create launches this kernel with the fused kernel's geometry
// (blocks, threads, dynamic LDS) and reads back where every workgroup ran: HW_REG_XCC_ID (hwreg 20, bits 3:0).
__global__ void xcc_probe_kernel(int* out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char probeSmem[];
  if (threadIdx.x == 0) out[blockIdx.x] = (int)(__builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 20) & 15);
}
hipError_t launch_xcc_probe(int nBlocks, int nThreads, size_t ldsBytes, int* out, hipStream_t s) {
  { hipError_t e = ensureDynLds(reinterpret_cast<const void*>(xcc_probe_kernel), ldsBytes); if (e != hipSuccess) return e; }
  hipLaunchKernelGGL(xcc_probe_kernel, dim3(nBlocks), dim3(nThreads), ldsBytes, s, out);
  return hipGetLastError();
}

}  // namespace hl
