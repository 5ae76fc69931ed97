// smarties_amd/csrc/rec_dev.h -- device helpers shared by the recurrent kernels (rec.hip: a workgroup or wavefront per sample;
// rectm.hip: a launch per (layer, window step) over the whole minibatch)
#pragma once
#include "dev_common.h"

namespace hl {

__device__ __forceinline__ float recSigm(float in) {     // Sigm::_eval (Functions.h:158-165), safeExp cut at 8 (Definitions.h:43)
  // (one exponential for both branches of the reference: the argument is -|in| cut at -8 either way)
  const float ex = expf(fmaxf(-8.f, -fabsf(in)));
  return in > 0.f ? 1.f / (1.f + ex) : ex / (1.f + ex);
}

// Element e of the network input at step k of sample b's window (general form; T = steps in front of the sampled one, t its index
// in the episode):
//   Xin != nullptr   rows written by launches in front of this one (a convolutional stack): row b K + k, the next state's row behind
//                    the B K window rows (row B K + nextRow - B)
//   acting           the agent's last states, oldest first, `actCtx` of them in front of the window (they only feed appended
//                    observations); steps before the first given one repeat it
//   otherwise        Episode::standardizedState (Episode.h:172-183): the state of the step followed by the nApp ones before it,
//                    steps before the episode's first repeat the first
__device__ __forceinline__ float recInputAt(const RecArgs& a, bool acting, int b, long long slot, int t, int T, int nextRow, int k, int e) {
  if (a.Xin) { const long long row = k <= T ? (long long)b * a.K + k : (long long)a.B * a.K + (nextRow - a.B); return a.Xin[row * a.ldXin + e]; }
  const int j = e / a.dS, i = e - j * a.dS;
  float raw;
  if (acting) { const int g = a.actCtx + k - j; raw = a.actStates[(size_t)(g > 0 ? g : 0) * a.dS + i]; }
  else { const int tt = t - T + k, back = j < tt ? j : tt; raw = a.rp.S[(size_t)(slot - T + k - back) * a.dS + i]; }
  return (raw - a.rp.stMean[i]) * a.rp.stScale[i];
}
// its acting form for one of many agents: `states` = the agent's own states, oldest first, `ctx` of them in front of its window
__device__ __forceinline__ float recActInputAt(const RecArgs& a, const float* states, int ctx, int k, int e) {
  const int j = e / a.dS, i = e - j * a.dS, g = ctx + k - j;
  return (states[(size_t)(g > 0 ? g : 0) * a.dS + i] - a.rp.stMean[i]) * a.rp.stScale[i];
}
// The acting window of workgroup b of the per-sample kernels (rec.hip): the one agent's of the arguments (actSteps states behind actCtx
// context states) or -- MANY, the kernels' form for the per-agent tables -- agent b's own: the last nBPTT + 1 of its actCnt[b] states,
// those in front as context.  win() = its window steps; states() = its first given state.  MANY is a flag of the kernel, not a test of
// the tables at run time, and without it the accessors are the arguments' fields read where they are used: the training form stays the
// code it was, register for register.
template <bool MANY>
struct RecActWin {
  const float* st; int w, c;
  __device__ __forceinline__ RecActWin(const RecArgs& a, int b) : st(nullptr), w(0), c(0) {
    if constexpr (MANY) { const int steps = a.actCnt[b]; w = min(steps, a.nBPTT + 1); c = steps - w; st = a.actStates + (size_t)a.actOff[b] * a.dS; }
  }
  __device__ __forceinline__ const float* states(const RecArgs& a) const { if constexpr (MANY) return st; else return a.actStates; }
  __device__ __forceinline__ int win(const RecArgs& a) const { if constexpr (MANY) return w; else return a.actSteps; }
};
// element e of the first layer's input at step k: recInputAt or, MANY, its form for agent b's own window `aw`
template <bool MANY>
__device__ __forceinline__ float recInputAtWin(const RecArgs& a, bool acting, const RecActWin<MANY>& aw, int b, long long slot, int t, int T, int nextRow, int k, int e) {
  if constexpr (MANY) { if (a.Xin == nullptr) return recActInputAt(a, aw.st, aw.c, k, e); }
  return recInputAt(a, acting, b, slot, t, T, nextRow, k, e);
}

}  // namespace hl
