// smarties_amd/csrc/rollout.hip -- the bookkeeping of a vectorised simulator's rollouts on the device (include/smarties_hip_rollout.h:
// hl_rollout_step).  The forward pass, the action head and the ingestion are the existing launches (learner_dev.h); the four kernels here
// keep the episodes in flight around them.
//
//   rollout_book_kernel   in front of the forward pass: every environment's state and reward into row t = len[env] of its slab, the window
//                         tables (firstRow, nSteps) the acting kernels read, and the environments whose state ended an episode compacted IN
//                         ASCENDING ENVIRONMENT ORDER into mapped pinned memory, which the host polls while the forward pass runs.
//   rollout_noise_kernel  the library's action noise: Philox4x32-10 on (seed; env, episode, step, component) -- rollout_rng.h.
//   rollout_store_kernel  behind the head: action, policy, V and advantage into row t; the terminal row of RACER::processTerminal
//                         (Learners/RACER.cpp) where the episode ended; the action out to the caller; len and the episode count.
//   rollout_stage_kernel  behind the store kernel, for a rollout with a staging ring under the snapshot source: the ended episodes out of
//                         their slabs into the ring, from where the ingestion reads them on the learner's stream.
//
// No kernel waits for another workgroup.  len is read by every workgroup of the book kernel and written by the store kernel only, so
// that the copy of the states needs no order against the bookkeeping.
#include "dev_common.h"
#include "rollout_rng.h"

#pragma clang fp contract(off)

namespace hl {

__device__ __forceinline__ int rolloutStep(const int* __restrict__ len, int e, int maxSteps) { return min(max(len[e], 0), maxSteps - 1); }

// Workgroup 0: the per-environment numbers and the compaction, walking nEnv in passes of ROLLOUT_BLOCK -- a ballot per wavefront, the
// wavefronts' counts through LDS, the running total carried in a register, so the table is in ascending environment order whatever the
// arrival order (the ingestion order decides episode ids and tags).  Workgroups 1 .. : the state rows, 16 bytes per access where `vec`
// (a launch of one workgroup does both).  Every row written lies inside its slab: t is clamped to maxSteps - 1, and an episode whose
// state count reaches maxSteps is closed here (kind 3), so len never exceeds maxSteps - 1
template <bool VEC> __global__ __launch_bounds__(ROLLOUT_BLOCK) void rollout_book_kernel(RolloutBookArgs a) {
  const int tid = threadIdx.x, nEnv = a.nEnv, maxSteps = a.maxSteps;
  if (blockIdx.x == 0) {
    __shared__ int sEnd[ROLLOUT_BLOCK / 64], sCap[ROLLOUT_BLOCK / 64];
    const int lane = tid & 63, wave = tid >> 6;
    int nEnded = 0, nCapped = 0;
    for (int e0 = 0; e0 < nEnv; e0 += ROLLOUT_BLOCK) {
      const int e = e0 + tid;
      int ns = 0, kind = 0; bool ended = false, capped = false;
      if (e < nEnv) {
        const int t = rolloutStep(a.len, e, maxSteps), flag = a.end[e];
        ns = t + 1;
        kind = flag == 1 ? 1 : (flag != 0 ? 2 : 0);
        if (kind == 0 && ns >= maxSteps) { kind = 3; capped = true; }
        a.R[(long long)e * maxSteps + t] = t == 0 ? 0.0 : a.rewards[e];
        a.firstRow[e] = (long long)e * maxSteps; a.nSteps[e] = ns; a.kind[e] = kind;
        ended = kind != 0 && ns >= 2;      // (an episode of one state holds no transition: its slab is reused, nothing is ingested)
        capped = capped && ended;
      }
      const unsigned long long bEnd = __ballot(ended), bCap = __ballot(capped);
      if (lane == 0) { sEnd[wave] = __popcll(bEnd); sCap[wave] = __popcll(bCap); }
      __syncthreads();
      int at = nEnded + __popcll(bEnd & ((1ull << lane) - 1ull));
      for (int w = 0; w < ROLLOUT_BLOCK / 64; ++w) { if (w < wave) at += sEnd[w]; nEnded += sEnd[w]; nCapped += sCap[w]; }
      if (ended) { int* q = a.host + ROLLOUT_HOST_HEAD + 3 * (long long)at; q[0] = e; q[1] = ns; q[2] = kind; }
      __syncthreads();
    }
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
      a.host[1] = nEnded; a.host[2] = nCapped;
      __hip_atomic_store(reinterpret_cast<unsigned*>(a.host), a.tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (gridDim.x > 1) return;
  }
  const long long nb = gridDim.x > 1 ? gridDim.x - 1 : 1, cb = gridDim.x > 1 ? blockIdx.x - 1 : 0;
  const int w = VEC ? a.dS >> 2 : a.dS;      // accesses per row
  const long long total = (long long)nEnv * w;
  for (long long i = cb * ROLLOUT_BLOCK + tid; i < total; i += nb * ROLLOUT_BLOCK) {
    const int e = (int)(i / w), c = (int)(i - (long long)e * w);
    const long long at = ((long long)e * maxSteps + rolloutStep(a.len, e, maxSteps)) * w + c;
    if (VEC) reinterpret_cast<f32x4*>(a.S)[at] = reinterpret_cast<const f32x4*>(a.states)[i];
    else a.S[at] = a.states[i];
  }
}
hipError_t launch_rollout_book(const RolloutBookArgs& a, hipStream_t s) {
  if (!a.states || !a.rewards || !a.end || !a.S || !a.R || !a.len || !a.firstRow || !a.nSteps || !a.kind || !a.host) return hipErrorInvalidValue;
  if (a.nEnv < 1 || a.nEnv > ROLLOUT_MAX_ENV || a.maxSteps < 2 || a.dS < 1) return hipErrorInvalidValue;
  const bool vec = a.dS % 4 == 0 && !((reinterpret_cast<uintptr_t>(a.states) | reinterpret_cast<uintptr_t>(a.S)) & 15);
  const long long total = (long long)a.nEnv * (vec ? a.dS / 4 : a.dS), copy = (total + ROLLOUT_BLOCK - 1) / ROLLOUT_BLOCK;
  const unsigned grid = copy <= 2 ? 1u : 1u + (unsigned)std::min(copy, 512ll);
  if (vec) hipLaunchKernelGGL(rollout_book_kernel<true>, dim3(grid), dim3(ROLLOUT_BLOCK), 0, s, a);
  else hipLaunchKernelGGL(rollout_book_kernel<false>, dim3(grid), dim3(ROLLOUT_BLOCK), 0, s, a);
  return hipGetLastError();
}

// a thread per (environment, component): the draw of the environment's episode count and of step t = nSteps - 1 as the book kernel left it
__global__ __launch_bounds__(256) void rollout_noise_kernel(RolloutNoiseArgs a) {
  const int per = a.discrete ? 1 : a.dA, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.nEnv * per) return;
  const int e = i / per, k = i - e * per;
  a.noise[i] = rolloutDraw(a.seed, (uint32_t)e, (uint32_t)a.episode[e], (uint32_t)(a.nSteps[e] - 1), (uint32_t)k, a.discrete != 0);
}
hipError_t launch_rollout_noise(const RolloutNoiseArgs& a, hipStream_t s) {
  if (!a.noise || !a.nSteps || !a.episode || a.nEnv < 1 || a.nEnv > ROLLOUT_MAX_ENV || a.dA < 1 || a.dA > 64) return hipErrorInvalidValue;
  const int n = a.nEnv * (a.discrete ? 1 : a.dA);
  hipLaunchKernelGGL(rollout_noise_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// a thread per environment (a few dozen bytes each).  Running: the head's row into row t, the action out.  Ended: what RACER::processTerminal
// stores -- action and policy zeros, advantage 0, V = 0 for a terminal state and the head's V of a truncated one --, zeros out
__global__ __launch_bounds__(256) void rollout_store_kernel(RolloutStoreArgs a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.nEnv) return;
  const int ns = min(max(a.nSteps[e], 1), a.maxSteps), kind = a.kind[e], dA = a.dA, pD = a.polDim;
  const long long row = (long long)e * a.maxSteps + (ns - 1);
  const bool run = kind == 0;
  for (int k = 0; k < dA; ++k) { const double v = run ? a.act[(long long)e * dA + k] : 0.0; a.A[row * dA + k] = v; a.outAct[(long long)e * dA + k] = v; }
  for (int k = 0; k < pD; ++k) a.MU[row * pD + k] = run ? a.mu[(long long)e * pD + k] : 0.0;
  a.V[row] = kind == 1 ? 0.f : a.v[e];
  a.ADV[row] = run ? a.adv[e] : 0.f;
  a.len[e] = run ? ns : 0;
  if (!run) a.episode[e] += 1;
}
hipError_t launch_rollout_store(const RolloutStoreArgs& a, hipStream_t s) {
  if (!a.act || !a.mu || !a.v || !a.adv || !a.A || !a.MU || !a.V || !a.ADV || !a.outAct || !a.len || !a.episode || !a.nSteps || !a.kind) return hipErrorInvalidValue;
  if (a.nEnv < 1 || a.nEnv > ROLLOUT_MAX_ENV || a.maxSteps < 2 || a.dA < 1 || a.polDim < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rollout_store_kernel, dim3((a.nEnv + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// Workgroups (x, y): episode y of the batch, its rows walked by the gridDim.x workgroups of its column.  An episode's rows are contiguous
// in the slab and in the ring, so each array is one flat copy of nsteps rows; the states 16 bytes per access where VEC.  Plain loads and
// stores: the kernel waits for nothing and shares no word with another workgroup
template <bool VEC> __global__ __launch_bounds__(256) void rollout_stage_kernel(RolloutStageArgs a) {
  const RolloutStageEp q = a.ep[blockIdx.y];
  const long long src = (long long)q.env * a.maxSteps, dst = q.dst, n = q.nsteps;
  const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
  const long long w = VEC ? a.dS >> 2 : a.dS, dA = a.dA, pD = a.polDim;
  for (long long i = i0; i < n * w; i += step) {
    if (VEC) reinterpret_cast<f32x4*>(a.rS)[dst * w + i] = reinterpret_cast<const f32x4*>(a.S)[src * w + i];
    else a.rS[dst * w + i] = a.S[src * w + i];
  }
  for (long long i = i0; i < n * dA; i += step) a.rA[dst * dA + i] = a.A[src * dA + i];
  for (long long i = i0; i < n * pD; i += step) a.rMU[dst * pD + i] = a.MU[src * pD + i];
  for (long long i = i0; i < n; i += step) { a.rR[dst + i] = a.R[src + i]; a.rV[dst + i] = a.V[src + i]; a.rADV[dst + i] = a.ADV[src + i]; }
}
hipError_t launch_rollout_stage(const RolloutStageArgs& a, hipStream_t s) {
  if (!a.S || !a.A || !a.MU || !a.R || !a.V || !a.ADV || !a.rS || !a.rA || !a.rMU || !a.rR || !a.rV || !a.rADV) return hipErrorInvalidValue;
  if (a.nEnv < 1 || a.nEnv > ROLLOUT_MAX_ENV || a.maxSteps < 2 || a.dS < 1 || a.dA < 1 || a.polDim < 1) return hipErrorInvalidValue;
  if (a.nEp < 1 || a.nEp > ROLLOUT_STAGE_MAX_EP || a.ringRows < 1) return hipErrorInvalidValue;
  long long most = 0;      // the widest array of the longest episode, in accesses
  const bool vec = a.dS % 4 == 0 && !((reinterpret_cast<uintptr_t>(a.S) | reinterpret_cast<uintptr_t>(a.rS)) & 15);
  for (int k = 0; k < a.nEp; ++k) {      // every row read lies in its slab, every row written in the ring
    const RolloutStageEp& q = a.ep[k];
    if (q.env < 0 || q.env >= a.nEnv || q.nsteps < 2 || q.nsteps > a.maxSteps || q.dst < 0 || q.dst + q.nsteps > a.ringRows) return hipErrorInvalidValue;
    most = std::max(most, (long long)q.nsteps * std::max<long long>(vec ? a.dS / 4 : a.dS, std::max(a.dA, a.polDim)));
  }
  const dim3 grid((unsigned)std::min((most + 255) / 256, 64ll), (unsigned)a.nEp);
  if (vec) hipLaunchKernelGGL(rollout_stage_kernel<true>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(rollout_stage_kernel<false>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace hl
