// smarties_amd/csrc/actdev.hip -- acting and episode ingestion for rollouts that live in device memory (include/smarties_hip_dev.h).
//
//   act_head_kernel    RACER::selectAction (Learners/RACER.cpp:30-47) behind the network: policy, sampled action, state value and
//                      advantage of n agents in fp64, a thread per agent.  It restates smarties_amd/host/vracer_hip.h:209-258 operation
//                      by operation: the reference's Real is double, so floating-point contraction is OFF in this file -- every product
//                      and sum is rounded as the host code rounds it, and an action, a stored policy or a value computed here equals the
//                      host's bit for bit wherever sqrt and the division are the only functions involved (both correctly rounded on
//                      the device).  Only the Gaussian advantage goes through exp, which may differ from the host's in the last place.
//   ingest_dev_kernel  MemoryBuffer::addEpisodeToTrainingSet / pushBackEpisode (MemoryBuffer.cpp:131-170, 479-520) for a batch of
//                      episodes whose steps are rows of the caller's device arrays: ingest_kernel (misc.hip) with a strided gather in
//                      place of the pinned host block, the same insertion values for the derived fields, the reward sum formed on the
//                      device in step order.
//   policy_snapshot_kernel  hl_policy_snapshot: the parameter blob and the state standardisation copied into one of the learner's two
//                      snapshot buffers, which the acting calls read on a stream of their own while gradient steps run.
#include "dev_common.h"

#pragma clang fp contract(off)

namespace hl {

// Functions.h:541-584 (SoftPlus), Learners/RACER_common.cpp:23-27 -- restated here so that they are compiled without contraction
__device__ __forceinline__ double headSoftPlus(double x) { return (x + sqrt(1 + x * x)) / 2; }
__device__ __forceinline__ double headNet2V(double x) {
  return x > 0 ? 100 * (x + 51) - 100 * sqrt(2601 + 100 * x) : 100 * (x - 51) + 100 * sqrt(2601 - 100 * x);
}
constexpr double HEAD_CLIP = 8.31776613503286;      // SquashedNormalPolicy::sample (Continuous_policy.h:356-360)
__device__ __forceinline__ double headClip(double v) { return v > HEAD_CLIP ? HEAD_CLIP : (v < -HEAD_CLIP ? -HEAD_CLIP : v); }

// One thread per agent: the head is a few dozen dependent fp64 operations on 1 + nAdv + 2 dA numbers, nothing to share between lanes.
// No per-thread arrays (they would live in scratch): every component is recomputed from the agent's output row where it is needed twice.
__global__ __launch_bounds__(256) void act_head_kernel(ActHeadArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const double* __restrict__ o = a.O + (size_t)i * a.nOut;
  const double V = headNet2V(o[0]);
  double A = 0;
  if (a.nOpt > 0) {
    // Discrete_policy (Math/Discrete_policy.h:63-83, 190-200) + Discrete_advantage (:64-70): outputs [V | A x nOpt | logits x nOpt]
    const int nOpt = a.nOpt;
    double norm = 0;
    for (int j = 0; j < nOpt; ++j) norm += headSoftPlus(o[1 + nOpt + j]);
    norm = fmax(norm, DBL_EPSILON);
    const bool sample = a.noise != nullptr;
    const double u = sample ? a.noise[i] : 0.0;
    double* mu = a.mu + (size_t)i * nOpt;
    double cdf = 0, expA = 0, best = -1.0;
    int label = -1, arg = 0;
    for (int j = 0; j < nOpt; ++j) {
      const double p = headSoftPlus(o[1 + nOpt + j]) / norm;
      mu[j] = p;
      expA += p * o[1 + j];
      cdf += p;
      if (label < 0 && cdf > u) label = j;      // inverse CDF: the first option whose running sum exceeds u
      if (p > best) { best = p; arg = j; }       // Utilities::maxInd: the first maximum
    }
    if (!sample) label = arg;
    else if (label < 0) label = nOpt - 1;        // (u at or beyond the rounded total)
    A = o[1 + label] - expA;
    a.act[i] = (double)label + 0.1;              // label2actionMessage (StateAction.h:327-341)
  } else {
    // Continuous_policy: outputs [V | nAdv advantage terms | mean x dA | stdev pre-images x dA (ParamLayer)]
    const int dA = a.dA, nAdv = a.nAdv;
    double* act = a.act + (size_t)i * dA;
    double* mu = a.mu + (size_t)i * 2 * dA;
    double quad = 0, ratio = 1;
    for (int k = 0; k < dA; ++k) {
      const bool bounded = (a.bounded >> k) & 1ull;
      const double mean = o[1 + nAdv + k], stdev = headSoftPlus(o[a.nDense + k]);
      double x = mean;                                                    // Continuous_policy.h:779: the evaluation action
      if (a.noise) {
        const double s = mean + stdev * a.noise[(size_t)i * dA + k];     // Continuous_policy.h:192-194
        x = bounded ? headClip(s) : s;
      }
      act[k] = x; mu[k] = mean; mu[dA + k] = stdev;
      if (nAdv) {      // Gaussian_advantage::computeAdvantage (Gaus_advantage.h:76-88) with the policy's clipped mean and variance
        const double m = bounded ? headClip(mean) : mean;
        const double p1 = headSoftPlus(o[2 + k]), p2 = headSoftPlus(o[2 + dA + k]), Sv = stdev * stdev;
        quad += (x - m) * (x - m) / (x > m ? p1 : p2);
        ratio *= sqrt(p1 / (p1 + Sv)) / 2 + sqrt(p2 / (p2 + Sv)) / 2;
      }
    }
    if (nAdv) A = headSoftPlus(o[1]) * (exp(-quad / 2) - ratio);
  }
  a.V[i] = (float)V;
  a.ADV[i] = (float)((float)(V + A) - (float)V);      // MB.appendValues(V, V + A) (RACER.cpp:44-46)
}
hipError_t launch_act_head(const ActHeadArgs& a, hipStream_t s) {
  if (a.n < 1) return hipSuccess;
  hipLaunchKernelGGL(act_head_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// A thread per float of the stacked rows, workgroups striding over them: block j of agent i's row is the state max(last - j, 0) of its
// window, last = max(nSteps[i], 1) - 1 (act_stack_row of act_host.h on a strided window).  Raw values: the acting kernels standardise
__global__ __launch_bounds__(256) void act_stack_dev_kernel(ActStackDevArgs a) {
  const int dS = a.dS, dIn = dS * (1 + a.nApp);
  const long long total = (long long)a.n * dIn;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int ag = (int)(e / dIn), c = (int)(e - (long long)ag * dIn), j = c / dS, i = c - j * dS;
    const long long g = max(max(a.nSteps[ag], 1) - 1 - j, 0);
    a.rows[e] = a.states[(a.firstRow[ag] + g * a.rowStride) * dS + i];
  }
}
hipError_t launch_act_stack_dev(const ActStackDevArgs& a, hipStream_t s) {
  if (a.n < 1) return hipSuccess;
  if (!a.states || !a.firstRow || !a.nSteps || !a.rows || a.rowStride < 1 || a.dS < 1 || a.nApp < 0) return hipErrorInvalidValue;
  const long long blocks = ((long long)a.n * a.dS * (1 + a.nApp) + 255) / 256;
  hipLaunchKernelGGL(act_stack_dev_kernel, dim3((unsigned)std::min(blocks, 4096ll)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// hl_policy_snapshot: everything the acting kernels read of the learner's mutable state -- the blob, the states' means and scales -- into a
// snapshot buffer, ONE launch.  16 bytes per access, four loads in flight per thread, workgroups striding over the blob; the last workgroup
// also takes the two small arrays (whole quads as 16 bytes, the up to three values behind them one by one).  Waits for nothing in the kernel
__global__ __launch_bounds__(256) void policy_snapshot_kernel(PolicySnapshotArgs a) {
  const long long n4 = a.nW >> 2, nT = (long long)gridDim.x * 256;
  const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(a.W);
  f32x4* __restrict__ dst = reinterpret_cast<f32x4*>(a.dW);
  for (long long i0 = (long long)blockIdx.x * 256 + threadIdx.x; i0 < n4; i0 += 4 * nT) {
    f32x4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { const long long i = i0 + q * nT; v[q] = i < n4 ? src[i] : f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int q = 0; q < 4; ++q) { const long long i = i0 + q * nT; if (i < n4) dst[i] = v[q]; }
  }
  if (blockIdx.x != gridDim.x - 1) return;
  const int dS = a.dS, q4 = dS >> 2;
  for (int i = threadIdx.x; i < 2 * q4; i += 256) {
    const bool sc = i >= q4; const int k = sc ? i - q4 : i;
    reinterpret_cast<f32x4*>(sc ? a.dScale : a.dMean)[k] = reinterpret_cast<const f32x4*>(sc ? a.stScale : a.stMean)[k];
  }
  for (int i = 4 * q4 + (int)threadIdx.x; i < dS; i += 256) { a.dMean[i] = a.stMean[i]; a.dScale[i] = a.stScale[i]; }
}
hipError_t launch_policy_snapshot(const PolicySnapshotArgs& a, hipStream_t s) {
  if (!a.W || !a.stMean || !a.stScale || !a.dW || !a.dMean || !a.dScale || a.nW < 0 || (a.nW & 3) || a.dS < 1) return hipErrorInvalidValue;
  for (const void* p : {(const void*)a.W, (const void*)a.stMean, (const void*)a.stScale, (const void*)a.dW, (const void*)a.dMean, (const void*)a.dScale})
    if (reinterpret_cast<uintptr_t>(p) & 15) return hipErrorInvalidValue;
  const long long blocks = ((a.nW >> 2) + 1023) / 1024;      // four quads per thread and pass
  hipLaunchKernelGGL(policy_snapshot_kernel, dim3((unsigned)std::max(1ll, std::min(blocks, 1024ll))), dim3(256), 0, s, a);
  return hipGetLastError();
}

// blockIdx.y = episode of the launch, blockIdx.x strides over its elements (as ingest_kernel).  Workgroup x = 0 of an episode also forms
// its reward sum: the rewards pass through LDS 256 at a time and ONE thread adds them in step order, so the sum is the host route's
// `for (t = 1; t < N; ++t) totR += rewards[t]` bit for bit (and, where the episode log wants it, the log's Fval += Real beside it).
__global__ __launch_bounds__(256) void ingest_dev_kernel(IngestDevArgs a) {
  __shared__ double sR[256];
  const IngestDevDesc d = a.d[blockIdx.y];
  const int N = d.N, dS = a.dS, dA = a.dA, pD = a.polDim;
  const long long off = d.off, first = d.first, stride = a.rowStride;
  const double avgSq = a.nEpTable > 0 ? a.stats[1] : 0.0;
  const float maxError = (float)sqrt(fmax((double)FLT_EPSILON, avgSq));      // (Fval) std::sqrt(std::max(EPS, stats.avgSquaredErr))
  const int tid = blockIdx.x * 256 + threadIdx.x, nT = gridDim.x * 256;
  for (int i = tid; i < N * dS; i += nT) { const int t = i / dS, c = i - t * dS; a.rp.S[(size_t)off * dS + i] = a.S[(size_t)(first + t * stride) * dS + c]; }
  for (int i = tid; i < N * dA; i += nT) { const int t = i / dA, c = i - t * dA; a.rp.A[(size_t)off * dA + i] = a.A[(size_t)(first + t * stride) * dA + c]; }
  for (int i = tid; i < N * pD; i += nT) { const int t = i / pD, c = i - t * pD; a.rp.MU[(size_t)off * pD + i] = a.MU[(size_t)(first + t * stride) * pD + c]; }
  for (int t = tid; t < N; t += nT) {
    const size_t row = (size_t)(first + t * stride);
    a.rp.R[off + t] = a.R[row]; a.rp.V[off + t] = a.V[row]; a.rp.ADV[off + t] = a.ADV ? a.ADV[row] : 0.f;
    a.rp.RET[off + t] = 0.f; a.rp.DQ[off + t] = maxError; a.rp.IMPW[off + t] = t == N - 1 ? 0.f : 1.f; a.rp.DKL[off + t] = 0.f;
  }
  if (blockIdx.x != 0) return;
  double totR = 0; float totRf = 0.f;
  for (int t0 = 1; t0 < N; t0 += 256) {
    const int t = t0 + (int)threadIdx.x;
    if (t < N) sR[threadIdx.x] = a.R[(size_t)(first + t * stride)];
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = min(256, N - t0);
      for (int q = 0; q < m; ++q) { totR += sR[q]; totRf = (float)((double)totRf + sR[q]); }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.rp.epOff[d.eid] = off; a.rp.epN[d.eid] = N; a.rp.epTerm[d.eid] = d.term ? 1 : 0; a.rp.epTag[d.eid] = d.tag;
    float* ag = a.rp.epAgg + (size_t)d.eid * AGG_N;
    for (int q = 0; q < AGG_N; ++q) ag[q] = 0.f;
    ag[AGG_TOTR] = (float)totR; ag[AGG_AVGSQERR] = maxError * maxError; ag[AGG_MAXABSERR] = maxError; ag[AGG_MAXQ] = -1e9f; ag[AGG_MINQ] = 1e9f;
    if (a.sums) { a.sums[2 * blockIdx.y] = totR; a.sums[2 * blockIdx.y + 1] = (double)totRf; }
  }
}
hipError_t launch_ingest_dev(const IngestDevArgs& a, hipStream_t s) {
  if (a.nEp <= 0) return hipSuccess;
  if (a.nEp > INGEST_DEV_MAX_EP) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ingest_dev_kernel, dim3(8, a.nEp), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace hl
