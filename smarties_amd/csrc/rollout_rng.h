// smarties_amd/csrc/rollout_rng.h -- the action noise of hl_rollout_step (include/smarties_hip_rollout.h states the mapping in words): a
// counter-based generator, so that a draw is a function of (seed, environment, episode, step, component) and of nothing else.  Compiled for
// the device (rollout.hip: rollout_noise_kernel) and for the host (learner_rollout.h: hl_rollout_noise), the same text for both.
#pragma once
#include <cmath>
#include <cstdint>

namespace hl {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of two 32 x 32 -> 64
// multiplications, the key bumped by the Weyl constants between rounds.  Known answer: counter 0, key 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
struct PhiloxBlock { uint32_t x[4]; };
__host__ __device__ inline PhiloxBlock philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return PhiloxBlock{{c0, c1, c2, c3}};
}
// 53 bits of two words as a double in [0, 1): the upper 27 bits of `hi` above the upper 26 bits of `lo`
__host__ __device__ inline double rolloutU53(uint32_t hi, uint32_t lo) {
  return (double)(((uint64_t)(hi >> 5) << 26) | (uint64_t)(lo >> 6)) * (1.0 / 9007199254740992.0);
}
constexpr double ROLLOUT_NORMDIST_MAX = 3.0;      // NORMDIST_MAX (Agent::sampleClippedGaussian)
constexpr double ROLLOUT_TWO_PI = 6.283185307179586476925286766559;
// The draw of (environment, episode, step, component): key = (seed's low word, seed's high word), counter = (env, episode mod 2^32, t,
// component + 65536 b), b = 0 for the first block x and 1 for the second block y.
//   discrete head   u = U53(x0, x1)
//   continuous      z = sqrt(-2 log(1 - U53(x0, x1))) cos(2 pi U53(x2, x3));  beyond +-3:  z = (2 U53(y0, y1) - 1) 3
__host__ __device__ inline double rolloutDraw(uint64_t seed, uint32_t env, uint32_t episode, uint32_t t, uint32_t component, bool discrete) {
#pragma clang fp contract(off)      // every product and sum rounded on its own, on the device as on the host
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const PhiloxBlock x = philox4x32_10(env, episode, t, component, k0, k1);
  const double u1 = rolloutU53(x.x[0], x.x[1]);
  if (discrete) return u1;
  const double u2 = rolloutU53(x.x[2], x.x[3]);
  const double z = sqrt(-2.0 * log(1.0 - u1)) * cos(ROLLOUT_TWO_PI * u2);
  if (z <= ROLLOUT_NORMDIST_MAX && z >= -ROLLOUT_NORMDIST_MAX) return z;
  const PhiloxBlock y = philox4x32_10(env, episode, t, component + 65536u, k0, k1);
  return (2.0 * rolloutU53(y.x[0], y.x[1]) - 1.0) * ROLLOUT_NORMDIST_MAX;
}

}  // namespace hl
