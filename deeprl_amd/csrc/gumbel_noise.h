// Rank-invariant categorical sampling, the ONE statement of its noise stream: action = argmax_a (logit_a + Gumbel noise), the
// noise a counter hash of (seed, sampler step, GLOBAL row, a).  Shared by gumbel_sample_kernel (losses.hip: one launch per
// sample, dist.DataParallel.sample) and the categorical rollout kernel (cat_mlp.hip), which must draw the same bits.
#pragma once
#include "common.h"

__device__ __forceinline__ uint64_t gs_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t gs_step_base(uint64_t seed, int64_t step) {
  return gs_mix64(seed * 0x9E3779B97F4A7C15ull + (uint64_t)step);
}
// logit + Gumbel noise of (global row, action a)
__device__ __forceinline__ float gs_perturbed(uint64_t base, int64_t row, int a, float logit) {
  const uint64_t h = gs_mix64(base + (uint64_t)row * 64ull + (uint64_t)a);
  // 23 bits: k + 0.5 is exact in fp32 for every k < 2^23, so u lies STRICTLY inside (0, 1) (with 24 bits the largest k
  // rounded up to 2^24 and u == 1 made -log(-log u) = +inf: that action won whatever the logits, 2^-24 per draw)
  const float u = ((float)(h >> 41) + 0.5f) * (1.0f / 8388608.0f);
  return logit - logf(-logf(u));
}
