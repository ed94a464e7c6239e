// The categorical (C51) pieces of dist_mlp.hip and rainbow_mlp.hip, stated ONCE: the atoms, the projection of
// CategoricalDQN_agent.py:72-78 and the softmax with its expectation over one wave (lane j = atom j).  dist_mlp's update keeps its
// thread-per-(action, row) softmax: another algorithm, other bits.
#pragma once
#include "common.h"
#include <math.h>

namespace {

constexpr int kMaxAtoms = 51;    // atoms / quantiles per action (one lane each in the acting kernels: at most 64)
static_assert(kMaxAtoms <= kWave, "every atom of an action has one lane of a wave");

// z = np.linspace(v_min, v_max, n) narrowed to float32 (what tensor(config.atoms) uploads): arange * step + start in fp64, the
// last one v_max itself
__device__ __forceinline__ float atom_value(double v_min, double v_max, int n, int i) {
  if (i == n - 1) return (float)v_max;
  const double step = (v_max - v_min) / (double)(n - 1);
  return (float)((double)i * step + v_min);
}

// element i of a row's projected target: sum_j clamp(1 - |clamp(rew + gm z_j) - z_i| / delta, 0, 1) p_j, p of row stride ldp
__device__ __forceinline__ float c51_project(const float* sZ, const float* p, int ldp, int N, float zi, float rew, float gm, float v_min,
                                             float v_max, float delta) {
  float t = 0.f;
  for (int j = 0; j < N; ++j) {
    float tz = __fadd_rn(rew, __fmul_rn(gm, sZ[j]));
    tz = fminf(fmaxf(tz, v_min), v_max);
    const float w = fminf(fmaxf(1.f - fabsf(tz - zi) / delta, 0.f), 1.f);
    t = fmaf(w, p[j * ldp], t);
  }
  return t;
}

// over one wave: p = softmax of the live lanes' logits l (this lane's; a dead lane's is not read), the return value sum_j p_j z_j
// with this lane's atom at *z (read on a live lane alone)
__device__ __forceinline__ float wave_softmax_value(float l, bool live, const float* z, float& p) {
  const float m = wave_max(live ? l : -INFINITY);
  const float e = live ? expf(l - m) : 0.f;
  const float s = wave_sum(e);
  p = e / s;
  return wave_sum(live ? p * *z : 0.f);
}

}  // namespace
