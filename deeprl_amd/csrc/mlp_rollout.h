// What the one-workgroup rollout kernels over small MLPs share (a2c_mlp.hip, cat_mlp.hip, q_mlp.hip, oc_mlp.hip): gate codes, row
// rounding, one hidden layer over TRANSPOSED activations and the launch; ppo_mlp.hip and dpg_mlp.hip take the vector type, the gate
// codes and softplus_f.  The cart-pole kernels (cat_mlp.hip, q_mlp.hip, oc_mlp.hip, dqn_mlp.hip, dist_mlp.hip) share more in
// cartpole_rollout.h: the environment lanes (load, observe, step with the episode-ring append, store), the staging of a two-layer
// body's weights (BodyWeights<H>; with the Q head QNetWeights<H>), the shape / offset / io checks and the hidden x gate dispatch.
// Their whole-update kernels share the row-block pieces in mlp_update_block.h.  The three kernels that act into a replay ring
// (dqn_mlp.hip, dist_mlp.hip, rainbow_mlp.hip) share their acting frame in replay_act.h, the two categorical files their atoms,
// projection and one-wave softmax in c51_block.h.
//
// Shared or not is decided by the generated code and the kernel trace, not by taste: a __forceinline__ function is optimised on
// its own before it is inlined, and these kernels sit at the edge of the SGPR file (DESIGN.md 4.13 has every figure).  The bar for
// every instantiation of every kernel, against the text in place: scratch 0, no VGPR spills, occupancy not below, VGPRs not above,
// SGPR spills not above.  Shared at that bar:
//   the cart-pole rollout pieces above;
//   gate_back / block_layer / gather_states / block_head at row blocks 16 and 64 (H 32 / 64 equal; at H 16 x 64 rows a thread now
//     carries 4 rows and no thread idles: q_mlp_update_kernel 65 / 71 -> 62 / 60 VGPRs (relu / tanh), 7 -> 8 waves; oc_mlp_update_kernel
//     86 / 88 -> 66 / 68, 5 -> 7; dqn_mlp_update_kernel 69 / 96 -> 64 / 70, 7 / 5 -> 8 / 7);
//   UpdateBody<H> (the online body's LDS layout and staging) in q_mlp_update_kernel and oc_mlp_update_kernel;
//   replay_act.h's ReplayActor (begin / observe / step / finish), ActScratch<H> and episode_row in the three replay acting kernels,
//     c51_block.h's atom_value / c51_project / wave_softmax_value in dist_mlp.hip and rainbow_mlp.hip: all 48 instances of the three
//     files hold the bar (profiles/replay_act_kernel_resources.txt).  35 are equal; SGPR spills fell in dqn_mlp_act_kernel<32> (5 / 7
//     -> 4 / 4), in three of dist_mlp_act_kernel's twelve (27 -> 25 at H 16 / 32 tanh qr, 8 -> 6 at H 64 relu c51; one VGPR less at
//     H 16 relu) and in all six of rainbow_mlp_act_kernel (160 / 164 / 145 / 149 / 161 / 165 -> 141 / 145 / 139 / 143 / 151 / 155; 153
//     -> 130 VGPRs at H 16 / 32 relu).  The form that holds it is the PLACE of begin(): behind the scratch's zeroing and ahead of the
//     weights' staging in dqn_mlp and dist_mlp, ahead of the zeroing in rainbow_mlp.  Zeroing first in rainbow_mlp_act_kernel: 149 ->
//     166 (H 32 tanh), 161 -> 174 (H 64 relu); begin() behind the atoms: 165 -> 166 (H 64 tanh); begin() first in
//     dqn_mlp_act_kernel: 4 / 4 / 5 / 7 / 4 / 4 -> 12 in all six; in dist_mlp_act_kernel: nine of twelve above (6 -> 12 at relu qr);
//     begin() behind the staging's barrier there: 9 -> 23 (H 64 tanh qr).  The members' order, the order inside begin() and the
//     softmax in place or shared moved nothing.
//   dqn_mlp_act_kernel's whole body (dqn_mlp_act_body) under the single kernel and the seed lanes' dqn_mlp_act_lanes_kernel: all six
//     single instances keep the parent's figures (profiles/dqn_lanes_kernel_resources.txt);
//   dist_mlp_act_kernel's whole body (dist_mlp_act_body) under the single kernel and dist_mlp_act_lanes_kernel, and
//     dist_mlp_update_kernel's LANES flag (dqn_mlp_update_kernel's form, tried first): all 36 instances of dist_mlp.hip keep the
//     parent's figures (profiles/dist_lanes_kernel_resources.txt).  The lane plumbing of both files is seed_lanes.h.
// NOT shared, each written in place in the four update kernels:
//   dqn_mlp_update_kernel's whole body under a lane kernel of its own: hoisted, <16, tanh> went 70 -> 78 VGPRs (71 -> 80 over the
//     window's io), the other ten equal.  The lane form is a template flag on the kernel itself (LANES; false: the parent's text,
//     arguments and figures);
//   the body's gradient bookkeeping (owner indices, dW2 / db2 / dW1 / db1 accumulators, their stores).  As one struct with the
//     same loop text it met the register bar everywhere but in dist_mlp_update_kernel's stores (H 16: 115 / 103 / 115 / 105 -> 117 /
//     104 / 117 / 109 VGPRs), yet its row loops come out with the `k2 == 0` / `j1 == 0` sums as selects and one more branch, and
//     the agents were SLOWER by more than the parent's spread (tools/bench_agents.py, medians of 3 alternating repeats, k
//     env-steps/s, parent -> struct: option_critic_feature 235.5 -> 234.8; then, with oc_mlp in place again, n_step_dqn_feature
//     282.5 -> 281.9 and quantile_regression_dqn_feature 45.39 -> 45.06);
//   dqn_mlp_update_kernel's and dist_mlp_update_kernel's staging of TWO networks' bodies: through a form of UpdateBody that also
//     holds the target's set (with or without the fill loops), dqn_mlp_update_kernel<64> goes 92 / 118 -> 96 / 122 VGPRs and
//     dist_mlp_update_kernel's SGPR spills at H 16 go 20 / 2 / 20 -> 25 / 31 / 32 (relu c51 / relu qr / tanh c51);
//   an update's staging through the rollout's BodyWeights<H> (q_mlp_update_kernel<16, tanh> went 71 -> 78 VGPRs, 7 -> 6 waves);
//   block_layer folded into hidden_layer (q_mlp_update_kernel<16, tanh> went 71 -> 77 VGPRs, 7 -> 6 waves);
//   the heads' dot products and gradients: each kernel has its own outputs per thread.
// What moved such figures in these kernels and is worth knowing before the next attempt: the order of a struct's members (it is
// the order of the values the register allocator sees), and an LDS pointer derived from a size_t count instead of continuing the
// chain of int offsets (q_mlp_update_kernel<32, tanh> 95 -> 106 VGPRs, 5 -> 4 waves).
#pragma once
#include "common.h"
#include <math.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kRB = 8;                        // rows a thread carries through one pass over k
constexpr int kGateRelu = 1, kGateTanh = 2;   // ops.ACT

__host__ __device__ constexpr int round_up8(int n) { return (n + 7) & ~7; }
__host__ __device__ constexpr int round_up4(int n) { return (n + 3) & ~3; }

// F.softplus (beta 1, threshold 20)
__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }

template <int GATE>
__device__ __forceinline__ float gate_f(float x) {
  if constexpr (GATE == kGateRelu) return fmaxf(x, 0.f);
  else return tanhf(x);
}

// one hidden layer of ONE network for the rows this thread carries: out^T[u][e] = gate(b[u] + sum_k in^T[k][e] W^T[k][u]).
// THREADS threads work on the layer, t is this one's index among them: unit u = t % H, row-block group rg = t / H; row blocks of
// kRB rows go round the THREADS / H groups.
template <int H, int GATE, int THREADS>
__device__ __forceinline__ void hidden_layer(const float* __restrict__ inT, const float* __restrict__ wT, const float* __restrict__ b,
                                             float* __restrict__ outT, int K, int NP, int t) {
  constexpr int G = THREADS / H;
  const int u = t & (H - 1), rg = t / H;
  const float bias = b[u];
  for (int e0 = rg * kRB; e0 < NP; e0 += G * kRB) {
    float acc[kRB];
#pragma unroll
    for (int r = 0; r < kRB; ++r) acc[r] = 0.f;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      const float w = wT[k * H + u];
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(&inT[k * NP + e0]);
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(&inT[k * NP + e0 + 4]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[r] = fmaf(x0[r], w, acc[r]);
        acc[4 + r] = fmaf(x1[r], w, acc[4 + r]);
      }
    }
    f32x4 y0, y1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      y0[r] = gate_f<GATE>(acc[r] + bias);
      y1[r] = gate_f<GATE>(acc[4 + r] + bias);
    }
    *reinterpret_cast<f32x4*>(&outT[u * NP + e0]) = y0;
    *reinterpret_cast<f32x4*>(&outT[u * NP + e0 + 4]) = y1;
  }
}

// KERNEL(net, io) as one workgroup of 256 threads with `bytes` of dynamic LDS
template <auto KERNEL, typename Net, typename Io>
int launch_one_workgroup(size_t bytes, const Net* net, const Io* io, void* stream) {
  static DraLdsAttr lds_attr;
  if (int rc = dra_grant_lds(lds_attr, reinterpret_cast<const void*>(KERNEL), bytes)) return rc;
  hipLaunchKernelGGL(KERNEL, dim3(1), dim3(256), bytes, dra_stream(stream), *net, *io);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}

}  // namespace
