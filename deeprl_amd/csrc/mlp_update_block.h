// The row-block pieces of a one-workgroup whole-update kernel over a two-layer cart-pole MLP, templated on the row block UB
// (dist_mlp.hip: UB 16).  q_mlp.hip and dqn_mlp.hip carry the same four functions with a fixed block of 64 rows, written in
// place; they are left as they are (their code objects and figures stay put) and move here in a change of their own (DESIGN.md
// 4.16).  Row stride of every transposed activation: UB + 4 floats (16-byte aligned rows, consecutive units 4 banks apart).
#pragma once
#include "cartpole_rollout.h"

namespace {

template <int GATE>
__device__ __forceinline__ float gate_back(float g, float h) {       // g * gate'(pre-activation), from the stored post-activation h
  if constexpr (GATE == kGateRelu) return h > 0.f ? g : 0.f;
  else return g * (1.f - h * h);
}

// rows one thread carries through a pass over k: the whole block spread over the 256 / H thread groups, at most kRB
template <int H, int UB>
struct BlockRows {
  static constexpr int raw = UB * H / 256;
  static constexpr int value = raw < 1 ? 1 : (raw > kRB ? kRB : raw);
};

// one layer over a block of UB rows.  BACK false: out = gate(b + in W); BACK true (b unused): out = (in W) * gate'(post), post^T
// the stored post-activations.  Unit u = tid % H, rows e0 .. e0 + RPT of group tid / H; every dot product one FMA chain in
// ascending k.
template <int H, int GATE, bool BACK, int UB>
__device__ __forceinline__ void block_layer(const float* __restrict__ inT, const float* __restrict__ wT, const float* __restrict__ b,
                                            const float* __restrict__ postT, float* __restrict__ outT, int K, int tid) {
  constexpr int LD = UB + 4, G = 256 / H, RPT = BlockRows<H, UB>::value;
  const int u = tid & (H - 1), rg = tid / H;
  const float bias = BACK ? 0.f : b[u];
  for (int e0 = rg * RPT; e0 < UB; e0 += G * RPT) {
    float acc[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) acc[r] = 0.f;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      const float w = wT[k * H + u];
#pragma unroll
      for (int r = 0; r < RPT; ++r) acc[r] = fmaf(inT[k * LD + e0 + r], w, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      float y;
      if constexpr (BACK) y = gate_back<GATE>(acc[r], postT[u * LD + e0 + r]);
      else y = gate_f<GATE>(acc[r] + bias);
      outT[u * LD + e0 + r] = y;
    }
  }
}

// x^T of a block from the ring's fp64 frames at sIdx[row] + shift (UB x 4 threads), zero behind the last row
template <int UB>
__device__ __forceinline__ void gather_states(const double* __restrict__ frames, const int* __restrict__ sIdx, int shift, int rows,
                                              float* __restrict__ sXT, int tid) {
  constexpr int LD = UB + 4;
  if (tid < UB * kS) {
    const int row = tid / kS, j = tid % kS;
    sXT[j * LD + row] = row < rows ? (float)frames[((int64_t)sIdx[row] + shift) * kS + j] : 0.f;
  }
}

// a head of n_out outputs over one block from h2^T: out[c * ldo + r] = b[c] + sum_k h2^T[k][r] w[c][k], outputs go round the threads
template <int H, int UB>
__device__ __forceinline__ void block_head(const float* __restrict__ sH2T, const float* __restrict__ w, const float* __restrict__ b,
                                           float* __restrict__ out, int n_out, int ldo, int tid) {
  constexpr int LD = UB + 4;
  for (int o = tid; o < n_out * UB; o += 256) {
    const int c = o / UB, r = o % UB;
    const float* wr = w + c * H;
    float acc = 0.f;
#pragma unroll 8
    for (int k = 0; k < H; ++k) acc = fmaf(sH2T[k * LD + r], wr[k], acc);
    out[c * ldo + r] = acc + b[c];
  }
}

}  // namespace
