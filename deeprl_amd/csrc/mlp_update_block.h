// The row-block pieces of a one-workgroup whole-update kernel over a two-layer cart-pole MLP, stated ONCE and templated on the row
// block UB (q_mlp.hip, oc_mlp.hip, dqn_mlp.hip: UB 64; dist_mlp.hip: UB 16): gate_back, block_layer, gather_states, block_head, the
// online body's LDS layout and staging (UpdateBody<H>: q_mlp.hip, oc_mlp.hip, rainbow_mlp.hip).  Heads, losses and the gradient
// bookkeeping stay in their kernels (the categorical projection and one-wave softmax of dist_mlp.hip / rainbow_mlp.hip: c51_block.h):
// what is NOT shared, with the figures that decided it, is in mlp_rollout.h's banner.
// Row stride of every transposed activation: UB + 4 floats (16-byte aligned rows, consecutive units 4 banks apart).
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
// ascending k.  Not folded into hidden_layer: mlp_rollout.h's banner.
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
    if constexpr (RPT == 8) {      // (UB 64 at H 32 / 64) hidden_layer's text: two 16-byte accesses a row of k, spelled out -- from
                                   // the per-float form below the compiler merges the loads but not every store
#pragma unroll 4
      for (int k = 0; k < K; ++k) {
        const float w = wT[k * H + u];
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(&inT[k * LD + e0]);
        const f32x4 x1 = *reinterpret_cast<const f32x4*>(&inT[k * LD + e0 + 4]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          acc[r] = fmaf(x0[r], w, acc[r]);
          acc[4 + r] = fmaf(x1[r], w, acc[4 + r]);
        }
      }
      f32x4 y0, y1;
      if constexpr (BACK) {
        const f32x4 p0 = *reinterpret_cast<const f32x4*>(&postT[u * LD + e0]);
        const f32x4 p1 = *reinterpret_cast<const f32x4*>(&postT[u * LD + e0 + 4]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          y0[r] = gate_back<GATE>(acc[r], p0[r]);
          y1[r] = gate_back<GATE>(acc[4 + r], p1[r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          y0[r] = gate_f<GATE>(acc[r] + bias);
          y1[r] = gate_f<GATE>(acc[4 + r] + bias);
        }
      }
      *reinterpret_cast<f32x4*>(&outT[u * LD + e0]) = y0;
      *reinterpret_cast<f32x4*>(&outT[u * LD + e0 + 4]) = y1;
    } else {
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

// the online network's body weights of an update in LDS, UNPADDED (the rollout's BodyWeights<H> is another layout): W1^T [S][H],
// W2^T [H][H] (transposed: [k][unit]), W2 [H][H] as stored ([unit][k]: the backward's "transposed" operand), b1, b2 at `base`, the
// kernel's own head behind them at `head`.  Every pointer continues the one before it in int arithmetic: an offset computed apart
// (lds + a size_t count) changes the form of every address behind it and cost q_mlp_update_kernel<32, tanh> a wave.
__host__ __device__ constexpr size_t update_body_floats(int H) { return (size_t)kS * H + 2 * (size_t)H * H + 2 * (size_t)H; }
template <int H>
struct UpdateBody {
  float *w1, *w2, *w2n, *b1, *b2, *head;
  __device__ explicit UpdateBody(float* base) : w1(base), w2(w1 + kS * H), w2n(w2 + H * H), b1(w2n + H * H), b2(b1 + H), head(b2 + H) {}
  template <typename Net>
  __device__ __forceinline__ void stage(const Net& net, int tid) const {
    const float* __restrict__ P = net.param;
    for (int i = tid; i < kS * H; i += 256) {
      const int k = i / H, u = i - k * H;
      w1[i] = P[net.w1 + u * kS + k];
    }
    for (int i = tid; i < H * H; i += 256) {
      const int k = i / H, u = i - k * H;
      w2[i] = P[net.w2 + u * H + k];
      w2n[i] = P[net.w2 + i];
    }
    for (int i = tid; i < H; i += 256) {
      b1[i] = P[net.b1 + i];
      b2[i] = P[net.b2 + i];
    }
  }
};

}  // namespace
