// Device-side pieces shared by the stand-alone kernels of igemm.hip and the fused rollout launches of conv_v2.hip (an A2C / PPO
// rollout step over NatureConvBody as four launches: [conv1 | policy head of the previous step], conv2, conv3, fc4).
// One statement of each piece, so that a fused launch and the separate kernels give the same bits.
#pragma once
#include "common.h"

__device__ __forceinline__ float rr_act(float v, int act) {      // DRA_ACT_*: igemm.h act_apply / conv_v2.hip v2_act
  if (act == DRA_ACT_RELU) return v > 0.f ? v : 0.f;
  if (act == DRA_ACT_TANH) return tanhf(v);
  return v;
}

// Two linear heads on the same features: the wave's work for input row b (in_features K <= 512: 8 registers per lane, k = lane +
// 64 i); the weight rows of up to eight outputs are requested together with them -- one memory round trip, no LDS, no barrier --
// then the eight dot products and their wave butterflies run interleaved.  sink(o, value) runs on lane 0 for every output o of
// [0, O0 + O1).  Per-output arithmetic (lane-strided partial sums in i order, then the butterfly) is linear_gemv_kernel's.
// load_x(k): feature k of the row (a plain row of x, or -- the update's fc4 handing its K-slice partial sums over -- their fold).
template <class XLoad, class Sink>
__device__ __forceinline__ void heads_row_outputs_from(XLoad load_x, const float* __restrict__ w0, const float* __restrict__ b0, int O0,
                                                       const float* __restrict__ w1, const float* __restrict__ b1, int O1, int K,
                                                       int act, int lane, Sink sink) {
  float xv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) xv[i] = (lane + 64 * i < K) ? load_x(lane + 64 * i) : 0.f;
  const int OT = O0 + O1;
  for (int oc = 0; oc < OT; oc += 8) {
    float wv[8][8], bias[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int o = min(oc + u, OT - 1);
      const float* __restrict__ row = o < O0 ? w0 + (int64_t)o * K : w1 + (int64_t)(o - O0) * K;
#pragma unroll
      for (int i = 0; i < 8; ++i) wv[u][i] = (lane + 64 * i < K) ? row[lane + 64 * i] : 0.f;
      const float* __restrict__ bp = o < O0 ? b0 : b1;
      bias[u] = bp ? bp[o < O0 ? o : o - O0] : 0.f;
    }
    float part[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      float p = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) p += (lane + 64 * i < K) ? xv[i] * wv[u][i] : 0.f;
      part[u] = p;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int u = 0; u < 8; ++u) part[u] += __shfl_xor(part[u], off, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int o = oc + u;
        if (o < OT) sink(o, rr_act(part[u] + bias[u], act));
      }
    }
  }
}

template <class Sink>
__device__ __forceinline__ void heads_row_outputs(const float* __restrict__ x, const float* __restrict__ w0,
                                                  const float* __restrict__ b0, int O0, const float* __restrict__ w1,
                                                  const float* __restrict__ b1, int O1, int b, int K, int act, int lane, Sink sink) {
  heads_row_outputs_from([&](int k) { return x[(int64_t)b * K + k]; }, w0, b0, O0, w1, b1, O1, K, act, lane, sink);
}

// A categorical actor-critic's whole policy head for input row b (network_heads.py:240-255): logits = x W0^T + b0 [A <= 64],
// v = x w1^T + b1, then Categorical(logits) of the row on the lane that holds the outputs -- inverse-CDF sample from uniform[b]
// (action_in == nullptr) or the given action, log_pi_a, entropy (common.h categorical_row).  so: >= A + 1 floats of LDS owned by
// the calling wave.
// KS > 0 (template argument of policy_head_row): the features are the fold of KS K-slice partial sums slabs[s][b][k] of the layer
// below (fc4's one-pass forward) + fold_bias[k], through a ReLU -- linear_finish_kernel's sum, slab 0 first -- and are written to
// out_x [B][K] for the backward pass; KS == 0: x [B][K] as is.
struct PolicyHeadArgs {
  const float *x, *w0, *b0, *w1, *b1, *uniform;
  const int64_t* action_in;
  int64_t* out_action;
  float *out_lp, *out_ent, *out_v, *out_logits;
  int B, K, A;
  const float *slabs, *fold_bias;
  float* out_x;
};
template <int KS = 0>
__device__ __forceinline__ void policy_head_row(const PolicyHeadArgs& h, int b, int lane, float* so) {
  auto sink = [&](int o, float v) { so[o] = v; };
  if constexpr (KS > 0) {
    heads_row_outputs_from([&](int k) {
      const float* sl = h.slabs + (int64_t)b * h.K + k;
      float part[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) part[s] = sl[(int64_t)s * h.B * h.K];
      float v = part[0];
#pragma unroll
      for (int s = 1; s < KS; ++s) v += part[s];
      v = rr_act(v + h.fold_bias[k], DRA_ACT_RELU);
      h.out_x[(int64_t)b * h.K + k] = v;
      return v;
    }, h.w0, h.b0, h.A, h.w1, h.b1, 1, h.K, /*act=*/0, lane, sink);
  } else {
    heads_row_outputs(h.x, h.w0, h.b0, h.A, h.w1, h.b1, 1, b, h.K, /*act=*/0, lane, sink);
  }
  if (lane == 0) {      // (the same lane wrote so[]: program order, no barrier)
    int64_t act;
    float lp, ent;
    categorical_row(so, h.A, h.action_in != nullptr, h.action_in ? h.action_in[b] : 0, h.uniform ? h.uniform[b] : 0.f, &act, &lp,
                    &ent);
    if (h.out_action) h.out_action[b] = act;
    h.out_lp[b] = lp;
    h.out_ent[b] = ent;
    h.out_v[b] = so[h.A];
    if (h.out_logits)
      for (int a = 0; a < h.A; ++a) h.out_logits[(int64_t)b * h.A + a] = so[a];
  }
}

// The same head for ONE row per WORKGROUP of four waves, the row's features folded from KS K-slice partial sums first (fc4 of a
// rollout step through the one-pass K-slice kernel with 28 slices: 4.3 us at 8-32 samples against the eight-wave GEMV's 5.6 / 8.1 /
// 13.2 us, tools/fc4_small_probe.py -- its finish happens here, and in a rollout this head rides in the NEXT step's conv1 launch,
// where the fold's loads cost nothing on the chain): thread t folds features t and t + 256 (2 KS loads in flight, slab 0 first, +
// bias, ReLU: linear_finish_kernel's sum) into LDS, then wave 0 runs the head on them.  s_phi: 512 floats, so: >= A + 1 floats.
// The fold itself (thread t < 256 of the row's workgroup: features t and t + 256 into s_phi, and out_x[b] when given) -- shared by
// the policy head below and the Q head of an n-step DQN rollout (q_head_row_fold_wg): the same features, bit for bit.  K = 512.
template <int KS>
__device__ __forceinline__ void fold_row_slabs_wg(const float* __restrict__ slabs, const float* __restrict__ fold_bias, int B, int K,
                                                  int b, float* s_phi, float* out_x) {
  const int t = threadIdx.x;
  float part[2][KS];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float* sl = slabs + (int64_t)b * K + t + 256 * j;
#pragma unroll
    for (int s = 0; s < KS; ++s) part[j][s] = sl[(int64_t)s * B * K];
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = t + 256 * j;
    float v = part[j][0];
#pragma unroll
    for (int s = 1; s < KS; ++s) v += part[j][s];
    v = rr_act(v + fold_bias[k], DRA_ACT_RELU);
    s_phi[k] = v;
    if (out_x) out_x[(int64_t)b * K + k] = v;
  }
}

template <int KS>
__device__ __forceinline__ void policy_head_row_fold_wg(const PolicyHeadArgs& h, int b, float* s_phi, float* so) {
  const int t = threadIdx.x;
  fold_row_slabs_wg<KS>(h.slabs, h.fold_bias, h.B, h.K, b, s_phi, h.out_x);
  __syncthreads();
  if (t >= 64) return;
  const int lane = t;
  heads_row_outputs_from([&](int k) { return s_phi[k]; }, h.w0, h.b0, h.A, h.w1, h.b1, 1, h.K, /*act=*/0, lane,
                         [&](int o, float v) { so[o] = v; });
  if (lane == 0) {
    int64_t act;
    float lp, ent;
    categorical_row(so, h.A, h.action_in != nullptr, h.action_in ? h.action_in[b] : 0, h.uniform ? h.uniform[b] : 0.f, &act, &lp,
                    &ent);
    if (h.out_action) h.out_action[b] = act;
    h.out_lp[b] = lp;
    h.out_ent[b] = ent;
    h.out_v[b] = so[h.A];
    if (h.out_logits)
      for (int a = 0; a < h.A; ++a) h.out_logits[(int64_t)b * h.A + a] = so[a];
  }
}

// The Q head of an n-step DQN rollout step (NStepDQN_agent.py:33-36: q = network(states)['q'], epsilon_greedy(epsilon, q)) for ONE
// row per workgroup of four waves, its features folded from fc4's KS K-slice partial sums first (fold_row_slabs_wg: the A2C head's
// fold, bit for bit): q = phi W^T + b [A <= 64] (heads_row_outputs_from), the first index of the row's maximum (np.argmax: exact
// ties go to the lower index, a NaN wins), and the behaviour action explore[b] ? random_action[b] : argmax -- both planned on the
// host in the reference's draw order, so no random draw and no compare against epsilon happens here.  Every output is optional:
// out_phi [B][512], out_q [B][A], out_action [B] (needs explore / random_action), out_max [B] = max_a q (the bootstrap of the
// target network, NStepDQN_agent.py:56-57).  s_phi: 512 floats, so: >= A floats.
struct QHeadArgs {
  const float *slabs, *fold_bias, *w, *b;
  const uint8_t* explore;
  const int64_t* random_action;
  float *out_phi, *out_q, *out_max;
  int64_t* out_action;
  int B, A;
};
template <int KS>
__device__ __forceinline__ void q_head_row_fold_wg(const QHeadArgs& h, int b, float* s_phi, float* so) {
  const int t = threadIdx.x;
  fold_row_slabs_wg<KS>(h.slabs, h.fold_bias, h.B, 512, b, s_phi, h.out_phi);
  __syncthreads();
  if (t >= 64) return;
  const int lane = t;
  heads_row_outputs_from([&](int k) { return s_phi[k]; }, h.w, h.b, h.A, nullptr, nullptr, 0, 512, /*act=*/0, lane,
                         [&](int o, float v) { so[o] = v; });
  if (lane == 0) {      // (the same lane wrote so[]: program order, no barrier)
    float best = so[0];
    int arg = 0;
    for (int a = 1; a < h.A; ++a) {
      if (best != best) break;                        // NaN: np.argmax stops at the first one
      const float v = so[a];
      if (v > best || v != v) { best = v; arg = a; }
    }
    if (h.out_q)
      for (int a = 0; a < h.A; ++a) h.out_q[(int64_t)b * h.A + a] = so[a];
    if (h.out_max) h.out_max[b] = best;
    if (h.out_action) h.out_action[b] = h.explore[b] ? h.random_action[b] : (int64_t)arg;
  }
}

// Three linear heads on the same features, their outputs spread over the NWAVES waves of a workgroup: wave `wave` runs the chunks
// of eight outputs oc = 8 wave, 8 (wave + NWAVES), ... of [0, O0 + O1 + O2) -- the sibling of heads_row_outputs_from for a head
// too wide for one wave (option-critic: 2 O + O A outputs), with that function's per-output arithmetic (lane-strided partial sums
// in i order, then the butterfly, + bias).  K = 512.  sink(o, value) runs on lane 0 of the wave that owns output o.
template <int NWAVES, class Sink>
__device__ __forceinline__ void heads3_row_outputs_lds(const float* __restrict__ x, const float* __restrict__ w0,
                                                       const float* __restrict__ b0, int O0, const float* __restrict__ w1,
                                                       const float* __restrict__ b1, int O1, const float* __restrict__ w2,
                                                       const float* __restrict__ b2, int O2, int wave, int lane, Sink sink) {
  constexpr int K = 512;
  float xv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) xv[i] = x[lane + 64 * i];
  const int OT = O0 + O1 + O2;
  for (int oc = 8 * wave; oc < OT; oc += 8 * NWAVES) {
    float wv[8][8], bias[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int o = min(oc + u, OT - 1);
      const float* __restrict__ row;
      const float* __restrict__ bp;
      int j;
      if (o < O0) { row = w0; bp = b0; j = o; }
      else if (o < O0 + O1) { row = w1; bp = b1; j = o - O0; }
      else { row = w2; bp = b2; j = o - O0 - O1; }
      row += (int64_t)j * K;
#pragma unroll
      for (int i = 0; i < 8; ++i) wv[u][i] = row[lane + 64 * i];
      bias[u] = bp ? bp[j] : 0.f;
    }
    float part[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      float p = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) p += xv[i] * wv[u][i];
      part[u] = p;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int u = 0; u < 8; ++u) part[u] += __shfl_xor(part[u], off, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int o = oc + u;
        if (o < OT) sink(o, part[u] + bias[u]);
      }
    }
  }
}

// Inverse CDF of a row of unnormalised weights p[0, n) at u, as Categorical(probs=p) sees it: the row is divided by its fp32 sum
// (index order) in place, then the first k whose running fp32 sum exceeds u wins, the last index when none does --
// categorical_row's rule (common.h).  (pi_hat of sample_option does not sum to one: beta is a vector over options.)
__device__ __forceinline__ int inv_cdf_row(float* p, int n, float u) {
  float s = 0.f;
  for (int k = 0; k < n; ++k) s += p[k];
  for (int k = 0; k < n; ++k) p[k] = p[k] / s;
  float cum = 0.f;
  for (int k = 0; k < n; ++k) {
    cum += p[k];
    if (cum > u) return k;
  }
  return n - 1;
}

// The option-critic head of a rollout step (OptionCritic_agent.py:55-63, network_heads.py:118-127) for ONE row per workgroup of
// four waves, its features folded from fc4's KS K-slice partial sums first (fold_row_slabs_wg: the A2C / n-step fold, bit for bit):
// q = phi Wq^T + bq [O], z_beta = phi Wb^T + bb [O] and the O A intra-option logits phi Wp^T + bp (row o A + a: action a of option
// o) over all four waves (heads3_row_outputs_lds), then on one lane the decisions of sample_option (OptionCritic_agent.py:29-49):
// beta = sigmoid(z_beta), g = the first index of q's maximum, pi_opt = eps / O with 1 - eps + eps / O at g, pi_hat = (1 - beta)
// 1[o == prev] + beta pi_opt, option = init ? invCDF(pi_opt, u0) : invCDF(pi_hat, u1) (each row normalised by its sum first, as
// Categorical(probs=) does: inv_cdf_row), then categorical_row on the chosen option's
// A logits with u2: action, log pi(a), entropy.  The carried state is read and replaced in place: prev_option[b] <- option,
// init[b] <- (mask[b] == 0) (the next step's is_initial_states = terminals); out_prev / out_init record what this step read.
// Bootstrap mode (out_boot != nullptr; OptionCritic_agent.py:87-93, the target network over observation T): only q and z_beta,
// out_boot[b] = (1 - beta[prev]) q[prev] + beta[prev] max q with prev = prev_option[b], the carried state untouched.
// Every per-row output is optional.  uniform [B][3] (fresh option, continued option, action); eps [1]: this step's option epsilon.
// s_phi: 512 floats; so: >= 2 O + O A floats.  O <= 8, A <= 18 (the launchers check).
struct OCHeadArgs {
  const float *slabs, *fold_bias, *wq, *bq, *wb, *bb, *wp, *bp;
  const float *uniform, *eps, *mask;
  int64_t* prev_option;
  uint8_t* init;
  float *out_phi, *out_q, *out_beta, *out_logits, *out_lp, *out_ent, *out_init, *out_boot;
  int64_t *out_option, *out_action, *out_prev;
  int B, O, A;
};
template <int KS>
__device__ __forceinline__ void oc_head_row_fold_wg(const OCHeadArgs& h, int b, float* s_phi, float* so) {
  const int t = threadIdx.x;
  fold_row_slabs_wg<KS>(h.slabs, h.fold_bias, h.B, 512, b, s_phi, h.out_phi);
  __syncthreads();
  const int O = h.O, A = h.A;
  const bool boot = h.out_boot != nullptr;
  heads3_row_outputs_lds<4>(s_phi, h.wq, h.bq, O, h.wb, h.bb, O, h.wp, h.bp, boot ? 0 : O * A, t >> 6, t & 63,
                            [&](int o, float v) { so[o] = v; });
  __syncthreads();
  if (t != 0) return;
  const float* q = so;
  const float* zb = so + O;
  float beta[8];
  for (int o = 0; o < O; ++o) beta[o] = 1.f / (1.f + expf(-zb[o]));
  float qmax = q[0];
  int g = 0;
  for (int o = 1; o < O; ++o) {
    if (qmax != qmax) break;                          // NaN: argmax stops at the first one
    if (q[o] > qmax || q[o] != q[o]) { qmax = q[o]; g = o; }
  }
  const int64_t prev_in = h.prev_option[b];
  const int prev = prev_in < 0 ? 0 : (prev_in >= O ? O - 1 : (int)prev_in);
  if (h.out_q)
    for (int o = 0; o < O; ++o) h.out_q[(int64_t)b * O + o] = q[o];
  if (h.out_beta)
    for (int o = 0; o < O; ++o) h.out_beta[(int64_t)b * O + o] = beta[o];
  if (boot) {
    h.out_boot[b] = (1.f - beta[prev]) * q[prev] + beta[prev] * qmax;
    return;
  }
  const float eps = h.eps[0];
  const float base = eps / (float)O, top = 1.f - eps + eps / (float)O;
  float pi_opt[8], pi_hat[8];
  for (int o = 0; o < O; ++o) {
    pi_opt[o] = o == g ? top : base;
    pi_hat[o] = (1.f - beta[o]) * (o == prev ? 1.f : 0.f) + beta[o] * pi_opt[o];
  }
  const float* u = h.uniform + (int64_t)b * 3;
  const bool init = h.init[b] != 0;
  const int fresh = inv_cdf_row(pi_opt, O, u[0]), continued = inv_cdf_row(pi_hat, O, u[1]);
  const int option = init ? fresh : continued;
  const float* logits = so + 2 * O + option * A;
  int64_t act;
  float lp, ent;
  categorical_row(logits, A, false, 0, u[2], &act, &lp, &ent);
  if (h.out_logits)
    for (int a = 0; a < A; ++a) h.out_logits[(int64_t)b * A + a] = logits[a];
  if (h.out_option) h.out_option[b] = option;
  if (h.out_action) h.out_action[b] = act;
  if (h.out_lp) h.out_lp[b] = lp;
  if (h.out_ent) h.out_ent[b] = ent;
  if (h.out_prev) h.out_prev[b] = prev_in;
  if (h.out_init) h.out_init[b] = init ? 1.f : 0.f;
  h.prev_option[b] = option;
  h.init[b] = h.mask[b] == 0.f ? 1 : 0;
}

// A wide linear layer at rollout batch sizes (fc4 of NatureConvBody, 3136 -> 512, for the 8 / 16 environments of one rollout
// step): a workgroup of EIGHT waves owns 8 / WPR output rows (o2 = index of the group), each row's reduction split over WPR waves
// (K parts); a lane keeps its R float4 of the weight row in registers and, per round, the matching float4 of up to RB input
// rows -- all requested before the first is used; per sample: products, a wave sum, the WPR part sums met in LDS as a fixed
// pairwise tree.  Per-sample arithmetic depends on (R, WPR) only.  K % 4 == 0, K <= 4 * 64 * WPR * R.
//   <4, 8, 4>: two rows per workgroup, eight samples per round (<= 8 samples: one round; 16 samples were two dependent rounds,
//              9.4 us against 6.3: profiles/r05t_kernel_stats_a2c_pixel_16.txt)
//   <2, 16, 8>: one row per workgroup, sixteen samples per round (the same 128 registers of inputs in flight)
// s_part: [32][8] floats of LDS.
template <int R, int RB, int WPR>
__device__ __forceinline__ void gemv_rows_body(const float* __restrict__ x, const float* __restrict__ w,
                                               const float* __restrict__ bias, float* __restrict__ y, int o2, int b0, int B, int K,
                                               int O, int act, float (*s_part)[8]) {
  static_assert(WPR == 4 || WPR == 8, "a row's K parts: 4 or 8 waves");
  constexpr int RPW = 8 / WPR;                             // output rows per workgroup
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, row = wave / WPR, part = wave % WPR;
  const int o = o2 * RPW + row;
  const int nv = K >> 2, nvq = (nv + WPR - 1) / WPR;       // float4 per row / per part
  const int v0 = part * nvq, v1 = min(nv, v0 + nvq);
  const int nb = min(32, B - b0);
  const float4* __restrict__ w4 = reinterpret_cast<const float4*>(w + (int64_t)min(o, O - 1) * K);
  const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x + (int64_t)b0 * K);
  float4 wv[R];
  int vi[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int v = v0 + lane + 64 * i;
    vi[i] = v < v1 ? v : -1;
    wv[i] = w4[v < v1 ? v : (v1 > v0 ? v1 - 1 : 0)];
  }
  for (int bb = 0; bb < nb; bb += RB) {
    float4 xv[RB][R];
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const int b = min(bb + u, nb - 1);
#pragma unroll
      for (int i = 0; i < R; ++i) xv[u][i] = x4[(int64_t)b * nv + (vi[i] >= 0 ? vi[i] : 0)];
    }
    float acc[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      float a_ = 0.f;
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const float4 a = wv[i], xx = xv[u][i];
        if (vi[i] >= 0) a_ += (a.x * xx.x + a.y * xx.y) + (a.z * xx.z + a.w * xx.w);
      }
      acc[u] = a_;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {      // RB independent butterflies, interleaved by offset
#pragma unroll
      for (int u = 0; u < RB; ++u) acc[u] += __shfl_xor(acc[u], off, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < RB; ++u)
        if (bb + u < nb) s_part[bb + u][wave] = acc[u];
    }
  }
  __syncthreads();
  // thread t < RPW * nb: (row, sample)
  const int t = threadIdx.x;
  if (t < RPW * nb) {
    const int r = t / nb, b = t - r * nb, oo = o2 * RPW + r;
    if (oo < O) {
      const float* sp = &s_part[b][WPR * r];
      float v = (sp[0] + sp[1]) + (sp[2] + sp[3]);
      if constexpr (WPR == 8) v = v + ((sp[4] + sp[5]) + (sp[6] + sp[7]));
      y[(int64_t)(b0 + b) * O + oo] = rr_act(v + (bias ? bias[oo] : 0.f), act);
    }
  }
}

// (Measured and removed, round 5 -- the eight-wave form above stayed the fastest at 8 AND 16 samples:
//   gemv_rows_body<2, 16, 8>  sixteen samples per round, K in eighths             a2c_pixel 215 k against 224-226 k env-steps/s
//   eight-sample groups on separate workgroups (two per output pair at 16)      221 k
//   two output rows per wave, four waves per workgroup (half the input reads)   222 k; ppo_pixel 116.1 k against 117.6 k
//  profiles/r05y_bench_agents_gemv16.jsonl, r05z3_bench_agents_gemv_split.jsonl, r05z4_bench_agents_gemv_pair.jsonl (second pair
//  of lines: the eight-wave form in the same call): the launch is a latency chain -- weights, inputs,
//  butterflies, LDS exchange -- that eight waves per workgroup hide best, not a traffic problem.)
