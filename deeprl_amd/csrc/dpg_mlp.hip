// dpg_mlp: the DDPG / TD3 update (DDPG_agent.py:62-100, TD3_agent.py:62-108; examples.py:554-617: 17 -> 400 -> 300 -> {6, 1} relu
// MLPs, minibatch 100, two Adam optimisers, polyak-averaged targets) as a few eager launches.  "dpg": deterministic policy gradient.
//
//   dpg_critic_pass_kernel   row-tiled: a workgroup carries 16 minibatch rows through the TARGET actor and critic(s) (y = r + gamma
//                            mask min_i Q_i'(s', clamp(pi'(s') + clamp(sigma eps)))), then through the online critic(s) forward and
//                            back (dz chain); activations and dz of every layer go to a workspace in HBM
//   dpg_wgrad_adam_kernel    tile-owned: one wave per 16 x 16 tile of one layer's [W | b]: dW[n][k] = sum_row dz[row][n] x[row][k]
//                            over ALL rows, then Adam on that tile of the flat parameter buffer in place.  The gradient never
//                            reaches HBM and no element has two owners (no atomics: the same bits on every launch)
//   dpg_policy_pass_kernel   row-tiled: a = pi(s), critic 1 forward on (s, a) with the weights just stepped, dq = -1 / B back to the
//                            critic's input, da through the tanh, the actor's dz chain.  No critic weight gradient is formed
//   (dpg_wgrad_adam_kernel again for the actor; dra_soft_update, optim.hip, for the targets)
//   dpg_act_kernel           the actor forward alone for n <= 128 rows (behaviour action, eval_step)
//
// Every dependency between stages is a launch boundary: no workgroup waits on another, no persistent grid.  The chain is
// latency-bound (100 rows through ~130 k-parameter networks): weights stream from L2, a workgroup's activations stay in LDS.
// Contractions run on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation); operand layout as in ppo_mlp.hip: lane l,
// c16 = l & 15, g = l >> 4 gives A[i = c16][k = g], B[k = g][j = c16] and receives D[i = 4 g + reg][j = c16].  No dimension
// needs to be a multiple of 16 or 4: every operand outside a tensor is replaced by zero where it is loaded.
#include "common.h"
#include "cont_env.h"
#include "pendulum_env.h"
#include "mlp_rollout.h"
#include <math.h>

namespace {

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

constexpr int kMaxB = 128, kMaxS = 64, kMaxA = 16, kMaxH = 512;
constexpr int kRows = 16;                     // minibatch rows of a row-tiled workgroup
constexpr int kLdX = kMaxS + kMaxA + 4;       // stride of the [rows][state | action] tile
constexpr int kActNone = 0;
constexpr int kMaxJobs = 6;
constexpr int kThreads = 512, kWaves = kThreads / 64;    // of a row-tiled workgroup: 8 waves walk a layer's unit tiles
// The row-tiled kernels are chains of dependent layers whose weights come from L2: what a tile costs is the number of times a
// wave WAITS for memory, not the bytes.  Operands are therefore requested a chunk at a time with unconditional loads (indices
// clamped into the tensor, values outside it replaced by zero afterwards) so that a chunk's loads are all in flight together.
constexpr int kChunk = 8;

__host__ __device__ constexpr int ld_hidden(int h1, int h2) { return (((h1 > h2 ? h1 : h2) + 3) & ~3) + 4; }
__host__ __device__ constexpr size_t pass_lds_floats(int h1, int h2, int n_buf) {
  return (size_t)kRows * kLdX + (size_t)n_buf * kRows * ld_hidden(h1, h2) + 4 * kRows;
}

// workspace (floats): y [B] | q [2][B] | loss [B] | x = [s | a] [B][S + A] | per critic: h1, h2, dz1, dz2, dz3 | actor: h1, h2,
// dz1, dz2, a [B][A], dz3 [B][A]
struct Ws {
  float *y, *q, *loss, *x;
  float *c_h1[2], *c_h2[2], *c_dz1[2], *c_dz2[2], *c_dz3[2];
  float *a_h1, *a_h2, *a_dz1, *a_dz2, *a_out, *a_dz3;
  int64_t total;
};
__host__ __device__ inline Ws ws_layout(float* base, int B, int S, int A, int H1, int H2, int n_critics) {
  Ws w;
  int64_t o = 0;
  auto take = [&](int64_t n) { float* p = base + o; o += n; return p; };
  w.y = take(B); w.q = take(2 * (int64_t)B); w.loss = take(B); w.x = take((int64_t)B * (S + A));
  for (int c = 0; c < 2; ++c) {
    const bool on = c < n_critics;
    w.c_h1[c] = take(on ? (int64_t)B * H1 : 0); w.c_h2[c] = take(on ? (int64_t)B * H2 : 0);
    w.c_dz1[c] = take(on ? (int64_t)B * H1 : 0); w.c_dz2[c] = take(on ? (int64_t)B * H2 : 0);
    w.c_dz3[c] = take(on ? B : 0);
  }
  w.a_h1 = take((int64_t)B * H1); w.a_h2 = take((int64_t)B * H2);
  w.a_dz1 = take((int64_t)B * H1); w.a_dz2 = take((int64_t)B * H2);
  w.a_out = take((int64_t)B * A); w.a_dz3 = take((int64_t)B * A);
  w.total = o;
  return w;
}

template <int ACT>
__device__ __forceinline__ float act_f(float x) {
  if constexpr (ACT == kGateRelu) return fmaxf(x, 0.f);
  else if constexpr (ACT == kGateTanh) return tanhf(x);
  else return x;
}
// gradient through the gate, from the gate's OUTPUT h (torch's threshold_backward on the result / tanh_backward)
template <int ACT>
__device__ __forceinline__ float dact_f(float dh, float h) {
  if constexpr (ACT == kGateRelu) return h > 0.f ? dh : 0.f;
  else if constexpr (ACT == kGateTanh) return dh * (1.f - h * h);
  else return dh;
}

// rows [row0, row0 + 16) x `ncols` columns of a [B][stride] fp32 / fp64 array into sDst[r][col0 + c] (fp64 narrowed on load:
// what the agents' _f32 cast does); rows past B are zeros
__device__ __forceinline__ void load_rows(float* sDst, int ld, int col0, const void* src, int64_t stride, int in_f64, int ncols,
                                          int row0, int B) {
  for (int i = threadIdx.x; i < kRows * ncols; i += kThreads) {
    const int r = i / ncols, c = i - r * ncols, row = row0 + r;
    float v = 0.f;
    if (row < B) {
      const int64_t o = (int64_t)row * stride + c;
      v = in_f64 ? (float)static_cast<const double*>(src)[o] : static_cast<const float*>(src)[o];
    }
    sDst[r * ld + col0 + c] = v;
  }
}

// sOut[r][col_out + n] = act(b[n] + sum_k sIn[r][k] W[n][k]) for n < N, W [N][K] row-major at P + off_w.  Wave w takes the unit
// tiles w, w + 8, ...; k walks as 16 tk + 4 g + r (a lane's four weights of a step are consecutive in memory), kChunk steps
// requested at once, two accumulator chains.  g_out (optional): the same values to a [B][N] array in HBM, rows below B only.
template <int ACT, int CH>
__device__ __forceinline__ void fwd_layer_ch(const float* __restrict__ P, int off_w, int off_b, int N, int K, const float* sIn, int ld_in,
                                             float* sOut, int ld_out, int col_out, float* __restrict__ g_out, int row0, int B) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c16 = l & 15, g = l >> 4;
  const int NT = (N + 15) >> 4;
  for (int nt = w; nt < NT; nt += kWaves) {
    const int n = 16 * nt + c16;
    const bool nok = n < N;
    const float* __restrict__ wrow = P + off_w + (int64_t)(nok ? n : 0) * K;
    const float* xrow = sIn + c16 * ld_in;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < K; kc += 16 * CH) {
      float a[CH][4], b[CH][4];
#pragma unroll
      for (int s = 0; s < CH; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = min(kc + 16 * s + 4 * g + r, K - 1);
          a[s][r] = xrow[k];
          b[s][r] = wrow[k];
        }
      __builtin_amdgcn_sched_barrier(0);     // every request of the chunk is issued before its first use
#pragma unroll
      for (int s = 0; s < CH; ++s) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool kok = kc + 16 * s + 4 * g + r < K;
          a[s][r] = kok ? a[s][r] : 0.f;
          b[s][r] = (kok && nok) ? b[s][r] : 0.f;
        }
        acc0 = MFMA16(a[s][0], b[s][0], acc0);
        acc1 = MFMA16(a[s][1], b[s][1], acc1);
        acc0 = MFMA16(a[s][2], b[s][2], acc0);
        acc1 = MFMA16(a[s][3], b[s][3], acc1);
      }
    }
    const f32x4 acc = acc0 + acc1;
    const float bias = nok ? P[off_b + n] : 0.f;
    if (nok) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        const float v = act_f<ACT>(acc[r] + bias);
        sOut[row * ld_out + col_out + n] = v;
        if (g_out && row0 + row < B) g_out[(int64_t)(row0 + row) * N + n] = v;
      }
    }
  }
}

// The same layer when every weight row and the input tile are 16-byte aligned (K a multiple of 4: the hidden layers of the
// optimiser's flat buffer): a lane's four k of a step are ONE 16-byte request, 8 steps in flight per wave -- a workgroup pulls
// its weights alone through one CU, and what bounds it is the bytes it has in flight.
template <int ACT>
__device__ __forceinline__ void fwd_layer_x4(const float* __restrict__ P, int off_w, int off_b, int N, int K, const float* sIn, int ld_in,
                                             float* sOut, int ld_out, int col_out, float* __restrict__ g_out, int row0, int B) {
  constexpr int CH = 8;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c16 = l & 15, g = l >> 4;
  const int NT = (N + 15) >> 4;
  for (int nt = w; nt < NT; nt += kWaves) {
    const int n = 16 * nt + c16;
    const bool nok = n < N;
    const float* __restrict__ wrow = P + off_w + (int64_t)(nok ? n : 0) * K;
    const float* xrow = sIn + c16 * ld_in;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < K; kc += 16 * CH) {
      f32x4 a[CH], b[CH];
#pragma unroll
      for (int s = 0; s < CH; ++s) {
        const int k = min(kc + 16 * s + 4 * g, K - 4);
        a[s] = *reinterpret_cast<const f32x4*>(xrow + k);
        b[s] = *reinterpret_cast<const f32x4*>(wrow + k);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < CH; ++s) {
        if (kc + 16 * s < K) {             // (wave-uniform)
          const bool kok = kc + 16 * s + 4 * g < K;
          const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
          const f32x4 av = kok ? a[s] : zero, bv = (kok && nok) ? b[s] : zero;
          acc0 = MFMA16(av[0], bv[0], acc0);
          acc1 = MFMA16(av[1], bv[1], acc1);
          acc0 = MFMA16(av[2], bv[2], acc0);
          acc1 = MFMA16(av[3], bv[3], acc1);
        }
      }
    }
    const f32x4 acc = acc0 + acc1;
    const float bias = nok ? P[off_b + n] : 0.f;
    if (nok) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        const float v = act_f<ACT>(acc[r] + bias);
        sOut[row * ld_out + col_out + n] = v;
        if (g_out && row0 + row < B) g_out[(int64_t)(row0 + row) * N + n] = v;
      }
    }
  }
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int ACT>
__device__ __forceinline__ void fwd_layer(const float* __restrict__ P, int off_w, int off_b, int N, int K, const float* sIn, int ld_in,
                                          float* sOut, int ld_out, int col_out, float* __restrict__ g_out, int row0, int B) {
  // (a chunk's steps past K multiply zeros: the first layers, K = S or S + A, take the short chunk)
  if (K <= 32) fwd_layer_ch<ACT, 2>(P, off_w, off_b, N, K, sIn, ld_in, sOut, ld_out, col_out, g_out, row0, B);
  else if (((K | off_w | ld_in) & 3) == 0 && aligned16(P) && aligned16(sIn))
    fwd_layer_x4<ACT>(P, off_w, off_b, N, K, sIn, ld_in, sOut, ld_out, col_out, g_out, row0, B);
  else fwd_layer_ch<ACT, kChunk>(P, off_w, off_b, N, K, sIn, ld_in, sOut, ld_out, col_out, g_out, row0, B);
}

// sH[r][j] <- dact((sum_n sDz[r][n] W[n][k_off + j]), sH[r][j]) for j < K_out, IN PLACE over the layer's stored output (W rows
// of length ld_w).  Wave w takes the tiles w, w + 8, ... of j; consecutive lanes read consecutive weights.
template <int ACT, int CH>
__device__ __forceinline__ void bwd_layer_ch(const float* __restrict__ P, int off_w, int ld_w, int k_off, int K_out, int N,
                                             const float* sDz, int ld_dz, float* sH, int ld_h, float* __restrict__ g_out, int row0, int B) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c16 = l & 15, g = l >> 4;
  const int KT = (K_out + 15) >> 4;
  for (int kt = w; kt < KT; kt += kWaves) {
    const int j = 16 * kt + c16;
    const bool jok = j < K_out;
    const float* __restrict__ wcol = P + off_w + k_off + (jok ? j : 0);
    const float* drow = sDz + c16 * ld_dz;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int nc = 0; nc < N; nc += 8 * CH) {
      float a[CH][2], b[CH][2];
#pragma unroll
      for (int s = 0; s < CH; ++s)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int n = min(nc + 8 * s + 4 * h + g, N - 1);
          a[s][h] = drow[n];
          b[s][h] = wcol[(int64_t)n * ld_w];
        }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < CH; ++s) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bool ok = nc + 8 * s + 4 * h + g < N;
          a[s][h] = ok ? a[s][h] : 0.f;
          b[s][h] = (ok && jok) ? b[s][h] : 0.f;
        }
        acc0 = MFMA16(a[s][0], b[s][0], acc0);
        acc1 = MFMA16(a[s][1], b[s][1], acc1);
      }
    }
    const f32x4 acc = acc0 + acc1;
    if (jok) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        const float v = dact_f<ACT>(acc[r], sH[row * ld_h + j]);
        sH[row * ld_h + j] = v;
        if (g_out && row0 + row < B) g_out[(int64_t)(row0 + row) * K_out + j] = v;
      }
    }
  }
}

// The same with 16-byte requests (rows of W 16-byte aligned, K_out a multiple of 4): a wave takes 64 columns, lane (c16, g)
// the four columns 64 jb + 4 c16 + r of row n0 + g -- one request -- as the B operands of four accumulators (accumulator r
// holds column 4 c16 + r of the block: any assignment of columns to lanes serves, as long as the result is read the same way).
template <int ACT>
__device__ __forceinline__ void bwd_layer_x4(const float* __restrict__ P, int off_w, int ld_w, int k_off, int K_out, int N,
                                             const float* sDz, int ld_dz, float* sH, int ld_h, float* __restrict__ g_out, int row0, int B) {
  constexpr int CH = 8;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c16 = l & 15, g = l >> 4;
  const int KB = (K_out + 63) >> 6;
  for (int jb = w; jb < KB; jb += kWaves) {
    const int j0 = 64 * jb + 4 * c16;
    const bool jok = j0 < K_out;
    const float* __restrict__ wcol = P + off_w + k_off + (jok ? j0 : 0);
    const float* drow = sDz + c16 * ld_dz;
    f32x4 acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int nc = 0; nc < N; nc += 4 * CH) {
      float a[CH];
      f32x4 b[CH];
#pragma unroll
      for (int s = 0; s < CH; ++s) {
        const int n = min(nc + 4 * s + g, N - 1);
        a[s] = drow[n];
        b[s] = *reinterpret_cast<const f32x4*>(wcol + (int64_t)n * ld_w);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < CH; ++s) {
        if (nc + 4 * s < N) {              // (wave-uniform)
          const bool ok = nc + 4 * s + g < N;
          const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
          const float av = ok ? a[s] : 0.f;
          const f32x4 bv = (ok && jok) ? b[s] : zero;
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[r] = MFMA16(av, bv[r], acc[r]);
        }
      }
    }
    if (jok) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int row = 4 * g + rr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = j0 + r;
          const float v = dact_f<ACT>(acc[r][rr], sH[row * ld_h + j]);
          sH[row * ld_h + j] = v;
          if (g_out && row0 + row < B) g_out[(int64_t)(row0 + row) * K_out + j] = v;
        }
      }
    }
  }
}

template <int ACT>
__device__ __forceinline__ void bwd_layer(const float* __restrict__ P, int off_w, int ld_w, int k_off, int K_out, int N,
                                          const float* sDz, int ld_dz, float* sH, int ld_h, float* __restrict__ g_out, int row0, int B) {
  if (N > 16 && ((ld_w | (off_w + k_off) | K_out) & 3) == 0 && aligned16(P))
    bwd_layer_x4<ACT>(P, off_w, ld_w, k_off, K_out, N, sDz, ld_dz, sH, ld_h, g_out, row0, B);
  else if (N <= 16) bwd_layer_ch<ACT, 2>(P, off_w, ld_w, k_off, K_out, N, sDz, ld_dz, sH, ld_h, g_out, row0, B);      // the heads
  else bwd_layer_ch<ACT, kChunk>(P, off_w, ld_w, k_off, K_out, N, sDz, ld_dz, sH, ld_h, g_out, row0, B);
}

struct Dims { int S, A, H1, H2, B; };

// the actor's forward for the rows whose states sit in sX[:, :S]: h1 -> sA, h2 -> sB, tanh(head) -> sX[:, S : S + A]
template <int GATE>
__device__ __forceinline__ void actor_forward(const dra_dpg_net& net, const Dims& d, float* sX, float* sA, float* sB, int ldh,
                                              float* g_h1, float* g_h2, float* g_a, int row0) {
  const int* o = net.actor;
  fwd_layer<GATE>(net.param, o[0], o[1], d.H1, d.S, sX, kLdX, sA, ldh, 0, g_h1, row0, d.B);
  __syncthreads();
  fwd_layer<GATE>(net.param, o[2], o[3], d.H2, d.H1, sA, ldh, sB, ldh, 0, g_h2, row0, d.B);
  __syncthreads();
  fwd_layer<kGateTanh>(net.param, o[4], o[5], d.A, d.H2, sB, ldh, sX, kLdX, d.S, g_a, row0, d.B);
  __syncthreads();
}
// a critic's hidden layers on sX = [s | a]: h1 -> sA, h2 -> sB
template <int GATE>
__device__ __forceinline__ void critic_hidden(const dra_dpg_net& net, int c, const Dims& d, const float* sX, float* sA, float* sB,
                                              int ldh, float* g_h1, float* g_h2, int row0) {
  const int* o = net.critic[c];
  fwd_layer<GATE>(net.param, o[0], o[1], d.H1, d.S + d.A, sX, kLdX, sA, ldh, 0, g_h1, row0, d.B);
  __syncthreads();
  fwd_layer<GATE>(net.param, o[2], o[3], d.H2, d.H1, sA, ldh, sB, ldh, 0, g_h2, row0, d.B);
  __syncthreads();
}

template <int GATE>
__global__ void __launch_bounds__(kThreads)
dpg_critic_pass_kernel(dra_dpg_net on, dra_dpg_net tg, dra_dpg_batch bt, dra_dpg_step st, float* __restrict__ wsp) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Dims d = {on.state_dim, on.action_dim, on.h1, on.h2, bt.batch};
  const int tid = threadIdx.x, row0 = blockIdx.x * kRows, ldh = ld_hidden(d.H1, d.H2), NC = on.n_critics;
  const Ws ws = ws_layout(wsp, d.B, d.S, d.A, d.H1, d.H2, NC);
  float* sX = lds;
  float* sA = sX + kRows * kLdX;
  float* sB = sA + kRows * ldh;
  float* sQ = sB + kRows * ldh;       // [2][16]
  float* sY = sQ + 2 * kRows;         // [16]
  float* sDq = sY + kRows;            // [16]

  // ---- target: a' = pi'(s') (+ clipped noise, TD3), q' = min_i Q_i'(s', a'), y = r + gamma mask q'
  load_rows(sX, kLdX, 0, bt.next_state, bt.next_state_stride, bt.in_f64, d.S, row0, d.B);
  __syncthreads();
  actor_forward<GATE>(tg, d, sX, sA, sB, ldh, nullptr, nullptr, nullptr, row0);
  if (NC == 2) {      // TD3_agent.py:75-79
    if (tid < kRows * d.A) {
      const int r = tid / d.A, c = tid - r * d.A, row = row0 + r;
      if (row < d.B) {
        const float eps = bt.noise ? bt.noise[(int64_t)row * d.A + c] : gauss_noise(st.noise_seed, st.noise_counter, d.B, row, c);
        const float nz = fminf(fmaxf(eps * st.td3_noise, -st.td3_noise_clip), st.td3_noise_clip);
        sX[r * kLdX + d.S + c] = fminf(fmaxf(sX[r * kLdX + d.S + c] + nz, st.action_low), st.action_high);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {      // (unrolled: the per-critic offsets and workspace pointers stay in registers)
    if (c >= NC) continue;
    critic_hidden<GATE>(tg, c, d, sX, sA, sB, ldh, nullptr, nullptr, row0);
    fwd_layer<kActNone>(tg.param, tg.critic[c][4], tg.critic[c][5], 1, d.H2, sB, ldh, sQ + c * kRows, 1, 0, nullptr, row0, d.B);
    __syncthreads();
  }
  if (tid < kRows) {
    const int row = row0 + tid;
    float y = 0.f;
    if (row < d.B) {
      const float qn = NC == 2 ? fminf(sQ[tid], sQ[kRows + tid]) : sQ[tid];
      y = bt.reward[row] + (st.discount * bt.mask[row]) * qn;
      ws.y[row] = y;
    }
    sY[tid] = y;
  }
  __syncthreads();

  // ---- online critic(s): forward on (s, a), dq, the dz chain
  load_rows(sX, kLdX, 0, bt.state, bt.state_stride, bt.in_f64, d.S, row0, d.B);
  load_rows(sX, kLdX, d.S, bt.action, bt.action_stride, bt.in_f64, d.A, row0, d.B);
  __syncthreads();
  for (int i = tid; i < kRows * (d.S + d.A); i += kThreads) {
    const int r = i / (d.S + d.A), c = i - r * (d.S + d.A);
    if (row0 + r < d.B) ws.x[(int64_t)(row0 + r) * (d.S + d.A) + c] = sX[r * kLdX + c];
  }
  // DDPG: mean_rows(0.5 (q - y)^2) -> dq = (q - y) / B;  TD3: mse(q1, y) + mse(q2, y) -> dq_i = 2 (q_i - y) / B
  const float coef = (NC == 2 ? 2.f : 1.f) / (float)d.B;
  float loss = 0.f;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    if (c >= NC) continue;
    const int* o = on.critic[c];
    critic_hidden<GATE>(on, c, d, sX, sA, sB, ldh, ws.c_h1[c], ws.c_h2[c], row0);
    fwd_layer<kActNone>(on.param, o[4], o[5], 1, d.H2, sB, ldh, sQ + c * kRows, 1, 0, nullptr, row0, d.B);
    __syncthreads();
    if (tid < kRows) {
      const int row = row0 + tid;
      const float q = sQ[c * kRows + tid], diff = q - sY[tid];
      const float dq = row < d.B ? diff * coef : 0.f;
      sDq[tid] = dq;
      loss += NC == 2 ? diff * diff : 0.5f * (diff * diff);
      if (row < d.B) {
        ws.q[c * d.B + row] = q;
        ws.c_dz3[c][row] = dq;
        if (c == NC - 1) ws.loss[row] = loss;
      }
    }
    __syncthreads();
    bwd_layer<GATE>(on.param, o[4], d.H2, 0, d.H2, 1, sDq, 1, sB, ldh, ws.c_dz2[c], row0, d.B);
    __syncthreads();
    bwd_layer<GATE>(on.param, o[2], d.H1, 0, d.H1, d.H2, sB, ldh, sA, ldh, ws.c_dz1[c], row0, d.B);
    __syncthreads();
  }
}

template <int GATE>
__global__ void __launch_bounds__(kThreads)
dpg_policy_pass_kernel(dra_dpg_net on, int B, float* __restrict__ wsp) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Dims d = {on.state_dim, on.action_dim, on.h1, on.h2, B};
  const int tid = threadIdx.x, row0 = blockIdx.x * kRows, ldh = ld_hidden(d.H1, d.H2);
  const Ws ws = ws_layout(wsp, d.B, d.S, d.A, d.H1, d.H2, on.n_critics);
  float* sX = lds;
  float* sA = sX + kRows * kLdX;      // actor h1 -> dz1
  float* sB = sA + kRows * ldh;       // actor h2 -> dz2
  float* sC = sB + kRows * ldh;       // critic h1 -> dz1
  float* sD = sC + kRows * ldh;       // critic h2 -> dz2
  float* sDq = sD + kRows * ldh;      // [16]

  load_rows(sX, kLdX, 0, ws.x, d.S + d.A, 0, d.S, row0, d.B);      // the states the critic pass stored (fp32)
  if (tid < kRows) sDq[tid] = -1.f / (float)d.B;                   // -mean_rows(Q1(s, pi(s)))
  __syncthreads();
  actor_forward<GATE>(on, d, sX, sA, sB, ldh, ws.a_h1, ws.a_h2, ws.a_out, row0);
  critic_hidden<GATE>(on, 0, d, sX, sC, sD, ldh, nullptr, nullptr, row0);
  const int* o = on.critic[0];
  bwd_layer<GATE>(on.param, o[4], d.H2, 0, d.H2, 1, sDq, 1, sD, ldh, nullptr, row0, d.B);
  __syncthreads();
  bwd_layer<GATE>(on.param, o[2], d.H1, 0, d.H1, d.H2, sD, ldh, sC, ldh, nullptr, row0, d.B);
  __syncthreads();
  // da = dz1 W1[:, S : S + A], through the head's tanh (in place over a)
  bwd_layer<kGateTanh>(on.param, o[0], d.S + d.A, d.S, d.A, d.H1, sC, ldh, sX + d.S, kLdX, ws.a_dz3, row0, d.B);
  __syncthreads();
  const int* p = on.actor;
  bwd_layer<GATE>(on.param, p[4], d.H2, 0, d.H2, d.A, sX + d.S, kLdX, sB, ldh, ws.a_dz2, row0, d.B);
  __syncthreads();
  bwd_layer<GATE>(on.param, p[2], d.H1, 0, d.H1, d.H2, sB, ldh, sA, ldh, ws.a_dz1, row0, d.B);
}

template <int GATE>
__global__ void __launch_bounds__(kThreads)
dpg_act_kernel(dra_dpg_net net, const void* __restrict__ state, int64_t state_stride, int in_f64, int n, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Dims d = {net.state_dim, net.action_dim, net.h1, net.h2, n};
  const int row0 = blockIdx.x * kRows, ldh = ld_hidden(d.H1, d.H2);
  float* sX = lds;
  float* sA = sX + kRows * kLdX;
  float* sB = sA + kRows * ldh;
  load_rows(sX, kLdX, 0, state, state_stride, in_f64, d.S, row0, n);
  __syncthreads();
  actor_forward<GATE>(net, d, sX, sA, sB, ldh, nullptr, nullptr, out, row0);
}

// ------------------------------------------------------------------------------------------------ acting on a device environment
// One agent transition (dra_dpg_env_act_io in the header): dpg_act_kernel's forward on ONE row -- the same LDS layout, the same
// actor_forward, hence the same bits -- then the behaviour action, the ring row and the environment step in wave 0.  The fp64
// scratch (observation [kMaxS], action [kMaxA]) lies BEHIND the forward's tiles in the dynamic region: a static array in front of
// it would move the tiles off their 16-byte alignment and fwd_layer onto its other path.
constexpr int kEnvPendulum = 0, kEnvSynthetic = 1;
constexpr int kModeWarmup = 0, kModeGauss = 1, kModeOU = 2;
__host__ __device__ constexpr size_t env_act_lds_floats(int h1, int h2) { return pass_lds_floats(h1, h2, 2) + 2 * (kMaxS + kMaxA); }

template <int GATE>
__global__ void __launch_bounds__(kThreads)
dpg_env_act_kernel(dra_dpg_net net, dra_dpg_env_act_io io) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Dims d = {net.state_dim, net.action_dim, net.h1, net.h2, 1};
  const int tid = threadIdx.x, ldh = ld_hidden(d.H1, d.H2);
  float* sX = lds;
  float* sA = sX + kRows * kLdX;
  float* sB = sA + kRows * ldh;
  double* sObs = reinterpret_cast<double*>(lds + pass_lds_floats(d.H1, d.H2, 2));
  double* sAct = sObs + kMaxS;
  const bool pendulum = io.env_kind == kEnvPendulum;

  // ---- the observation the action is chosen on
  PendulumState pst = {0.0, 0.0};
  if (pendulum) {
    if (tid == 0) {
      pst.th = io.env_state[0];
      pst.thd = io.env_state[1];
      pendulum_observe(pst, sObs);
    }
  } else if (tid < d.S) {
    sObs[tid] = io.env_state[tid];
  }
  __syncthreads();
  for (int i = tid; i < kRows * d.S; i += kThreads) {        // load_rows of dpg_act_kernel with n = 1: the rows behind it are zeros
    const int r = i / d.S, c = i - r * d.S;
    sX[r * kLdX + c] = r == 0 ? (float)sObs[c] : 0.f;
  }
  __syncthreads();
  actor_forward<GATE>(net, d, sX, sA, sB, ldh, nullptr, nullptr, io.out_action, 0);

  if (tid >= 64) return;       // (no workgroup barrier below: wave 0 alone)
  // ---- the behaviour action (DDPG_agent.py:62-69), lane dd = dimension dd
  const int64_t mode = *io.mode;
  double x_next = 0.0;
  if (tid < d.A) {
    const double a = (double)sX[d.S + tid], v = io.v[tid];
    double x = io.ou_x[tid], act;
    if (mode == kModeWarmup) act = v;
    else if (mode == kModeGauss) act = a + v;
    else {
      x = (x + ((io.ou_theta * (io.ou_mu - x)) * io.ou_dt)) + v;
      act = a + x;
    }
    const double lo = io.bounds[0], hi = io.bounds[1];
    act = act < lo ? lo : (act > hi ? hi : act);
    sAct[tid] = act;
    x_next = x;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");      // the wave's lanes read each other's actions below
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

  // ---- the ring row and the environment step
  int64_t slot = *io.slot;
  const bool bad_slot = slot < 0 || slot >= io.capacity;
  if (bad_slot) slot = 0;
  if (tid < d.S) io.ring_frames[slot * d.S + tid] = sObs[tid];
  if (tid < d.A) io.ring_actions[slot * d.A + tid] = sAct[tid];
  const uint64_t seed = (uint64_t)*io.env_seed;
  int64_t counter = *io.env_counter;
  double ep_return = *io.ep_return, reward = 0.0, ended = 0.0;
  int32_t ep_steps = *io.ep_steps;
  bool done = false;
  if (pendulum) {
    if (tid == 0) {
      done = pendulum_step(pst, counter, ep_steps, ep_return, seed, sAct[0], io.horizon, reward, ended);
      io.env_state[0] = pst.th;
      io.env_state[1] = pst.thd;
    }
    done = __shfl((int)done, 0, 64) != 0;
  } else {
    // envs.py SyntheticContinuous.step: every lane forms the mean action and the terminal, lane j the component j
    double m = 0.0;
    for (int dd = 0; dd < d.A; ++dd) m += (double)fminf(fmaxf((float)sAct[dd], -1.f), 1.f);
    m = m / (double)d.A;
    counter = counter + 1;
    done = cenv_done(seed, counter, io.horizon);
    if (tid < d.S) io.env_state[tid] = cenv_next_state(seed, counter, tid, sObs[tid], m, done);
    reward = cenv_reward(seed, counter);
    ep_return = ep_return + reward;
    if (done) {
      ended = ep_return;
      ep_return = 0.0;
    }
  }
  if (tid < d.A) io.ou_x[tid] = done ? io.ou_x0[tid] : x_next;
  if (tid == 0) {
    io.ring_rewards[slot] = reward;
    io.ring_masks[slot] = done ? 0 : 1;
    const int64_t t = *io.step_counter, n_ep = *io.ep_count;
    if (done) {
      double* row = io.ep_ring + (n_ep % io.ring_cap) * 3;
      row[0] = (double)t;
      row[1] = 0.0;
      row[2] = ended;
      *io.ep_count = n_ep + 1;
    }
    *io.step_counter = t + 1;
    *io.env_counter = counter;
    *io.ep_steps = ep_steps;
    *io.ep_return = ep_return;
    if (bad_slot) *io.err = *io.err + 1;
  }
}

// ------------------------------------------------------------------------------------------------ evaluation on a device pendulum
// n_episodes greedy episodes of `horizon` steps (dra_dpg_eval_io in the header) as ROWS of dpg_act_kernel's forward: the pendulum
// has no terminal state but the step limit and draws its reset state from the total step counter, so episode e of an evaluation
// that starts at counter c0 begins at pendulum_reset(c0 + e horizon), known before anything runs; the episodes are independent and
// walk in lockstep.  Workgroup b owns the episodes [16 b, 16 b + 16): lane r of wave 0 carries episode 16 b + r in registers (its
// state and its fp64 return) and row r of the tile -- the same LDS layout and the same actor_forward as dpg_act_kernel, so row r's
// action has dra_dpg_act's bits for that observation.  The trip count is `horizon` for every thread of every workgroup: no thread
// skips a barrier.  The environment's words are read by every workgroup when it starts and written once, by the workgroup that
// is the last to have read them (a ticket in *io.arrive): nobody waits for anybody.
template <int GATE>
__global__ void __launch_bounds__(kThreads)
dpg_eval_kernel(dra_dpg_net net, dra_dpg_eval_io io) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int n = io.n_episodes;
  const Dims d = {kPendulumS, kPendulumA, net.h1, net.h2, n};      // (dra_dpg_eval_supported: the pendulum's sizes, known here)
  const int tid = threadIdx.x, row0 = blockIdx.x * kRows, ldh = ld_hidden(d.H1, d.H2);
  float* sX = lds;
  float* sA = sX + kRows * kLdX;
  float* sB = sA + kRows * ldh;
  const int64_t horizon = io.horizon, c0 = *io.env_counter;
  const uint64_t seed = (uint64_t)*io.env_seed;
  const int e = row0 + tid;
  const bool live = tid < kRows && e < n;

  // ---- what Task.reset() does at the head of eval_episode: the episode's start state, return 0
  PendulumState st = {0.0, 0.0};
  double ret = 0.0;
  if (live) pendulum_reset(st, seed, c0 + (int64_t)e * horizon);
  for (int i = tid; i < kRows * d.S; i += kThreads) sX[(i / d.S) * kLdX + i % d.S] = 0.f;      // rows past n_episodes stay zeros
  // ---- the environment as the host loop leaves it after its last auto reset.  It depends on c0 alone, so it is written here, ahead
  // of the loop, by the workgroup that is the LAST to have read c0 and the seed (the ticket's release orders the reads in front of it)
  if (tid == 0 && __hip_atomic_fetch_add(io.arrive, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1) {
    const int64_t c1 = c0 + (int64_t)n * horizon;
    PendulumState fresh;
    pendulum_reset(fresh, seed, c1);
    io.env_state[0] = fresh.th;
    io.env_state[1] = fresh.thd;
    *io.env_counter = c1;
    *io.ep_steps = 0;
    *io.ep_return = 0.0;
    *io.out_steps = (int64_t)n * horizon;
    *io.arrive = 0;
  }
  __syncthreads();

  for (int64_t t = 0; t < horizon; ++t) {
    if (live) {
      double obs[kPendulumS];
      pendulum_observe(st, obs);
#pragma unroll
      for (int c = 0; c < kPendulumS; ++c) sX[tid * kLdX + c] = (float)obs[c];
      if (io.out_state) {
        double* row = io.out_state + ((int64_t)e * (horizon + 1) + t) * kPendulumVars;
        row[0] = st.th;
        row[1] = st.thd;
      }
    }
    __syncthreads();
    actor_forward<GATE>(net, d, sX, sA, sB, ldh, nullptr, nullptr, nullptr, row0);
    if (live) {
      const float a = sX[tid * kLdX + d.S];
      if (io.out_action) io.out_action[(int64_t)e * horizon + t] = a;
      ret = ret + pendulum_advance(st, (double)a);
    }
    __syncthreads();      // before the next observation overwrites sX
  }

  if (live) {
    io.out_return[e] = ret;
    if (io.out_state) {
      double* row = io.out_state + ((int64_t)e * (horizon + 1) + horizon) * kPendulumVars;
      row[0] = st.th;
      row[1] = st.thd;
    }
  }
}

// ------------------------------------------------------------------------------------------------ weight gradient + Adam
// One job = one Linear layer: dz [B][N], x [B][ld_x] (K columns used), W [N][K] at off_w, b [N] at off_b.  The bias is column K of
// [W | b] (x's column K is 1): tiles_k = ceil((K + 1) / 16).
struct WJob {
  const float* dz;
  const float* x;
  int ld_x, K, N, off_w, off_b, tiles_k, tile0;
};
struct WArgs {
  WJob job[kMaxJobs];
  int n_jobs, total_tiles, B;
  float *param, *m, *v;
  float step_size, inv_sqrt_bc2, beta1, beta2, eps;
};

__global__ void __launch_bounds__(256)
dpg_wgrad_adam_kernel(WArgs a) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c16 = l & 15, g = l >> 4;
  const int tile = blockIdx.x * 4 + w;
  if (tile >= a.total_tiles) return;       // (wave-uniform)
  int ji = 0;
  for (int i = 1; i < a.n_jobs; ++i)
    if (tile >= a.job[i].tile0) ji = i;
  const WJob& jb = a.job[ji];
  const int local = tile - jb.tile0, nt = local / jb.tiles_k, kt = local - nt * jb.tiles_k;
  const int n_in = 16 * nt + c16, k = 16 * kt + c16, N = jb.N, K = jb.K, B = a.B;
  const bool nok = n_in < N;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const int nl = nok ? n_in : 0, kl = min(k, K - 1);       // clamped: every load below is unconditional (see kChunk)
  constexpr int CH = 4;
  for (int rc = 0; rc < B; rc += 8 * CH) {
    float dv[CH][2], xv[CH][2];
#pragma unroll
    for (int s = 0; s < CH; ++s)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int row = min(rc + 8 * s + 4 * h + g, B - 1);
        dv[s][h] = jb.dz[(int64_t)row * N + nl];
        xv[s][h] = jb.x[(int64_t)row * jb.ld_x + kl];
      }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < CH; ++s) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool ok = rc + 8 * s + 4 * h + g < B;
        dv[s][h] = (ok && nok) ? dv[s][h] : 0.f;
        xv[s][h] = !ok ? 0.f : (k < K ? xv[s][h] : (k == K ? 1.f : 0.f));
      }
      acc0 = MFMA16(dv[s][0], xv[s][0], acc0);
      acc1 = MFMA16(dv[s][1], xv[s][1], acc1);
    }
  }
  const f32x4 acc = acc0 + acc1;
  if (k > K) return;
  // optim.hip adam_step_kernel's element formula (torch.optim.Adam without amsgrad / weight decay), IEEE sqrt and division
  const float omb1 = 1.f - a.beta1, omb2 = 1.f - a.beta2;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = 16 * nt + 4 * g + r;
    if (n >= N) continue;
    const int64_t i = k < K ? (int64_t)jb.off_w + (int64_t)n * K + k : (int64_t)jb.off_b + n;
    const float gk = acc[r];
    const float mk = a.m[i] * a.beta1 + omb1 * gk;
    const float vk = a.v[i] * a.beta2 + omb2 * gk * gk;
    a.m[i] = mk;
    a.v[i] = vk;
    a.param[i] = a.param[i] - a.step_size * (mk / (sqrtf(vk) * a.inv_sqrt_bc2 + a.eps));
  }
}

void add_job(WArgs& a, const float* dz, const float* x, int ld_x, int K, int N, int off_w, int off_b) {
  WJob& j = a.job[a.n_jobs++];
  j.dz = dz; j.x = x; j.ld_x = ld_x; j.K = K; j.N = N; j.off_w = off_w; j.off_b = off_b;
  j.tiles_k = (K + 1 + 15) / 16;
  j.tile0 = a.total_tiles;
  a.total_tiles += ((N + 15) / 16) * j.tiles_k;
}

int launch_wgrad(WArgs& a, const dra_dpg_net* net, const dra_dpg_step* st, int B, void* stream) {
  a.B = B;
  a.param = net->param; a.m = st->exp_avg; a.v = st->exp_avg_sq;
  a.step_size = st->step_size; a.inv_sqrt_bc2 = st->inv_sqrt_bc2; a.beta1 = st->beta1; a.beta2 = st->beta2; a.eps = st->eps;
  hipLaunchKernelGGL(dpg_wgrad_adam_kernel, dim3((unsigned)((a.total_tiles + 3) / 4)), dim3(256), 0, dra_stream(stream), a);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}

int check_net(const dra_dpg_net* n) {
  if (!n || !n->param) return DRA_EINVAL;
  if (n->n_critics != 1 && n->n_critics != 2) return DRA_EINVAL;
  for (int i = 0; i < 6; ++i) {
    if (n->actor[i] < 0) return DRA_EINVAL;
    for (int c = 0; c < n->n_critics; ++c)
      if (n->critic[c][i] < 0) return DRA_EINVAL;
  }
  return DRA_OK;
}
bool same_dims(const dra_dpg_net* a, const dra_dpg_net* b) {
  return a->state_dim == b->state_dim && a->action_dim == b->action_dim && a->h1 == b->h1 && a->h2 == b->h2 && a->gate == b->gate &&
         a->n_critics == b->n_critics;
}
int check_step(const dra_dpg_step* st) {
  if (!st || !st->exp_avg || !st->exp_avg_sq) return DRA_EINVAL;
  if (!(st->step_size > 0.f) || !(st->inv_sqrt_bc2 > 0.f) || !(st->eps >= 0.f)) return DRA_EINVAL;
  if (!(st->beta1 >= 0.f && st->beta1 < 1.f && st->beta2 >= 0.f && st->beta2 < 1.f)) return DRA_EINVAL;
  return DRA_OK;
}

template <int GATE>
int launch_critic_pass(const dra_dpg_net* on, const dra_dpg_net* tg, const dra_dpg_batch* bt, const dra_dpg_step* st, float* ws,
                       void* stream) {
  const size_t bytes = pass_lds_floats(on->h1, on->h2, 2) * sizeof(float);
  static DraLdsAttr lds_attr;
  if (int rc = dra_grant_lds(lds_attr, reinterpret_cast<const void*>(&dpg_critic_pass_kernel<GATE>), bytes)) return rc;
  hipLaunchKernelGGL((dpg_critic_pass_kernel<GATE>), dim3((unsigned)((bt->batch + kRows - 1) / kRows)), dim3(kThreads), bytes,
                     dra_stream(stream), *on, *tg, *bt, *st, ws);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}
template <int GATE>
int launch_policy_pass(const dra_dpg_net* on, int B, float* ws, void* stream) {
  const size_t bytes = pass_lds_floats(on->h1, on->h2, 4) * sizeof(float);
  static DraLdsAttr lds_attr;
  if (int rc = dra_grant_lds(lds_attr, reinterpret_cast<const void*>(&dpg_policy_pass_kernel<GATE>), bytes)) return rc;
  hipLaunchKernelGGL((dpg_policy_pass_kernel<GATE>), dim3((unsigned)((B + kRows - 1) / kRows)), dim3(kThreads), bytes, dra_stream(stream),
                     *on, B, ws);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}
template <int GATE>
int launch_act(const dra_dpg_net* net, const void* state, int64_t stride, int in_f64, int n, float* out, void* stream) {
  const size_t bytes = pass_lds_floats(net->h1, net->h2, 2) * sizeof(float);
  static DraLdsAttr lds_attr;
  if (int rc = dra_grant_lds(lds_attr, reinterpret_cast<const void*>(&dpg_act_kernel<GATE>), bytes)) return rc;
  hipLaunchKernelGGL((dpg_act_kernel<GATE>), dim3((unsigned)((n + kRows - 1) / kRows)), dim3(kThreads), bytes, dra_stream(stream), *net,
                     state, stride, in_f64, n, out);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}

template <int GATE>
int launch_env_act(const dra_dpg_net* net, const dra_dpg_env_act_io* io, void* stream) {
  const size_t bytes = env_act_lds_floats(net->h1, net->h2) * sizeof(float);
  static DraLdsAttr lds_attr;
  if (int rc = dra_grant_lds(lds_attr, reinterpret_cast<const void*>(&dpg_env_act_kernel<GATE>), bytes)) return rc;
  hipLaunchKernelGGL((dpg_env_act_kernel<GATE>), dim3(1), dim3(kThreads), bytes, dra_stream(stream), *net, *io);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}

template <int GATE>
int launch_eval(const dra_dpg_net* net, const dra_dpg_eval_io* io, void* stream) {
  const size_t bytes = pass_lds_floats(net->h1, net->h2, 2) * sizeof(float);
  static DraLdsAttr lds_attr;
  if (int rc = dra_grant_lds(lds_attr, reinterpret_cast<const void*>(&dpg_eval_kernel<GATE>), bytes)) return rc;
  hipLaunchKernelGGL((dpg_eval_kernel<GATE>), dim3((unsigned)((io->n_episodes + kRows - 1) / kRows)), dim3(kThreads), bytes,
                     dra_stream(stream), *net, *io);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}

}  // namespace

DRA_API int dra_dpg_supported(int batch, int state_dim, int action_dim, int h1, int h2, int gate, int n_critics) {
  if (batch < 1 || batch > kMaxB || state_dim < 1 || state_dim > kMaxS || action_dim < 1 || action_dim > kMaxA) return DRA_EINVAL;
  if (h1 < 1 || h1 > kMaxH || h2 < 1 || h2 > kMaxH) return DRA_EINVAL;
  if ((gate != kGateRelu && gate != kGateTanh) || (n_critics != 1 && n_critics != 2)) return DRA_EINVAL;
  return DRA_OK;
}

DRA_API int dra_dpg_workspace_floats(int batch, int state_dim, int action_dim, int h1, int h2, int n_critics, int64_t* out) {
  if (!out || dra_dpg_supported(batch, state_dim, action_dim, h1, h2, kGateRelu, n_critics)) return DRA_EINVAL;
  *out = ws_layout(nullptr, batch, state_dim, action_dim, h1, h2, n_critics).total;
  return DRA_OK;
}

DRA_API int dra_dpg_critic_update(const dra_dpg_net* online, const dra_dpg_net* target, const dra_dpg_batch* batch,
                                  const dra_dpg_step* step, float* workspace, void* stream) {
  if (check_net(online) || check_net(target) || !same_dims(online, target) || !batch || !workspace || check_step(step))
    return DRA_EINVAL;
  const dra_dpg_net& n = *online;
  if (dra_dpg_supported(batch->batch, n.state_dim, n.action_dim, n.h1, n.h2, n.gate, n.n_critics)) return DRA_EINVAL;
  if (!batch->state || !batch->next_state || !batch->action || !batch->reward || !batch->mask) return DRA_EINVAL;
  if (batch->state_stride < n.state_dim || batch->next_state_stride < n.state_dim || batch->action_stride < n.action_dim)
    return DRA_EINVAL;
  if (n.n_critics == 2 && (!(step->td3_noise_clip >= 0.f) || !(step->action_low <= step->action_high))) return DRA_EINVAL;
  const int rc = n.gate == kGateRelu ? launch_critic_pass<kGateRelu>(online, target, batch, step, workspace, stream)
                                     : launch_critic_pass<kGateTanh>(online, target, batch, step, workspace, stream);
  if (rc) return rc;
  const int B = batch->batch, X = n.state_dim + n.action_dim;
  const Ws ws = ws_layout(workspace, B, n.state_dim, n.action_dim, n.h1, n.h2, n.n_critics);
  WArgs a = {};
  for (int c = 0; c < n.n_critics; ++c) {
    const int32_t* o = n.critic[c];
    add_job(a, ws.c_dz1[c], ws.x, X, X, n.h1, o[0], o[1]);
    add_job(a, ws.c_dz2[c], ws.c_h1[c], n.h1, n.h1, n.h2, o[2], o[3]);
    add_job(a, ws.c_dz3[c], ws.c_h2[c], n.h2, n.h2, 1, o[4], o[5]);
  }
  return launch_wgrad(a, online, step, B, stream);
}

DRA_API int dra_dpg_actor_update(const dra_dpg_net* online, const dra_dpg_batch* batch, const dra_dpg_step* step, float* workspace,
                                 void* stream) {
  if (check_net(online) || !batch || !workspace || check_step(step)) return DRA_EINVAL;
  const dra_dpg_net& n = *online;
  if (dra_dpg_supported(batch->batch, n.state_dim, n.action_dim, n.h1, n.h2, n.gate, n.n_critics)) return DRA_EINVAL;
  const int B = batch->batch;
  const int rc = n.gate == kGateRelu ? launch_policy_pass<kGateRelu>(online, B, workspace, stream)
                                     : launch_policy_pass<kGateTanh>(online, B, workspace, stream);
  if (rc) return rc;
  const Ws ws = ws_layout(workspace, B, n.state_dim, n.action_dim, n.h1, n.h2, n.n_critics);
  WArgs a = {};
  const int32_t* o = n.actor;
  add_job(a, ws.a_dz1, ws.x, n.state_dim + n.action_dim, n.state_dim, n.h1, o[0], o[1]);
  add_job(a, ws.a_dz2, ws.a_h1, n.h1, n.h1, n.h2, o[2], o[3]);
  add_job(a, ws.a_dz3, ws.a_h2, n.h2, n.h2, n.action_dim, o[4], o[5]);
  return launch_wgrad(a, online, step, B, stream);
}

DRA_API int dra_dpg_act(const dra_dpg_net* net, const void* state, int64_t state_stride, int in_f64, int n, float* out_action,
                        void* stream) {
  if (check_net(net) || !state || !out_action) return DRA_EINVAL;
  if (dra_dpg_supported(n, net->state_dim, net->action_dim, net->h1, net->h2, net->gate, net->n_critics)) return DRA_EINVAL;
  if (state_stride < net->state_dim) return DRA_EINVAL;
  return net->gate == kGateRelu ? launch_act<kGateRelu>(net, state, state_stride, in_f64, n, out_action, stream)
                                : launch_act<kGateTanh>(net, state, state_stride, in_f64, n, out_action, stream);
}

DRA_API int dra_dpg_env_act_supported(int env_kind, int state_dim, int action_dim, int h1, int h2, int gate) {
  if (dra_dpg_supported(1, state_dim, action_dim, h1, h2, gate, 1)) return DRA_EINVAL;
  if (env_kind == kEnvPendulum) return state_dim == kPendulumS && action_dim == kPendulumA ? DRA_OK : DRA_EINVAL;
  return env_kind == kEnvSynthetic ? DRA_OK : DRA_EINVAL;
}

DRA_API int dra_dpg_env_act(const dra_dpg_net* net, const dra_dpg_env_act_io* io, void* stream) {
  if (check_net(net) || !io) return DRA_EINVAL;
  if (dra_dpg_env_act_supported(io->env_kind, net->state_dim, net->action_dim, net->h1, net->h2, net->gate)) return DRA_EINVAL;
  if (io->horizon < 1 || io->ring_cap < 1 || io->capacity < 1) return DRA_EINVAL;
  if (!io->env_state || !io->env_counter || !io->ep_steps || !io->ep_return || !io->env_seed || !io->step_counter || !io->ep_count ||
      !io->ep_ring || !io->mode || !io->slot || !io->bounds || !io->v || !io->ou_x || !io->ou_x0 || !io->ring_frames ||
      !io->ring_actions || !io->ring_rewards || !io->ring_masks || !io->out_action || !io->err)
    return DRA_EINVAL;
  return net->gate == kGateRelu ? launch_env_act<kGateRelu>(net, io, stream) : launch_env_act<kGateTanh>(net, io, stream);
}

DRA_API int dra_dpg_eval_supported(int n_episodes, int64_t horizon, int state_dim, int action_dim, int h1, int h2, int gate) {
  if (n_episodes < 1 || n_episodes > kMaxB || horizon < 1 || horizon > 65536 || (int64_t)n_episodes * horizon > 65536) return DRA_EINVAL;
  return dra_dpg_env_act_supported(kEnvPendulum, state_dim, action_dim, h1, h2, gate);
}

DRA_API int dra_dpg_eval(const dra_dpg_net* net, const dra_dpg_eval_io* io, void* stream) {
  if (check_net(net) || !io) return DRA_EINVAL;
  if (dra_dpg_eval_supported(io->n_episodes, io->horizon, net->state_dim, net->action_dim, net->h1, net->h2, net->gate)) return DRA_EINVAL;
  if (!io->env_state || !io->env_counter || !io->ep_steps || !io->ep_return || !io->env_seed || !io->out_return || !io->out_steps ||
      !io->arrive)
    return DRA_EINVAL;
  return net->gate == kGateRelu ? launch_eval<kGateRelu>(net, io, stream) : launch_eval<kGateTanh>(net, io, stream);
}
