// q_mlp: n_step_dqn_feature (examples.py:408-424: 5 workers, rollout length 5, VanillaNet over FCBody(state_dim), ONE RMSprop
// optimiser, a target network copied every 200 steps) over device-resident cart-pole environments (cartpole_env.h).
//
//   q_mlp_rollout_kernel   NStepDQN_agent.py:31-57 as ONE launch of one workgroup: per step the observation narrowed to float32
//                          (what tensor() uploads), the body (4 -> H -> H, relu or tanh), q, the epsilon-greedy action -- the
//                          exploration draws are made by the host ahead of the launch, in the reference's order, and read from
//                          fixed addresses --, the environment step, reward, mask and one appended row of the episode ring per
//                          episode that ended; then the TARGET network's forward of the last observation and its max.
//   q_mlp_update_kernel    NStepDQN_agent.py:58-65 and the whole backward as ONE launch of one workgroup: the return scan, the
//                          forward recomputed from the stored observations (same inputs, same parameters: the graph the reference
//                          kept), 0.5 mean (q_a - ret)^2 and its gradient with respect to all six tensors, written into the
//                          optimiser's flat gradient buffer at the parameters' own offsets.
//
// Both are chains of dependent layers over a few rows: latency-bound, nothing to spread over 256 CUs.  Plain fp32 VALU code as in
// cat_mlp.hip (the rollout's environment lanes and weight staging ARE cartpole_rollout.h's): weights are copied to LDS once per
// launch, activations are kept TRANSPOSED ([unit][row]) and read 16 bytes at a time, every dot product is one FMA chain in
// ascending k.  The update walks the rows in blocks of 64 (its body staging and layers are mlp_update_block.h's); every gradient
// element is owned by ONE thread that adds its rows in ascending order, block after block: no atomics, the same bits on every
// launch.
#include "common.h"
#include "mlp_update_block.h"
#include <math.h>

namespace {

// ---------------------------------------------------------------------------------------------------- the rollout
__host__ __device__ constexpr size_t rollout_lds_floats(int H, int N) {
  return 2 * q_net_weight_floats(H)                                            // online, target
         + round_up4(kA * kMaxN)                                         // q [N][A]
         + (size_t)kS * round_up8(N) + 2 * (size_t)H * round_up8(N);     // x^T [S][NP], h1^T, h2^T [H][NP]
}

template <int H, int GATE>
__global__ void __launch_bounds__(256)
q_mlp_rollout_kernel(dra_q_mlp_net net, dra_q_mlp_rollout_io io) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int N = io.n_env, T = io.t_len, NP = round_up8(N);

  const QNetWeights<H> online(lds), target(lds + q_net_weight_floats(H));
  float* sQ = lds + 2 * q_net_weight_floats(H);             // [N][A]
  float* sXT = sQ + round_up4(kA * kMaxN);            // [S][NP]
  float* sH1T = sXT + kS * NP;                        // [H][NP]
  float* sH2T = sH1T + H * NP;                        // [H][NP]
  const int total = (int)(sH2T + H * NP - lds);
  for (int i = tid; i < total; i += 256) lds[i] = 0.f;
  const int64_t t0 = *io.step_counter;                // (rewritten by thread 0 behind the last barrier)
  __syncthreads();

  // ---- both networks' weights, once per launch
  online.stage(net.param, net, tid);
  target.stage(net.target, net, tid);

  // ---- the environments: lane e of wave 0 carries environment e
  const bool env_lane = tid < N;
  CartPoleLanes lanes;
  lanes.load(io, tid);
  const float reward = (float)(1.0 * io.reward_coef);

  for (int t = 0; t <= T; ++t) {
    const QNetWeights<H>& w = t < T ? online : target;          // NStepDQN_agent.py:56: the bootstrap is the TARGET network's
    if (env_lane) lanes.observe(sXT, NP, io.out_state, N, T, t, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(sXT, w.body.w1, w.body.b1, sH1T, kS, NP, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(sH1T, w.body.w2, w.body.b2, sH2T, H, NP, tid);
    __syncthreads();
    // ---- the head: one output per thread, (environment e, action c)
    if (tid < N * kA) {
      const int e = tid / kA, c = tid - e * kA;
      const float* hT = sH2T + e;
      const float* wr = w.wq + c * (H + 1);
      float acc = 0.f;
#pragma unroll 8
      for (int k = 0; k < H; ++k) acc = fmaf(hT[k * NP], wr[k], acc);
      acc += w.bq[c];
      sQ[tid] = acc;
      if (t < T) io.out_q[(int64_t)t * N * kA + tid] = acc;
    }
    __syncthreads();
    if (t == T) {
      if (env_lane) io.bootstrap[tid] = fmaxf(sQ[tid * kA], sQ[tid * kA + 1]);      // torch.max(q_target, dim=1)
      break;
    }
    // ---- epsilon-greedy action (torch_utils.py:51-58 with the draws made ahead), environment step, ring append: wave 0
    if (tid < 64) {
      int arg = 0;
      if (env_lane) {
        const int64_t o = (int64_t)t * N + tid;
        arg = sQ[tid * kA + 1] > sQ[tid * kA] ? 1 : 0;              // np.argmax: the first maximum
        if (io.explore[o]) arg = io.random_action[o] == 1 ? 1 : 0;
      }
      lanes.step(io, t, arg, reward, t0 + t, tid, tid);
    }
    // (wave 0 writes the next observation into x^T next: layer 1 of this step, its only reader, is three barriers back; q is
    // rewritten behind the three barriers of the next step)
  }
  __syncthreads();
  lanes.store(io, tid);
  if (tid == 0) *io.step_counter = t0 + T;
}

// ---------------------------------------------------------------------------------------------------- the update
constexpr int kUB = 64;          // rows of one block
constexpr int kLD = kUB + 4;     // row stride of the transposed activations: 16-byte aligned, consecutive units 4 banks apart
constexpr int kMaxRows = 1024;   // ret [rows] stays in LDS

__host__ __device__ constexpr size_t update_lds_floats(int H) {
  return update_body_floats(H) + (size_t)kA * H + 4                                   // W1^T, W2^T, W2, b1, b2; the head, its bias
         + kMaxRows + 3 * kUB                                                         // ret, d, action, the loss partials
         + (size_t)kS * kLD + 3 * (size_t)H * kLD;                                    // x^T, h1^T, h2^T (later dz1^T), dz2^T
}

template <int H, int GATE>
__global__ void __launch_bounds__(256)
q_mlp_update_kernel(dra_q_mlp_net net, dra_q_mlp_update_io io) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int TPU = 256 / H;       // threads that share one unit's row of dW2
  constexpr int KPT = H / TPU;       // columns of it each carries
  const int tid = threadIdx.x;
  const int N = io.n_env, T = io.t_len, R = T * N;
  const float* __restrict__ P = net.param;

  const UpdateBody<H> w(lds);             // W1^T, W2^T, W2 as stored, b1, b2
  float* sWq = w.head;                    // [A][H]
  float* sBq = sWq + kA * H;              // [A] (+ pad)
  float* sRet = sBq + 4;                  // [R]
  float* sD = sRet + kMaxRows;            // [kUB]: (q_a - ret) / R of the block's rows, 0 behind the last row
  int* sAct = reinterpret_cast<int*>(sD + kUB);      // [kUB]
  float* sRed = sD + 2 * kUB;             // [kUB]: the loss partials
  float* sXT = sRed + kUB;                // [S][kLD]
  float* sH1T = sXT + kS * kLD;           // [H][kLD]
  float* sH2T = sH1T + H * kLD;           // [H][kLD]: h2^T, then dz1^T
  float* sG2T = sH2T + H * kLD;           // [H][kLD]: dz2^T

  w.stage(net, tid);
  for (int i = tid; i < kA * H; i += 256) sWq[i] = P[net.wq + i];
  if (tid < kA) sBq[tid] = P[net.bq + tid];
  // ---- returns: NStepDQN_agent.py:58-60, one environment per thread, backwards from the bootstrap
  const float gamma = (float)io.discount;
  for (int e = tid; e < N; e += 256) {
    float ret = io.bootstrap[e];
    for (int t = T - 1; t >= 0; --t) {
      const int r = t * N + e;
      ret = __fadd_rn(io.reward[r], __fmul_rn(__fmul_rn(gamma, io.mask[r]), ret));
      sRet[r] = ret;
      io.out_ret[r] = ret;
    }
  }
  __syncthreads();

  // what this thread owns of the gradient
  const int u2 = tid / TPU, k2 = (tid % TPU) * KPT;       // dW2 [u2][k2 .. k2 + KPT), db2 [u2] on the first of the unit's threads
  float gW2[KPT], gB2 = 0.f;
#pragma unroll
  for (int i = 0; i < KPT; ++i) gW2[i] = 0.f;
  const int u1 = tid / kS, j1 = tid % kS;                 // dW1 [u1][j1] (tid < S H), db1 [u1] where j1 == 0
  float gW1 = 0.f, gB1 = 0.f;
  const int aq = tid / H, kq = tid % H;                   // dWq [aq][kq] (tid < A H); dbq [tid - A H] on the two threads behind
  float gWq = 0.f, gBq = 0.f;
  float loss = 0.f;
  const float inv_rows = 1.f / (float)R;

  for (int r0 = 0; r0 < R; r0 += kUB) {
    // ---- x^T of the block (256 threads: 64 rows x 4), zero behind the last row
    {
      const int row = tid / kS, j = tid % kS;
      sXT[j * kLD + row] = r0 + row < R ? io.state[(int64_t)(r0 + row) * kS + j] : 0.f;
    }
    __syncthreads();
    block_layer<H, GATE, false, kUB>(sXT, w.w1, w.b1, nullptr, sH1T, kS, tid);
    __syncthreads();
    block_layer<H, GATE, false, kUB>(sH1T, w.w2, w.b2, nullptr, sH2T, H, tid);
    __syncthreads();
    // ---- q of the action taken, dq = (q_a - ret) / R, the loss
    if (tid < kUB) {
      const int r = r0 + tid;
      float d = 0.f;
      int a = 0;
      if (r < R) {
        a = io.action[r] == 1 ? 1 : 0;
        const float* wr = sWq + a * H;
        float acc = 0.f;
#pragma unroll 8
        for (int k = 0; k < H; ++k) acc = fmaf(sH2T[k * kLD + tid], wr[k], acc);
        const float diff = (acc + sBq[a]) - sRet[r];
        loss = fmaf(diff, diff, loss);
        d = diff * inv_rows;
      }
      sD[tid] = d;
      sAct[tid] = a;
    }
    __syncthreads();
    // ---- dz2 = dq wq[a] gate'(h2); the head's gradient
    for (int i = tid; i < H * kUB; i += 256) {
      const int k = i / kUB, r = i % kUB;
      sG2T[k * kLD + r] = gate_back<GATE>(sD[r] * sWq[sAct[r] * H + k], sH2T[k * kLD + r]);
    }
    if (tid < kA * H) {
#pragma unroll 1
      for (int r = 0; r < kUB; r += 4) {
        const f32x4 h = *reinterpret_cast<const f32x4*>(&sH2T[kq * kLD + r]);
#pragma unroll
        for (int c = 0; c < 4; ++c) gWq = fmaf(sAct[r + c] == aq ? sD[r + c] : 0.f, h[c], gWq);
      }
    } else if (tid < kA * H + kA) {
#pragma unroll 1
      for (int r = 0; r < kUB; ++r) gBq += sAct[r] == tid - kA * H ? sD[r] : 0.f;
    }
    __syncthreads();
    // ---- dW2 += dz2 h1^T, db2 += dz2; dz1 = (dz2 W2) gate'(h1) into h2^T's place (its readers are behind the barrier)
#pragma unroll 1
    for (int r = 0; r < kUB; r += 4) {
      const f32x4 dz = *reinterpret_cast<const f32x4*>(&sG2T[u2 * kLD + r]);
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const f32x4 h = *reinterpret_cast<const f32x4*>(&sH1T[(k2 + i) * kLD + r]);
#pragma unroll
        for (int c = 0; c < 4; ++c) gW2[i] = fmaf(dz[c], h[c], gW2[i]);
      }
      if (k2 == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) gB2 += dz[c];
      }
    }
    block_layer<H, GATE, true, kUB>(sG2T, w.w2n, nullptr, sH1T, sH2T, H, tid);
    __syncthreads();
    // ---- dW1 += dz1 x^T, db1 += dz1
    if (tid < kS * H) {
#pragma unroll 1
      for (int r = 0; r < kUB; r += 4) {
        const f32x4 dz = *reinterpret_cast<const f32x4*>(&sH2T[u1 * kLD + r]);
        const f32x4 x = *reinterpret_cast<const f32x4*>(&sXT[j1 * kLD + r]);
#pragma unroll
        for (int c = 0; c < 4; ++c) gW1 = fmaf(dz[c], x[c], gW1);
        if (j1 == 0) {
#pragma unroll
          for (int c = 0; c < 4; ++c) gB1 += dz[c];
        }
      }
    }
    __syncthreads();       // (the next block rewrites x^T and h2^T)
  }

  // ---- every element of the six tensors, nothing between them
  float* __restrict__ Gd = io.grad;
#pragma unroll
  for (int i = 0; i < KPT; ++i) Gd[net.w2 + u2 * H + k2 + i] = gW2[i];
  if (k2 == 0) Gd[net.b2 + u2] = gB2;
  if (tid < kS * H) {
    Gd[net.w1 + tid] = gW1;
    if (j1 == 0) Gd[net.b1 + u1] = gB1;
  }
  if (tid < kA * H) Gd[net.wq + tid] = gWq;
  else if (tid < kA * H + kA) Gd[net.bq + tid - kA * H] = gBq;
  if (tid < kUB) sRed[tid] = loss;
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int i = 0; i < kUB; ++i) s += sRed[i];
    io.out_loss[0] = 0.5f * (s * inv_rows);
  }
}

bool offsets_ok(const dra_q_mlp_net* net) { return offsets_nonnegative({net->w1, net->b1, net->w2, net->b2, net->wq, net->bq}); }

}  // namespace

DRA_API int dra_q_mlp_supported(int state_dim, int n_actions, int hidden, int n_env, int gate) {
  return cartpole_mlp_supported(state_dim, n_actions, hidden, n_env, gate);
}

DRA_API int dra_q_mlp_update_supported(int state_dim, int n_actions, int hidden, int rows, int gate) {
  if (cartpole_mlp_supported(state_dim, n_actions, hidden, 1, gate)) return DRA_EINVAL;
  return rows < 1 || rows > kMaxRows ? DRA_EINVAL : DRA_OK;
}

DRA_API int dra_q_mlp_rollout(const dra_q_mlp_net* net, const dra_q_mlp_rollout_io* io, void* stream) {
  if (!net || !io || !net->param || !net->target) return DRA_EINVAL;
  if (cartpole_mlp_supported(net->state_dim, net->n_actions, net->hidden, io->n_env, net->gate)) return DRA_EINVAL;
  if (!offsets_ok(net) || !cartpole_io_ok(io)) return DRA_EINVAL;
  if (!io->step_counter || !io->explore || !io->random_action || !io->out_q || !io->bootstrap) return DRA_EINVAL;
  return dispatch_hidden_gate(net->hidden, net->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_one_workgroup<&q_mlp_rollout_kernel<H, GATE>>(rollout_lds_floats(H, io->n_env) * sizeof(float), net, io, stream);
  });
}

DRA_API int dra_q_mlp_update(const dra_q_mlp_net* net, const dra_q_mlp_update_io* io, void* stream) {
  if (!net || !io || !net->param) return DRA_EINVAL;
  if (io->t_len < 1 || io->n_env < 1 || (int64_t)io->t_len * io->n_env > kMaxRows) return DRA_EINVAL;
  if (dra_q_mlp_update_supported(net->state_dim, net->n_actions, net->hidden, io->t_len * io->n_env, net->gate)) return DRA_EINVAL;
  if (!offsets_ok(net)) return DRA_EINVAL;
  if (!io->state || !io->action || !io->reward || !io->mask || !io->bootstrap || !io->grad || !io->out_ret || !io->out_loss)
    return DRA_EINVAL;
  return dispatch_hidden_gate(net->hidden, net->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_one_workgroup<&q_mlp_update_kernel<H, GATE>>(update_lds_floats(H) * sizeof(float), net, io, stream);
  });
}
