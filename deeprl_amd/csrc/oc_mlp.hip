// oc_mlp: option_critic_feature (examples.py:450-468: 5 workers, rollout length 5, OptionCriticNet over FCBody(state_dim) with 2
// options, ONE RMSprop optimiser, a target network copied every 200 steps) over device-resident cart-pole environments
// (cartpole_env.h).
//
//   oc_mlp_rollout_kernel  OptionCritic_agent.py:55-93 as ONE launch of one workgroup: per step the observation narrowed to
//                          float32, the body (4 -> H -> H, relu or tanh), the three heads (q, beta = sigmoid, the intra-option
//                          logits) over all 256 threads, then on the environment's lane of wave 0 sample_option
//                          (OptionCritic_agent.py:29-49) and the action of the chosen option's policy -- by inverse CDF of
//                          uniforms the host drew ahead of the launch, read from fixed addresses --, the environment step,
//                          reward, mask, the carried prev_option / is_initial and one appended row of the episode ring per
//                          episode that ended; then the TARGET network's q and beta of the last observation and the bootstrap.
//   oc_mlp_update_kernel   OptionCritic_agent.py:95-116 and the whole backward as ONE launch of one workgroup: the return scan,
//                          the per-row terms from the rollout's stored q / beta / logits (csrc/option_critic.hip's phase A, its
//                          operation order), the body recomputed from the stored observations, the gradient of pi_loss + q_loss
//                          + beta_loss with respect to all ten tensors, written into the optimiser's flat gradient buffer at the
//                          parameters' own offsets.
//
// q_mlp.hip's mould: latency-bound chains over a few rows, plain fp32 VALU code, weights copied to LDS once per launch,
// activations kept TRANSPOSED ([unit][row]) and read 16 bytes at a time, every dot product one FMA chain in ascending k.  The
// update walks the rows in blocks of 64; every gradient element is owned by ONE thread that adds its rows in ascending order,
// block after block: no atomics, the same bits on every launch.  The three heads' gradient is one product per block: the rows'
// coefficients are laid out densely ([output row][row], zero where a row does not reach an output), so that every thread runs the
// same chain whatever the options were.
//
// The decision rule is RESTATED here, not shared with rollout_roles.h's oc_head_row_fold_wg: there one thread of a workgroup
// decides for one row with its arrays in registers and optional outputs; here 64 lanes decide at once with their rows in LDS (the
// option count is a run-time value: per-lane arrays indexed by it would live in scratch) and carry prev_option / is_initial in
// registers across the steps.  What both share is what fixes the bits: inv_cdf_row (rollout_roles.h) and categorical_row
// (common.h) are called, not rewritten.  The update's body staging and layers are mlp_update_block.h's; its gradient bookkeeping
// is written in place (mlp_rollout.h's banner: the measurements).
#include "common.h"
#include "mlp_update_block.h"
#include "rollout_roles.h"
#include <math.h>

namespace {

constexpr int kMaxO = 8;                          // options
constexpr int kMaxJ = 2 * kMaxO + kMaxO * kA;     // the three heads' outputs
constexpr int kJP = kMaxJ + 1;                    // an environment's row of head outputs in LDS: odd, lanes fall on different banks
constexpr int kPiP = 2 * kMaxO + 1;               // an environment's pi_opt | pi_hat

// ---------------------------------------------------------------------------------------------------- the rollout
// `rows` head rows [rows][H + 1] and their biases; every region starts at a multiple of 4 floats
__host__ __device__ constexpr size_t head_floats(int H, int rows) { return round_up4(rows * (H + 1)) + round_up4(rows); }
__host__ __device__ constexpr size_t rollout_lds_floats(int H, int N, int O) {
  return 2 * body_weight_floats(H) + head_floats(H, 2 * O + O * kA) + head_floats(H, 2 * O)      // online, target (q and beta only)
         + round_up4(N * kJP) + round_up4(N * kPiP)                                               // head outputs, pi_opt | pi_hat
         + (size_t)kS * round_up8(N) + 2 * (size_t)H * round_up8(N);                              // x^T [S][NP], h1^T, h2^T [H][NP]
}

// head rows in the order q [O], beta [O], pi [O A]: the target's two heads are a prefix
template <int H>
struct Heads {
  float *w, *b;
  __device__ Heads(float* base, int rows) : w(base), b(base + round_up4(rows * (H + 1))) {}
  __device__ __forceinline__ void stage(const float* __restrict__ P, const dra_oc_mlp_net& net, int O, int rows, int tid) const {
    for (int i = tid; i < rows * H; i += 256) {
      const int j = i / H, k = i - j * H;
      const int src = j < O ? net.wq + i : (j < 2 * O ? net.wb + i - O * H : net.wp + i - 2 * O * H);
      w[j * (H + 1) + k] = P[src];
    }
    if (tid < rows) b[tid] = P[tid < O ? net.bq + tid : (tid < 2 * O ? net.bb + tid - O : net.bp + tid - 2 * O)];
  }
};

// the first index of q's maximum, as torch.argmax / torch.max see it (a NaN wins and stops the search)
__device__ __forceinline__ int first_max(const float* q, int O, float* qmax_out) {
  float qmax = q[0];
  int g = 0;
  for (int o = 1; o < O; ++o) {
    if (qmax != qmax) break;
    if (q[o] > qmax || q[o] != q[o]) { qmax = q[o]; g = o; }
  }
  *qmax_out = qmax;
  return g;
}

template <int H, int GATE>
__global__ void __launch_bounds__(256)
oc_mlp_rollout_kernel(dra_oc_mlp_net net, dra_oc_mlp_rollout_io io) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int N = io.n_env, T = io.t_len, NP = round_up8(N), O = net.n_options;
  const int JO = 2 * O + O * kA, JT = 2 * O;

  float* p = lds;
  const BodyWeights<H> ob(p);
  p += body_weight_floats(H);
  const Heads<H> oh(p, JO);
  p += head_floats(H, JO);
  const BodyWeights<H> tb(p);
  p += body_weight_floats(H);
  const Heads<H> th(p, JT);
  p += head_floats(H, JT);
  float* sOut = p;                                    // [N][kJP]: q [O], beta [O], logits [O][A]
  float* sPi = sOut + round_up4(N * kJP);             // [N][kPiP]: pi_opt [O], pi_hat [O] of the lane
  float* sXT = sPi + round_up4(N * kPiP);             // [S][NP]
  float* sH1T = sXT + kS * NP;                        // [H][NP]
  float* sH2T = sH1T + H * NP;                        // [H][NP]
  const int total = (int)(sH2T + H * NP - lds);
  for (int i = tid; i < total; i += 256) lds[i] = 0.f;
  const int64_t t0 = *io.step_counter;                // (rewritten by thread 0 behind the last barrier)
  __syncthreads();

  // ---- both networks' weights, once per launch
  ob.stage(net.param, net, tid);
  oh.stage(net.param, net, O, JO, tid);
  tb.stage(net.target, net, tid);
  th.stage(net.target, net, O, JT, tid);

  // ---- the environments and their carried option state: lane e of wave 0 carries environment e
  const bool env_lane = tid < N;
  CartPoleLanes lanes;
  lanes.load(io, tid);
  const float reward = (float)(1.0 * io.reward_coef);
  int prev = 0;
  bool init = false;
  if (env_lane) {
    const int64_t pin = io.prev_option[tid];
    prev = pin < 0 ? 0 : (pin >= O ? O - 1 : (int)pin);
    init = io.is_initial[tid] != 0;
  }

  for (int t = 0; t <= T; ++t) {
    const bool boot = t == T;                           // OptionCritic_agent.py:87: the bootstrap is the TARGET network's
    const BodyWeights<H>& wb = boot ? tb : ob;
    const float* hw = boot ? th.w : oh.w;
    const float* hb = boot ? th.b : oh.b;
    const int J = boot ? JT : JO;
    if (env_lane) lanes.observe(sXT, NP, io.out_state, N, T, t, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(sXT, wb.w1, wb.b1, sH1T, kS, NP, tid);
    __syncthreads();
    hidden_layer<H, GATE, 256>(sH1T, wb.w2, wb.b2, sH2T, H, NP, tid);
    __syncthreads();
    // ---- the heads over all threads: pair i = (output j, environment e), j-major
    for (int i = tid; i < N * J; i += 256) {
      const int j = i / N, e = i - j * N;
      const float* hT = sH2T + e;
      const float* wr = hw + j * (H + 1);
      float acc = 0.f;
#pragma unroll 8
      for (int k = 0; k < H; ++k) acc = fmaf(hT[k * NP], wr[k], acc);
      acc += hb[j];
      if (j >= O && j < 2 * O) acc = 1.f / (1.f + expf(-acc));
      sOut[e * kJP + j] = acc;
      if (!boot && j < 2 * O) {
        const int64_t row = (int64_t)t * N + e;
        if (j < O) io.out_q[row * O + j] = acc;
        else io.out_beta[row * O + j - O] = acc;
      }
    }
    __syncthreads();
    if (boot) {
      if (env_lane) {                                   // OptionCritic_agent.py:88-93, prev = the option of step T - 1
        const float* q = sOut + tid * kJP;
        const float* beta = q + O;
        float qmax;
        first_max(q, O, &qmax);
        io.bootstrap[tid] = (1.f - beta[prev]) * q[prev] + beta[prev] * qmax;
      }
      break;
    }
    // ---- sample_option, the action, the environment step, the ring append: wave 0
    if (tid < 64) {
      int act = 0;
      if (env_lane) {
        const float* q = sOut + tid * kJP;
        const float* beta = q + O;
        float qmax;
        const int g = first_max(q, O, &qmax);
        const float eps = io.eps[t];
        const float base = eps / (float)O, top = 1.f - eps + eps / (float)O;
        float* pi_opt = sPi + tid * kPiP;
        float* pi_hat = pi_opt + kMaxO;
        for (int o = 0; o < O; ++o) {
          const float po = o == g ? top : base;
          pi_opt[o] = po;
          pi_hat[o] = (1.f - beta[o]) * (o == prev ? 1.f : 0.f) + beta[o] * po;
        }
        const int64_t row = (int64_t)t * N + tid;
        const float* u = io.uniform + row * 3;
        const int fresh = inv_cdf_row(pi_opt, O, u[0]), continued = inv_cdf_row(pi_hat, O, u[1]);
        const int option = init ? fresh : continued;
        const float* logits = q + 2 * O + option * kA;
        int64_t a64;
        float lp, ent;
        categorical_row(logits, kA, false, 0, u[2], &a64, &lp, &ent);
        io.out_logits[row * kA + 0] = logits[0];
        io.out_logits[row * kA + 1] = logits[1];
        io.out_option[row] = option;
        io.out_prev_option[row] = prev;
        io.out_init[row] = init ? 1.f : 0.f;
        io.out_log_pi_a[row] = lp;
        io.out_entropy[row] = ent;
        prev = option;
        act = a64 == 1 ? 1 : 0;
      }
      const CartPoleRow r(io);
      bool done = false;
      double ended = 0.0;
      if (env_lane) done = lanes.advance(r, t, act, reward, tid, ended);
      lanes.append(r, done, ended, t0 + t, tid, tid);
      init = done;                                      // the next step's is_initial_states = terminals
    }
    // (wave 0 writes the next observation into x^T next: layer 1 of this step, its only reader, is four barriers back; the head
    // outputs are rewritten behind the three barriers of the next step; pi_opt | pi_hat belong to their lane)
  }
  __syncthreads();
  lanes.store(io, tid);
  if (env_lane) {
    io.prev_option[tid] = prev;
    io.is_initial[tid] = init ? 1 : 0;
  }
  if (tid == 0) *io.step_counter = t0 + T;
}

// ---------------------------------------------------------------------------------------------------- the update
constexpr int kUB = 64;          // rows of one block
constexpr int kLD = kUB + 4;     // row stride of the transposed activations: 16-byte aligned, consecutive units 4 banks apart
constexpr int kMaxRows = 1024;   // the per-row terms stay in LDS

__host__ __device__ constexpr size_t update_lds_floats(int H) {
  return update_body_floats(H) + (size_t)kMaxJ * H                                   // W1^T, W2^T, W2, b1, b2; the heads' rows
         + 5 * (size_t)kMaxRows + 16                                                 // ret / g, gz, dlogit 0 / 1, option | prev; loss partials
         + (size_t)kMaxJ * kLD                                                       // the block's coefficients [output row][row]
         + (size_t)kS * kLD + 3 * (size_t)H * kLD;                                   // x^T, h1^T, h2^T (later dz1^T), dz2^T
}

template <int H, int GATE>
__global__ void __launch_bounds__(256)
oc_mlp_update_kernel(dra_oc_mlp_net net, dra_oc_mlp_update_io io) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int TPU = 256 / H;             // threads that share one unit's row of dW2
  constexpr int KPT = H / TPU;             // columns of it each carries
  constexpr int NHE = kMaxJ * H / 256;     // head-gradient elements a thread can own: element tid + 256 m
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = io.n_env, T = io.t_len, R = T * N, O = net.n_options;
  const int OA = O * kA, J = 2 * O + OA;   // the heads' rows HERE in the order q [O], pi [O A], beta [O]: the order dh2 adds them in
  const float* __restrict__ P = net.param;

  const UpdateBody<H> w(lds);             // W1^T, W2^T, W2 as stored, b1, b2
  float* sWh = w.head;                    // [J][H]: fc_q, fc_pi, fc_beta as stored
  float* sRet = sWh + kMaxJ * H;          // [R]: the returns, then g = (q[option] - ret) / R of the row
  float* sGz = sRet + kMaxRows;           // [R]: dz_beta at prev_option
  float* sDl0 = sGz + kMaxRows;           // [R]: dlogit of action 0 / 1 of the chosen option
  float* sDl1 = sDl0 + kMaxRows;
  int* sIdx = reinterpret_cast<int*>(sDl1 + kMaxRows);      // [R]: option | prev_option << 8
  float* sRed = sDl1 + 2 * kMaxRows;      // [3][4] (+ pad): the loss partials of the four waves
  float* sC = sRed + 16;                  // [J][kLD]: the block's coefficient of output row j at row r
  float* sXT = sC + kMaxJ * kLD;          // [S][kLD]
  float* sH1T = sXT + kS * kLD;           // [H][kLD]
  float* sH2T = sH1T + H * kLD;           // [H][kLD]: h2^T, then dz1^T
  float* sG2T = sH2T + H * kLD;           // [H][kLD]: dz2^T
  float* sG = sRet;

  w.stage(net, tid);
  for (int i = tid; i < J * H; i += 256) {
    const int j = i / H;
    sWh[i] = P[j < O ? net.wq + i : (j < O + OA ? net.wp + i - O * H : net.wb + i - (O + OA) * H)];
  }
  // ---- returns: OptionCritic_agent.py:95-98, one environment per thread, backwards from the bootstrap
  const float gamma = (float)io.discount, term_reg = (float)io.termination_regularizer, ent_w = (float)io.entropy_weight;
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
  // ---- the per-row terms from what the rollout stored (option_critic.hip's phase A): row r on thread r % 256
  const float rows_f = (float)R;
  const float ge = -__fdiv_rn(ent_w, rows_f);
  float lq = 0.f, lpi = 0.f, lb = 0.f;          // this thread's loss partial sums (ascending rows)
  for (int r = tid; r < R; r += 256) {
    int64_t o = io.option[r], pv = io.prev_option[r];
    o = o < 0 ? 0 : (o >= O ? O - 1 : o);       // (both come from the rollout: always in range)
    pv = pv < 0 ? 0 : (pv >= O ? O - 1 : pv);
    const bool a1 = io.action[r] == 1;
    const float* qr = io.q + (int64_t)r * O;
    const float ret = sRet[r], qo = qr[o];
    const float diff = __fsub_rn(qo, ret), adv = __fsub_rn(ret, qo);
    const float g = __fdiv_rn(diff, rows_f);
    float qmax = qr[0], qsum = qr[0];
    for (int j = 1; j < O; ++j) { qmax = fmaxf(qmax, qr[j]); qsum = __fadd_rn(qsum, qr[j]); }
    const float e_t = io.eps[r / N];
    const float v = __fadd_rn(__fmul_rn(qmax, __fsub_rn(1.f, e_t)), __fmul_rn(__fdiv_rn(qsum, (float)O), e_t));
    const float badv = __fadd_rn(__fsub_rn(qr[pv], v), term_reg);
    const float bp = io.beta[(int64_t)r * O + pv], keep = __fsub_rn(1.f, io.init[r]);
    const float lg[kA] = {io.logits[(int64_t)r * kA], io.logits[(int64_t)r * kA + 1]};
    float lse, ent;
    categorical_row_stats(lg, kA, &lse, &ent);
    sG[r] = g;                                  // (this thread was the only reader of ret [r])
    sGz[r] = __fdiv_rn(__fmul_rn(__fmul_rn(__fmul_rn(bp, __fsub_rn(1.f, bp)), badv), keep), rows_f);
    sDl0[r] = categorical_dlogit(lg[0], lse, ent, !a1, g, ge);
    sDl1[r] = categorical_dlogit(lg[1], lse, ent, a1, g, ge);
    sIdx[r] = (int)o | ((int)pv << 8);
    io.out_adv[r] = adv;
    io.out_beta_adv[r] = badv;
    lq = __fadd_rn(lq, __fmul_rn(0.5f, __fmul_rn(diff, diff)));
    lpi = __fadd_rn(lpi, __fsub_rn(-__fmul_rn(io.log_pi_a[r], adv), __fmul_rn(ent_w, io.entropy[r])));
    lb = __fadd_rn(lb, __fmul_rn(__fmul_rn(bp, badv), keep));
  }
  // the three means: a wave butterfly, then the four waves in order (a fixed order)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lq += __shfl_xor(lq, off, 64);
    lpi += __shfl_xor(lpi, off, 64);
    lb += __shfl_xor(lb, off, 64);
  }
  if (lane == 0) { sRed[wave] = lq; sRed[4 + wave] = lpi; sRed[8 + wave] = lb; }
  __syncthreads();
  if (tid == 0) {
    float m[3];
    for (int i = 0; i < 3; ++i) m[i] = __fdiv_rn(((sRed[4 * i] + sRed[4 * i + 1]) + sRed[4 * i + 2]) + sRed[4 * i + 3], rows_f);
    io.out_loss[0] = __fadd_rn(__fadd_rn(m[1], m[0]), m[2]);      // pi_loss + q_loss + beta_loss
    io.out_loss[1] = m[0];
    io.out_loss[2] = m[1];
    io.out_loss[3] = m[2];
  }

  // what this thread owns of the gradient
  const int u2 = tid / TPU, k2 = (tid % TPU) * KPT;       // dW2 [u2][k2 .. k2 + KPT), db2 [u2] on the first of the unit's threads
  float gW2[KPT], gB2 = 0.f;
#pragma unroll
  for (int i = 0; i < KPT; ++i) gW2[i] = 0.f;
  const int u1 = tid / kS, j1 = tid % kS;                 // dW1 [u1][j1] (tid < S H), db1 [u1] where j1 == 0
  float gW1 = 0.f, gB1 = 0.f;
  float gWh[NHE], gBh = 0.f;                              // the heads: element tid + 256 m of [J][H]; the bias of row tid (tid < J)
#pragma unroll
  for (int m = 0; m < NHE; ++m) gWh[m] = 0.f;

  for (int r0 = 0; r0 < R; r0 += kUB) {
    // ---- x^T of the block (256 threads: 64 rows x 4), zero behind the last row; the heads' coefficients of the block's rows
    {
      const int row = tid / kS, j = tid % kS;
      sXT[j * kLD + row] = r0 + row < R ? io.state[(int64_t)(r0 + row) * kS + j] : 0.f;
    }
    for (int i = tid; i < J * kUB; i += 256) {
      const int j = i / kUB, c = i % kUB, r = r0 + c;
      float v = 0.f;
      if (r < R) {
        const int idx = sIdx[r], o = idx & 255, pv = idx >> 8;
        if (j < O) v = o == j ? sG[r] : 0.f;
        else if (j < O + OA) v = (j - O) / kA == o ? ((j - O) % kA ? sDl1[r] : sDl0[r]) : 0.f;
        else v = pv == j - O - OA ? sGz[r] : 0.f;
      }
      sC[j * kLD + c] = v;
    }
    __syncthreads();
    block_layer<H, GATE, false, kUB>(sXT, w.w1, w.b1, nullptr, sH1T, kS, tid);
    __syncthreads();
    block_layer<H, GATE, false, kUB>(sH1T, w.w2, w.b2, nullptr, sH2T, H, tid);
    __syncthreads();
    // ---- dz2 = (g Wq[o] + sum_a dlogit_a Wp[o A + a] + gz Wb[prev]) gate'(h2); the heads' gradient
    for (int i = tid; i < H * kUB; i += 256) {
      const int k = i / kUB, c = i % kUB, r = r0 + c;
      float v = 0.f;
      if (r < R) {
        const int idx = sIdx[r], o = idx & 255, pv = idx >> 8;
        float vp = __fmul_rn(sDl0[r], sWh[(O + o * kA) * H + k]);
        vp = __fadd_rn(vp, __fmul_rn(sDl1[r], sWh[(O + o * kA + 1) * H + k]));
        v = __fadd_rn(__fadd_rn(__fmul_rn(sG[r], sWh[o * H + k]), vp), __fmul_rn(sGz[r], sWh[(O + OA + pv) * H + k]));
      }
      sG2T[k * kLD + c] = gate_back<GATE>(v, sH2T[k * kLD + c]);
    }
#pragma unroll
    for (int m = 0; m < NHE; ++m) {
      const int i = tid + 256 * m;
      if (i < J * H) {
        const int j = i / H, k = i % H;
#pragma unroll 1
        for (int r = 0; r < kUB; r += 4) {
          const f32x4 cf = *reinterpret_cast<const f32x4*>(&sC[j * kLD + r]);
          const f32x4 h = *reinterpret_cast<const f32x4*>(&sH2T[k * kLD + r]);
#pragma unroll
          for (int c = 0; c < 4; ++c) gWh[m] = fmaf(cf[c], h[c], gWh[m]);
        }
      }
    }
    if (tid < J) {
#pragma unroll 1
      for (int r = 0; r < kUB; ++r) gBh += sC[tid * kLD + r];
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
    __syncthreads();       // (the next block rewrites x^T, the coefficients and h2^T)
  }

  // ---- every element of the ten tensors, nothing between them
  float* __restrict__ Gd = io.grad;
#pragma unroll
  for (int i = 0; i < KPT; ++i) Gd[net.w2 + u2 * H + k2 + i] = gW2[i];
  if (k2 == 0) Gd[net.b2 + u2] = gB2;
  if (tid < kS * H) {
    Gd[net.w1 + tid] = gW1;
    if (j1 == 0) Gd[net.b1 + u1] = gB1;
  }
#pragma unroll
  for (int m = 0; m < NHE; ++m) {
    const int i = tid + 256 * m;
    if (i < J * H) {
      const int j = i / H;
      Gd[j < O ? net.wq + i : (j < O + OA ? net.wp + i - O * H : net.wb + i - (O + OA) * H)] = gWh[m];
    }
  }
  if (tid < J) Gd[tid < O ? net.bq + tid : (tid < O + OA ? net.bp + tid - O : net.bb + tid - O - OA)] = gBh;
}

bool offsets_ok(const dra_oc_mlp_net* net) {
  return offsets_nonnegative({net->w1, net->b1, net->w2, net->b2, net->wq, net->bq, net->wp, net->bp, net->wb, net->bb});
}

bool options_ok(int n_options) { return n_options >= 2 && n_options <= kMaxO; }

}  // namespace

DRA_API int dra_oc_mlp_supported(int state_dim, int n_actions, int hidden, int n_env, int gate, int n_options) {
  if (!options_ok(n_options)) return DRA_EINVAL;
  return cartpole_mlp_supported(state_dim, n_actions, hidden, n_env, gate);
}

DRA_API int dra_oc_mlp_update_supported(int state_dim, int n_actions, int hidden, int rows, int gate, int n_options) {
  if (!options_ok(n_options) || cartpole_mlp_supported(state_dim, n_actions, hidden, 1, gate)) return DRA_EINVAL;
  return rows < 1 || rows > kMaxRows ? DRA_EINVAL : DRA_OK;
}

DRA_API int dra_oc_mlp_rollout(const dra_oc_mlp_net* net, const dra_oc_mlp_rollout_io* io, void* stream) {
  if (!net || !io || !net->param || !net->target) return DRA_EINVAL;
  if (dra_oc_mlp_supported(net->state_dim, net->n_actions, net->hidden, io->n_env, net->gate, net->n_options)) return DRA_EINVAL;
  if (!offsets_ok(net) || !cartpole_io_ok(io)) return DRA_EINVAL;
  if (!io->step_counter || !io->eps || !io->uniform || !io->prev_option || !io->is_initial || !io->out_q || !io->out_beta ||
      !io->out_logits || !io->out_option || !io->out_prev_option || !io->out_init || !io->out_log_pi_a || !io->out_entropy ||
      !io->bootstrap)
    return DRA_EINVAL;
  return dispatch_hidden_gate(net->hidden, net->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_one_workgroup<&oc_mlp_rollout_kernel<H, GATE>>(rollout_lds_floats(H, io->n_env, net->n_options) * sizeof(float), net,
                                                                 io, stream);
  });
}

DRA_API int dra_oc_mlp_update(const dra_oc_mlp_net* net, const dra_oc_mlp_update_io* io, void* stream) {
  if (!net || !io || !net->param) return DRA_EINVAL;
  if (io->t_len < 1 || io->n_env < 1 || (int64_t)io->t_len * io->n_env > kMaxRows) return DRA_EINVAL;
  if (dra_oc_mlp_update_supported(net->state_dim, net->n_actions, net->hidden, io->t_len * io->n_env, net->gate, net->n_options))
    return DRA_EINVAL;
  if (!offsets_ok(net)) return DRA_EINVAL;
  if (!io->state || !io->q || !io->beta || !io->logits || !io->option || !io->prev_option || !io->action || !io->init ||
      !io->log_pi_a || !io->entropy || !io->reward || !io->mask || !io->bootstrap || !io->eps || !io->grad || !io->out_ret ||
      !io->out_adv || !io->out_beta_adv || !io->out_loss)
    return DRA_EINVAL;
  return dispatch_hidden_gate(net->hidden, net->gate, [&](auto h, auto g) {
    constexpr int H = decltype(h)::value, GATE = decltype(g)::value;
    return launch_one_workgroup<&oc_mlp_update_kernel<H, GATE>>(update_lds_floats(H) * sizeof(float), net, io, stream);
  });
}
