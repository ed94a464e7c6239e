// n-step DQN on pixels (NStepDQN_agent.py:12-67) over a device-resident rollout: the stand-alone Q head of a rollout step (and,
// in "max" mode, the target network's bootstrap) and the update's n-step TD loss with the Q head's backward in one launch.
// The rollout's other launches are the A2C / PPO ones (conv_v2.hip dra_rollout_conv1_qheads, dra_conv_fwd_koc,
// dra_linear_fwd_slabs_one); agents.NStepDQNAgent strings them together.
#include "common.h"
#include "rollout_roles.h"

// ---- the Q head of one rollout step (rollout_roles.h q_head_row_fold_wg): one workgroup of four waves per row
__global__ void __launch_bounds__(256)
q_heads_fold28_kernel(const QHeadArgs h) {
  __shared__ float s_phi[512];
  __shared__ float s_out[68];
  q_head_row_fold_wg<28>(h, blockIdx.x, s_phi, s_out);
}

DRA_API int dra_q_heads_fold28(const float* slabs, const float* fold_bias, const float* w_q, const float* b_q, const uint8_t* explore,
                               const int64_t* random_action, int batch, int n_actions, float* out_q, int64_t* out_action,
                               float* out_phi, float* out_max, void* stream) {
  if (!slabs || !fold_bias || !w_q || batch < 1 || batch > 65536 || n_actions < 1 || n_actions > 64) return DRA_EINVAL;
  if (out_action && (!explore || !random_action)) return DRA_EINVAL;
  if (!out_q && !out_action && !out_phi && !out_max) return DRA_EINVAL;
  QHeadArgs h;
  h.slabs = slabs; h.fold_bias = fold_bias; h.w = w_q; h.b = b_q; h.explore = explore; h.random_action = random_action;
  h.out_phi = out_phi; h.out_q = out_q; h.out_max = out_max; h.out_action = out_action; h.B = batch; h.A = n_actions;
  hipLaunchKernelGGL(q_heads_fold28_kernel, dim3(batch), dim3(256), 0, dra_stream(stream), h);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}

// ---- the update (NStepDQN_agent.py:56-67) behind a rollout of T steps x N environments, R = T N rows, in ONE launch:
//   ret[t][n] = r + (gamma m) ret, backwards from the bootstrap max_a q_target(s_T) (the reference's loop and operation order; the
//     same arithmetic as scan.hip's use_gae = 0 replay), loss = 0.5 mean_r (q[r][a_r] - ret_r)^2, and the gradient of that loss
//     through the Q head: dq_r = (q[r][a_r] - ret_r) / R at the taken action only (d/dq of 0.5 mean(.)^2, what the
//     autograd path hands the head), so
//   workgroups [0, A): dW[a][k] = sum_r [a_r == a] dq_r phi[r][k], db[a] = sum_r [a_r == a] dq_r -- a fixed tree (8 rows, 16 of those
//     sums, then the sums of 128 rows, each level in ascending r), one thread per (a, k): a fixed-order reduction, no atomics, eager runs and
//     graph replays give the same bits
//   workgroups [A, A + ceil(R / 4)): four rows each, dphi[r][k] = dq_r W[a_r][k] [phi[r][k] > 0] (fc4's fused ReLU)
// Every workgroup forms the R returns / differences itself in LDS (R <= 2048: a few hundred loads); workgroup 0 writes ret and
// the loss.  phi: fc4's output [R][512] of the rollout (rows t-major), w: [A][512].
constexpr int kNstepMaxRows = 2048;
constexpr int kNstepRowsPerWg = 4;
constexpr int kNstepSumInner = 8, kNstepSumOuter = 128;
__global__ void __launch_bounds__(256)
nstep_q_loss_bwd_kernel(const float* __restrict__ q, const int64_t* __restrict__ action, const float* __restrict__ reward,
                        const float* __restrict__ mask, const float* __restrict__ bootstrap, float gamma,
                        const float* __restrict__ phi, const float* __restrict__ w, int T, int N, int A, float* __restrict__ out_ret,
                        float* __restrict__ out_loss, float* __restrict__ dw, float* __restrict__ db, float* __restrict__ dphi) {
  __shared__ float s_diff[kNstepMaxRows];
  __shared__ int s_act[kNstepMaxRows];
  const int tid = threadIdx.x;
  const int R = T * N;
  for (int e = tid; e < N; e += 256) {
    float ret = bootstrap[e];
    for (int t = T - 1; t >= 0; --t) {
      const int r = t * N + e;
      ret = __fadd_rn(reward[r], __fmul_rn(__fmul_rn(gamma, mask[r]), ret));
      int64_t a = action[r];
      a = a < 0 ? 0 : (a >= A ? A - 1 : a);          // (actions come from the rollout's head: always in range)
      s_act[r] = (int)a;
      s_diff[r] = __fsub_rn(q[(int64_t)r * A + a], ret);
      if (blockIdx.x == 0) out_ret[r] = ret;
    }
  }
  __syncthreads();
  const float rows_f = (float)R;
  if ((int)blockIdx.x < A) {
    const int a = blockIdx.x;
    if (blockIdx.x == 0 && tid == 0) {
      float s = 0.f;
      for (int r = 0; r < R; ++r) s = __fadd_rn(s, __fmul_rn(s_diff[r], s_diff[r]));
      out_loss[0] = __fmul_rn(0.5f, __fdiv_rn(s, rows_f));
    }
    // a fixed tree of three levels: 8 rows in ascending order, 16 such sums in ascending order (128 rows), then the up to 16
    // sums of 128 rows in ascending order -- at most 40 additions between a term and the sum of 2048 of them.  With all rows on
    // one action db is a mean of differences of both signs, some 400 times smaller than the sum of their magnitudes.
    float acc0 = 0.f, acc1 = 0.f, accb = 0.f;
    for (int ro = 0; ro < R; ro += kNstepSumOuter) {
      float m0 = 0.f, m1 = 0.f, mb = 0.f;
      const int rm_end = min(R, ro + kNstepSumOuter);
      for (int rm = ro; rm < rm_end; rm += kNstepSumInner) {
        float c0 = 0.f, c1 = 0.f, cb = 0.f;
        const int re = min(R, rm + kNstepSumInner);
        for (int r = rm; r < re; ++r) {
          if (s_act[r] != a) continue;
          const float g = __fdiv_rn(s_diff[r], rows_f);
          const float* pr = phi + (int64_t)r * 512;
          c0 = __fadd_rn(c0, __fmul_rn(g, pr[tid]));
          c1 = __fadd_rn(c1, __fmul_rn(g, pr[tid + 256]));
          cb = __fadd_rn(cb, g);
        }
        m0 = __fadd_rn(m0, c0);
        m1 = __fadd_rn(m1, c1);
        mb = __fadd_rn(mb, cb);
      }
      acc0 = __fadd_rn(acc0, m0);
      acc1 = __fadd_rn(acc1, m1);
      accb = __fadd_rn(accb, mb);
    }
    dw[(int64_t)a * 512 + tid] = acc0;
    dw[(int64_t)a * 512 + tid + 256] = acc1;
    if (tid == 0) db[a] = accb;
    return;
  }
  const int r0 = ((int)blockIdx.x - A) * kNstepRowsPerWg;
  for (int i = 0; i < kNstepRowsPerWg; ++i) {
    const int r = r0 + i;
    if (r >= R) break;
    const float g = __fdiv_rn(s_diff[r], rows_f);
    const float* pr = phi + (int64_t)r * 512;
    const float* wr = w + (int64_t)s_act[r] * 512;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = tid + 256 * j;
      dphi[(int64_t)r * 512 + k] = pr[k] > 0.f ? __fmul_rn(g, wr[k]) : 0.f;
    }
  }
}

DRA_API int dra_nstep_q_loss_bwd(const float* q, const int64_t* action, const float* reward, const float* mask, const float* bootstrap,
                                 double gamma, const float* phi, const float* w_q, int t_len, int n_env, int n_actions, float* out_ret,
                                 float* out_loss, float* dw_q, float* db_q, float* dphi, void* stream) {
  if (!q || !action || !reward || !mask || !bootstrap || !phi || !w_q || !out_ret || !out_loss || !dw_q || !db_q || !dphi)
    return DRA_EINVAL;
  if (t_len < 1 || n_env < 1 || (int64_t)t_len * n_env > kNstepMaxRows || n_actions < 1 || n_actions > 64) return DRA_EINVAL;
  const int rows = t_len * n_env;
  const int wgs = n_actions + (rows + kNstepRowsPerWg - 1) / kNstepRowsPerWg;
  hipLaunchKernelGGL(nstep_q_loss_bwd_kernel, dim3(wgs), dim3(256), 0, dra_stream(stream), q, action, reward, mask, bootstrap,
                     (float)gamma, phi, w_q, t_len, n_env, n_actions, out_ret, out_loss, dw_q, db_q, dphi);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}
