// Option-critic on pixels (OptionCritic_agent.py:29-119) over a device-resident rollout: the stand-alone head of a rollout step
// (and, in bootstrap mode, the target network's return of observation T) and the update's three losses with the heads' backward
// in one launch.  The rollout's other launches are the A2C / PPO / n-step ones (conv_v2.hip dra_rollout_conv1_ocheads,
// dra_conv_fwd_koc, dra_linear_fwd_slabs_one); agents.OptionCriticAgent strings them together.
#include "common.h"
#include "rollout_roles.h"

// ---- the head of one rollout step (rollout_roles.h oc_head_row_fold_wg): one workgroup of four waves per row
__global__ void __launch_bounds__(256)
oc_heads_fold28_kernel(const OCHeadArgs h) {
  __shared__ float s_phi[512];
  __shared__ float s_out[2 * 8 + 8 * 18];
  oc_head_row_fold_wg<28>(h, blockIdx.x, s_phi, s_out);
}

DRA_API int dra_oc_heads_fold28(const float* slabs, const float* fold_bias, const float* w_q, const float* b_q, const float* w_beta,
                                const float* b_beta, const float* w_pi, const float* b_pi, const float* uniform, const float* eps,
                                const float* mask, int64_t* prev_option, uint8_t* is_initial, int batch, int n_options,
                                int n_actions, float* out_q, float* out_beta, float* out_logits, int64_t* out_option,
                                int64_t* out_action, float* out_log_pi_a, float* out_entropy, int64_t* out_prev_option,
                                float* out_init, float* out_phi, float* out_boot, void* stream) {
  if (!slabs || !fold_bias || !w_q || !w_beta || !prev_option || batch < 1 || batch > 65536 || n_options < 1 || n_options > 8 ||
      n_actions < 1 || n_actions > 18)
    return DRA_EINVAL;
  if (!out_boot && (!w_pi || !uniform || !eps || !mask || !is_initial)) return DRA_EINVAL;
  OCHeadArgs h;
  h.slabs = slabs; h.fold_bias = fold_bias; h.wq = w_q; h.bq = b_q; h.wb = w_beta; h.bb = b_beta; h.wp = w_pi; h.bp = b_pi;
  h.uniform = uniform; h.eps = eps; h.mask = mask; h.prev_option = prev_option; h.init = is_initial;
  h.out_phi = out_phi; h.out_q = out_q; h.out_beta = out_beta; h.out_logits = out_logits; h.out_lp = out_log_pi_a;
  h.out_ent = out_entropy; h.out_init = out_init; h.out_boot = out_boot; h.out_option = out_option; h.out_action = out_action;
  h.out_prev = out_prev_option; h.B = batch; h.O = n_options; h.A = n_actions;
  hipLaunchKernelGGL(oc_heads_fold28_kernel, dim3(batch), dim3(256), 0, dra_stream(stream), h);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}

// ---- the update (OptionCritic_agent.py:87-117) behind a rollout of T steps x N environments, R = T N rows (t-major), ONE launch.
// Every workgroup first forms the per-row terms in LDS (phase A):
//   ret = r + (gamma m) ret backwards from ret_T (the reference's loop and operation order; threads e < N walk their env's T
//   steps), adv = ret - q[option], v = max q (1 - eps_t) + mean q eps_t, beta_adv = q[prev] - v + termination_regularizer,
//   g = (q[option] - ret) / R (= dq[option] = -adv / R, the intra-option policy's log-likelihood weight), gz = beta (1 - beta)
//   beta_adv (1 - init) / R at prev (dz_beta), and the chosen option's log-sum-exp / entropy (categorical_row_stats).
// Then by role:
//   workgroups [0, 2 O + O A): one output row j of [fc_q | fc_pi | fc_beta]: the ascending list of the rows that reach it
//     (option == o for fc_q / fc_pi, prev == o for fc_beta: a ballot compaction), their gradient values in LDS, then
//     dW[j][k] = sum over the list of g_r phi[r][k], db[j] = sum g_r -- a fixed order, no atomics: eager runs and graph replays
//     give the same bits.  Workgroup 0 also writes ret / adv / beta_adv and the losses (fixed-order tree sums).
//   workgroups [2 O + O A, ... + ceil(R / 4)): four rows each, dphi[r][k] = (g Wq[o][k] + sum_a dlogit_a Wp[o A + a][k] + gz
//     Wb[prev][k]) [phi[r][k] > 0] (fc4's fused ReLU), dlogit = categorical_dlogit(gl = g, ge = -entropy_weight / R).
// loss [4] = (pi_loss + q_loss + beta_loss, q_loss, pi_loss, beta_loss).  phi: [R][512]; wq / wb: [O][512]; wp: [O A][512].
constexpr int kOcMaxRows = 2048;
constexpr int kOcRowsPerWg = 4;
__global__ void __launch_bounds__(256)
oc_loss_bwd_kernel(const float* __restrict__ q, const float* __restrict__ beta, const float* __restrict__ logits,
                   const int64_t* __restrict__ option, const int64_t* __restrict__ action, const int64_t* __restrict__ prev_option,
                   const float* __restrict__ init, const float* __restrict__ log_pi_a, const float* __restrict__ entropy,
                   const float* __restrict__ reward, const float* __restrict__ mask, const float* __restrict__ boot,
                   const float* __restrict__ eps, float gamma, float term_reg, float ent_w, const float* __restrict__ phi,
                   const float* __restrict__ wq, const float* __restrict__ wp, const float* __restrict__ wb, int T, int N, int O,
                   int A, float* __restrict__ out_ret, float* __restrict__ out_adv, float* __restrict__ out_badv,
                   float* __restrict__ out_loss, float* __restrict__ dwq, float* __restrict__ dbq, float* __restrict__ dwp,
                   float* __restrict__ dbp, float* __restrict__ dwb, float* __restrict__ dbb, float* __restrict__ dphi) {
  __shared__ float s_ret[kOcMaxRows];      // phase A: the returns; role 1: the gradient values of the row list
  __shared__ float s_g[kOcMaxRows], s_gz[kOcMaxRows], s_lse[kOcMaxRows], s_ent[kOcMaxRows];
  __shared__ uint8_t s_opt[kOcMaxRows], s_prev[kOcMaxRows], s_act[kOcMaxRows];
  __shared__ int16_t s_list[kOcMaxRows];
  __shared__ float s_red[3][4];
  __shared__ int s_cnt[4];
  __shared__ float s_dl[kOcRowsPerWg][18];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = T * N;
  const float rows_f = (float)R;
  const bool wg0 = blockIdx.x == 0;
  // ---- phase A
  for (int e = tid; e < N; e += 256) {
    float ret = boot[e];
    for (int t = T - 1; t >= 0; --t) {
      const int r = t * N + e;
      ret = __fadd_rn(reward[r], __fmul_rn(__fmul_rn(gamma, mask[r]), ret));
      s_ret[r] = ret;
    }
  }
  __syncthreads();
  float lq = 0.f, lpi = 0.f, lb = 0.f;        // this thread's loss partial sums (ascending rows)
  for (int r = tid; r < R; r += 256) {
    int64_t o = option[r], p = prev_option[r], a = action[r];
    o = o < 0 ? 0 : (o >= O ? O - 1 : o);     // (all three come from the rollout's head: always in range)
    p = p < 0 ? 0 : (p >= O ? O - 1 : p);
    a = a < 0 ? 0 : (a >= A ? A - 1 : a);
    s_opt[r] = (uint8_t)o; s_prev[r] = (uint8_t)p; s_act[r] = (uint8_t)a;
    const float* qr = q + (int64_t)r * O;
    const float ret = s_ret[r], qo = qr[o];
    const float diff = __fsub_rn(qo, ret), adv = __fsub_rn(ret, qo);
    s_g[r] = __fdiv_rn(diff, rows_f);
    float qmax = qr[0], qsum = qr[0];
    for (int j = 1; j < O; ++j) { qmax = fmaxf(qmax, qr[j]); qsum = __fadd_rn(qsum, qr[j]); }
    const float e_t = eps[r / N];
    const float v = __fadd_rn(__fmul_rn(qmax, __fsub_rn(1.f, e_t)), __fmul_rn(__fdiv_rn(qsum, (float)O), e_t));
    const float badv = __fadd_rn(__fsub_rn(qr[p], v), term_reg);
    const float bp = beta[(int64_t)r * O + p], keep = __fsub_rn(1.f, init[r]);
    s_gz[r] = __fdiv_rn(__fmul_rn(__fmul_rn(__fmul_rn(bp, __fsub_rn(1.f, bp)), badv), keep), rows_f);
    float lse, ent;
    categorical_row_stats(logits + (int64_t)r * A, A, &lse, &ent);
    s_lse[r] = lse;
    s_ent[r] = ent;
    if (wg0) {
      out_ret[r] = ret;
      out_adv[r] = adv;
      out_badv[r] = badv;
      lq = __fadd_rn(lq, __fmul_rn(0.5f, __fmul_rn(diff, diff)));
      lpi = __fadd_rn(lpi, __fsub_rn(-__fmul_rn(log_pi_a[r], adv), __fmul_rn(ent_w, entropy[r])));
      lb = __fadd_rn(lb, __fmul_rn(__fmul_rn(bp, badv), keep));
    }
  }
  __syncthreads();
  const int n_w = 2 * O + O * A;
  if (wg0) {                                  // the three means: a wave butterfly, then the four waves in order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      lq += __shfl_xor(lq, off, 64);
      lpi += __shfl_xor(lpi, off, 64);
      lb += __shfl_xor(lb, off, 64);
    }
    if (lane == 0) { s_red[0][wave] = lq; s_red[1][wave] = lpi; s_red[2][wave] = lb; }
    __syncthreads();
    if (tid == 0) {
      float m[3];
      for (int i = 0; i < 3; ++i) m[i] = __fdiv_rn(((s_red[i][0] + s_red[i][1]) + s_red[i][2]) + s_red[i][3], rows_f);
      out_loss[0] = __fadd_rn(__fadd_rn(m[1], m[0]), m[2]);
      out_loss[1] = m[0];
      out_loss[2] = m[1];
      out_loss[3] = m[2];
    }
  }
  if ((int)blockIdx.x < n_w) {
    // ---- role 1: one output row j of the three heads
    const int j = blockIdx.x;
    int head, o, a = 0;                      // head 0: fc_q row o; 1: fc_pi row o A + a; 2: fc_beta row o
    if (j < O) { head = 0; o = j; }
    else if (j < O + O * A) { head = 1; o = (j - O) / A; a = (j - O) % A; }
    else { head = 2; o = j - O - O * A; }
    int n = 0;                               // ascending compaction of the rows that reach output row j
    for (int r0 = 0; r0 < R; r0 += 256) {
      const int r = r0 + tid;
      const bool hit = r < R && (head == 2 ? s_prev[r] : s_opt[r]) == o;
      const uint64_t m = __ballot(hit);
      if (lane == 0) s_cnt[wave] = __popcll(m);
      __syncthreads();
      int off = n;
      for (int w = 0; w < wave; ++w) off += s_cnt[w];
      if (hit) s_list[off + __popcll(m & ((1ull << lane) - 1ull))] = (int16_t)r;
      n += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
      __syncthreads();
    }
    const float ge = -__fdiv_rn(ent_w, rows_f);
    for (int i = tid; i < n; i += 256) {
      const int r = s_list[i];
      float gv;
      if (head == 0) gv = s_g[r];
      else if (head == 2) gv = s_gz[r];
      else gv = categorical_dlogit(logits[(int64_t)r * A + a], s_lse[r], s_ent[r], s_act[r] == a, s_g[r], ge);
      s_ret[i] = gv;
    }
    __syncthreads();
    float acc0 = 0.f, acc1 = 0.f, accb = 0.f;
    int i = 0;
    for (; i + 4 <= n; i += 4) {             // four rows' loads in flight, the sums still in ascending row order
      float x0[4], x1[4], gv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* pr = phi + (int64_t)s_list[i + u] * 512;
        x0[u] = pr[tid];
        x1[u] = pr[tid + 256];
        gv[u] = s_ret[i + u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc0 = __fadd_rn(acc0, __fmul_rn(gv[u], x0[u]));
        acc1 = __fadd_rn(acc1, __fmul_rn(gv[u], x1[u]));
        accb = __fadd_rn(accb, gv[u]);
      }
    }
    for (; i < n; ++i) {
      const float* pr = phi + (int64_t)s_list[i] * 512;
      const float g = s_ret[i];
      acc0 = __fadd_rn(acc0, __fmul_rn(g, pr[tid]));
      acc1 = __fadd_rn(acc1, __fmul_rn(g, pr[tid + 256]));
      accb = __fadd_rn(accb, g);
    }
    float* dw = head == 0 ? dwq + (int64_t)o * 512 : (head == 1 ? dwp + (int64_t)(o * A + a) * 512 : dwb + (int64_t)o * 512);
    dw[tid] = acc0;
    dw[tid + 256] = acc1;
    if (tid == 0) {
      if (head == 0) dbq[o] = accb;
      else if (head == 1) dbp[o * A + a] = accb;
      else dbb[o] = accb;
    }
    return;
  }
  // ---- role 2: the feature gradient of four rows
  const int r0 = ((int)blockIdx.x - n_w) * kOcRowsPerWg;
  const float ge = -__fdiv_rn(ent_w, rows_f);
  for (int i = 0; i < kOcRowsPerWg; ++i) {
    const int r = r0 + i;
    if (r < R && tid < A)
      s_dl[i][tid] = categorical_dlogit(logits[(int64_t)r * A + tid], s_lse[r], s_ent[r], s_act[r] == tid, s_g[r], ge);
  }
  __syncthreads();
  for (int i = 0; i < kOcRowsPerWg; ++i) {
    const int r = r0 + i;
    if (r >= R) break;
    const int o = s_opt[r], p = s_prev[r];
    const float g = s_g[r], gz = s_gz[r];
    const float* pr = phi + (int64_t)r * 512;
    const float* wqr = wq + (int64_t)o * 512;
    const float* wbr = wb + (int64_t)p * 512;
    const float* wpr = wp + (int64_t)o * A * 512;
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
      const int k = tid + 256 * h2;
      float vp = 0.f;
      for (int a = 0; a < A; ++a) vp = __fadd_rn(vp, __fmul_rn(s_dl[i][a], wpr[(int64_t)a * 512 + k]));
      const float v = __fadd_rn(__fadd_rn(__fmul_rn(g, wqr[k]), vp), __fmul_rn(gz, wbr[k]));
      dphi[(int64_t)r * 512 + k] = pr[k] > 0.f ? v : 0.f;
    }
  }
}

DRA_API int dra_oc_loss_bwd(const float* q, const float* beta, const float* logits, const int64_t* option, const int64_t* action,
                            const int64_t* prev_option, const float* init, const float* log_pi_a, const float* entropy,
                            const float* reward, const float* mask, const float* ret_boot, const float* eps, double gamma,
                            double termination_regularizer, double entropy_weight, const float* phi, const float* w_q,
                            const float* w_pi, const float* w_beta, int t_len, int n_env, int n_options, int n_actions,
                            float* out_ret, float* out_adv, float* out_beta_adv, float* out_loss, float* dw_q, float* db_q,
                            float* dw_pi, float* db_pi, float* dw_beta, float* db_beta, float* dphi, void* stream) {
  if (!q || !beta || !logits || !option || !action || !prev_option || !init || !log_pi_a || !entropy || !reward || !mask ||
      !ret_boot || !eps || !phi || !w_q || !w_pi || !w_beta || !out_ret || !out_adv || !out_beta_adv || !out_loss || !dw_q ||
      !db_q || !dw_pi || !db_pi || !dw_beta || !db_beta || !dphi)
    return DRA_EINVAL;
  if (t_len < 1 || n_env < 1 || (int64_t)t_len * n_env > kOcMaxRows || n_options < 1 || n_options > 8 || n_actions < 1 ||
      n_actions > 18)
    return DRA_EINVAL;
  const int rows = t_len * n_env;
  const int wgs = 2 * n_options + n_options * n_actions + (rows + kOcRowsPerWg - 1) / kOcRowsPerWg;
  hipLaunchKernelGGL(oc_loss_bwd_kernel, dim3(wgs), dim3(256), 0, dra_stream(stream), q, beta, logits, option, action, prev_option,
                     init, log_pi_a, entropy, reward, mask, ret_boot, eps, (float)gamma, (float)termination_regularizer,
                     (float)entropy_weight, phi, w_q, w_pi, w_beta, t_len, n_env, n_options, n_actions, out_ret, out_adv,
                     out_beta_adv, out_loss, dw_q, db_q, dw_pi, db_pi, dw_beta, db_beta, dphi);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}
