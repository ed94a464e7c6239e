/* deeprl_amd.h -- C ABI of libdeeprl_amd.so: the MI355X (gfx950) replacement for the
 * rollout -> replay -> update hot path of ShangtongZhang/DeepRL.
 *
 * The reference has no FFI of its own (it is pure Python over ATen); the boundary below is what a
 * binding for this path would call, one group per reference component (file:line into the
 * reference tree).  Conventions:
 *   - plain `extern "C"`, raw pointers + sizes, no torch / C++ types;
 *   - every pointer named *_dev or documented "device" is a DEVICE pointer (HBM), outputs are
 *     CALLER-allocated; handles own only their own HBM;
 *   - the last argument is a hipStream_t (as void*); every call is asynchronous on it, never
 *     synchronises the device, allocates nothing (except *_create) and is hipGraph-capturable;
 *   - return 0 on success, a positive hipError_t or a negative errno-style code otherwise;
 *     nothing throws or aborts across the boundary;
 *   - host RNG (numpy legacy RandomState / python `random`) stays with the caller so that index
 *     streams are the reference's own; only indices / uniforms cross the boundary.
 */
#ifndef DEEPRL_AMD_H
#define DEEPRL_AMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DRA_ACT_NONE 0
#define DRA_ACT_RELU 1
#define DRA_ACT_TANH 2
#define DRA_MAX_Z 4 /* independent (input, weights) sets per batched forward launch */

/* ---- replay ring: deep_rl/component/replay.py:57-149 (UniformReplay storage + construct_transition) */
typedef struct dra_ring dra_ring;
/* replay.py:60-67.  frame_bytes = bytes of ONE stored observation (84*84 for Atari), action_bytes = bytes of one
 * action record (8 for int64). */
int dra_ring_create(dra_ring** out, int64_t capacity, int64_t frame_bytes, int64_t action_bytes, int history,
                    int n_step, double discount);
int dra_ring_shape(dra_ring* ring, int* history, int* n_step);   /* the history_length / n_step it was created with */
int dra_ring_discount(dra_ring* ring, double* discount);           /* ... and the discount of its n-step fold */
int dra_ring_destroy(dra_ring* ring);
int dra_ring_pointers(dra_ring* ring, void** frames, void** actions, void** rewards, void** masks);
/* replay.py:75-90 (feed): write `count` consecutive slots from DEVICE-ACCESSIBLE sources (device or pinned host).
 * NULL action/reward/mask sources take the by-value scalars (count == 1 use). */
int dra_ring_put(dra_ring* ring, int64_t slot0, int64_t count, const void* frame_src, const void* action_src,
                 int64_t action_val, const double* reward_src, double reward_val, const int32_t* mask_src,
                 int32_t mask_val, void* stream);
/* replay.py:75-90 for the `count` <= 8 transitions of ONE agent step of a device-resident actor (DQN_agent.py:103-113: one feed
 * per transition).  The first slot is read from the device word slot0_dev (so that the launch replays from a captured graph) or,
 * when slot0_dev is NULL, is slot0; slots wrap at the capacity.  Frame k lies frame_stride bytes behind frame k - 1 (the newest
 * frame of each [history][frame] stack); actions i64 (action_bytes == 8), rewards f64, masks i32: device arrays of `count`.  A
 * by-value slot outside [0, capacity) or a count outside [1, 8] is refused; a device word outside the ring writes nothing. */
int dra_ring_put_rows(dra_ring* ring, const int64_t* slot0_dev, int64_t slot0, int count, const void* frame_src,
                      int64_t frame_stride, const int64_t* action_src, const double* reward_src, const int32_t* mask_src,
                      void* stream);
/* replay.py:75-90 from pageable HOST memory (staged through the handle's pinned buffer). */
int dra_ring_put_host(dra_ring* ring, int64_t slot, const void* frame_host, const void* action_host, double reward,
                      int32_t mask, void* stream);
/* synthetic transitions: frame k = splitmix64(seed, counter) bytes, action/reward/mask hashed. */
int dra_ring_fill_synthetic(dra_ring* ring, int64_t slot0, int64_t count, int64_t counter0, uint64_t seed,
                            int n_actions, int done_period, void* stream);
/* replay.py:112-140 (construct_transition) for a batch of validated indices idx_dev[batch] (int64, device):
 * out_state / out_next_state [batch][history][frame_bytes], out_action [batch][action_bytes], out_reward f64[batch]
 * (n-step return, fp64, reference association), out_mask i32[batch]; optional f32 copies of reward / mask
 * (what torch_utils.py:20-25 `tensor()` would produce).  Any output may be NULL. */
int dra_ring_gather(dra_ring* ring, const int64_t* idx_dev, int batch, void* out_state, void* out_next_state,
                    void* out_action, double* out_reward, int32_t* out_mask, float* out_reward_f32,
                    float* out_mask_f32, void* stream);
/* the same transition batch with state / next_state as two VIEWS of one block: out_block [batch][history + n_step][frame_bytes]
 * holds every frame of a sample's run once -- state = frames [0, history), next_state = frames [n_step, history + n_step) (the
 * reference stacks the history - n_step shared frames twice, replay.py:126-133; 1.13 instead of 1.81 MB written per DQN minibatch) */
int dra_ring_gather_block(dra_ring* ring, const int64_t* idx_dev, int batch, void* out_block, void* out_action, double* out_reward,
                          int32_t* out_mask, float* out_reward_f32, float* out_mask_f32, void* stream);
/* deep_rl/utils/normalizer.py:58-66 + torch_utils.py:23: out[i] = lut[in[i]], lut = f32(f64(v) * coef). */
int dra_u8_to_f32_lut(const void* in_u8, float* out, int64_t n, const float* lut256_dev, void* stream);
/* ... for n_rows rows of row_elems bytes that are in_row_stride bytes apart (such views); out dense; row_elems % 16 == 0 */
int dra_u8_to_f32_lut_rows(const void* in_u8, float* out, int64_t n_rows, int64_t row_elems, int64_t in_row_stride,
                           const float* lut256_dev, void* stream);

/* ---- sum tree: deep_rl/utils/sum_tree.py:6-66 as driven by replay.py:152-196 (PrioritizedReplay) */
typedef struct dra_sumtree dra_sumtree;
int dra_sumtree_create(dra_sumtree** out, int64_t capacity);            /* sum_tree.py:8-13 */
int dra_sumtree_destroy(dra_sumtree* tree);
int dra_sumtree_pointer(dra_sumtree* tree, void** tree_dev, int64_t* n_nodes);
/* sum_tree.py:54-60 + 16-20 for n (<= 1024) UNIQUE leaves (tree indices, int64 device) and fp64 priorities.
 * ordered != 0 replays the reference's incremental `+= change` walk update by update (slow, bit-exact always);
 * otherwise affected ancestors are recomputed level by level (bit-identical for fp32-valued priorities). */
int dra_sumtree_update(dra_sumtree* tree, const int64_t* leaf_idx_dev, const double* prio_dev, int n, int ordered,
                       void* stream);
int dra_sumtree_set(dra_sumtree* tree, int64_t leaf_idx, double prio, void* stream); /* sum_tree.py:39-51 (add) */
int dra_sumtree_set_from(dra_sumtree* tree, int64_t leaf_idx, const double* prio_dev, void* stream); /* same, *prio_dev */
/* n (<= 64) consecutive adds at write cursor write0, write0+1, ... (mod capacity), all at *prio_dev.  stat_dev = the
 * {max_priority, smallest priority offered} pair dra_sumtree_commit_f32 keeps: inside its exactness bound the adds run
 * level-parallel, outside it (or with stat_dev null) as the reference's n delta walks in order: bit-identical always. */
int dra_sumtree_set_many_from(dra_sumtree* tree, int64_t write0, int n, const double* prio_dev, const double* stat_dev,
                              void* stream);
/* replay.py:193-196 with the new priorities still on the device: leaf_idx_dev[i] <- f64(prio_f32_dev[pos_dev[i]]), i < n
 * (the host picks the pending, first-occurrence entries); stat_dev = {max_priority, smallest priority offered} is kept
 * over all `batch` offered values.  Falls back by itself to the reference's ordered walk when the level-parallel update
 * would not be exact in fp64 (capacity * max / ulp_f32(min) > 2^53), or when force_ordered != 0. */
int dra_sumtree_commit_f32(dra_sumtree* tree, const int64_t* leaf_idx_dev, const int32_t* pos_dev, int n,
                           const float* prio_f32_dev, int batch, double* stat_dev, int force_ordered, void* stream);
#define DRA_PER_CHAIN_MAX 1024
/* The whole of PrioritizedReplay.sample() on the device (round 3), so that the HOST is not between an update's priorities and
 * the next update: ONE kernel body = write-back of the update that just produced its loss vector (as dra_sumtree_commit_f32,
 * incl. its ordered-walk fallback) -> add_n adds at the write cursor at max_priority (as dra_sumtree_set_many_from) ->
 * stratified descent of the NEXT draw (as dra_sumtree_sample).  Every per-step input is read from one PINNED HOST block, so
 * the launch has constant arguments and is captured into the learner's update graph.  The kernel
 *   - gates the commit itself (sum_tree.py:54-60: first occurrence of a leaf in the minibatch wins; every sampled leaf is
 *     pending by construction, the sampled leaves are kept in `dev` from one launch to the next),
 *   - draws its uniforms from python's `random` stream: `rng_words` is a pinned ring of DRA_PER_RNG_WORDS raw Mersenne-Twister
 *     outputs the host generates ahead (random.getrandbits), `dev` keeps the cursor; random.random() = two words
 *     ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53, random.uniform(a, b) = a + (b - a) * random(),
 *   - applies replay.py:122-127's valid_index to every draw, drops the invalid ones and pads with random.choice of what
 *     has been picked so far (replay.py:176-186; _randbelow: k = n.bit_length(), words >> (32 - k) until one is < n),
 *   - writes the minibatch's ring indices to `idx_out_dev` (int64[next_batch], what the next update's kernels read) and
 *     f32(p / total) + the importance exponent to `samp_prob_dev` (f32[next_batch + 1]),
 *   - computes the priorities itself from the update's per-sample loss vector ((|loss| + eps)^alpha, DQN_agent.py:121-123;
 *     also left in prio_out_dev) and the NEXT update's importance weights ((P * B + 1e-6)^-beta / max, :124-126) into
 *     weights_out_dev: the update needs no batch-wide reduction of its own any more,
 *   - and leaves everything the host's (lagging) bookkeeping wants in the pinned block, out_seq last. */
#define DRA_PER_RNG_WORDS 65536
typedef struct dra_per_chain2_io {
  int32_t add_n, batch, next_batch, force_ordered;      /* inputs (batch = next_batch = the launch's `batch` argument) */
  int32_t history, n_step;
  int64_t add_write0;                  /* tree write cursor before the adds */
  int64_t memory_size;                 /* ring slots = leaves */
  int64_t pos_after, size_after;       /* replay.pos / size() after those adds (valid_index of the next draw) */
  uint64_t rng_produced;               /* words the host has generated so far: the cursor must not pass it */
  float beta_next;                     /* importance exponent of the next update (DQN_agent.py:124) */
  int32_t reserved;
  int64_t out_raw_idx[DRA_PER_CHAIN_MAX];   /* outputs: the leaf of every descent, in segment order (all become pending) */
  int64_t out_idx[DRA_PER_CHAIN_MAX];       /* the minibatch's leaves after the validity filter and the padding */
  double out_p[DRA_PER_CHAIN_MAX];          /* their priorities */
  double out_total;
  int32_t out_n_valid;
  int32_t out_flags;                   /* 1: the word ring ran dry, 2: no valid draw at all -- the results are invalid */
  uint64_t out_rng_cursor;             /* words consumed so far */
  uint64_t out_seq;                    /* launches completed, written LAST with system scope */
} dra_per_chain2_io;
/* dev: device state of *dra_sumtree_per_chain2_state_bytes bytes ({cursor, seq, leaves of the current minibatch}). */
int dra_sumtree_per_chain2_state_bytes(int64_t* bytes);
int dra_sumtree_per_chain2_state_set(void* dev_state, uint64_t rng_cursor, uint64_t seq, const int64_t* tree_idx_host, int n);
int dra_sumtree_per_chain2(dra_sumtree* tree, dra_per_chain2_io* io_pinned, const float* loss_vec_dev, float replay_eps,
                           float replay_alpha, float* prio_out_dev, double* stat_dev, void* dev_state,
                           const uint32_t* rng_words_pinned, int64_t* idx_out_dev, float* samp_prob_dev,
                           float* weights_out_dev, int batch, void* stream);
/* replay.py:168-175 + sum_tree.py:23-33,63-66: u_dev[batch] are raw python random.random() draws; lane i samples
 * s = a + (b-a)*u_i on segment i of total/batch and descends; outputs tree index, leaf priority, and the total. */
int dra_sumtree_sample(dra_sumtree* tree, const double* u_dev, int batch, int64_t* out_tree_idx, double* out_p,
                       double* out_total, void* stream);
int dra_sumtree_rebuild(dra_sumtree* tree, void* stream);

/* ---- fused losses (forward + backward) */
/* deep_rl/agent/DQN_agent.py:78-99 (+ PER :120-127).  q, q_next_* [batch][n_actions] f32; action int64[batch] or
 * f32[batch]; reward/mask f32[batch].  sampling_prob NULL = uniform replay.  out_dq = d(reduced loss)/dq.
 * beta < 0 (here and in dra_per_weights): the importance exponent is read from sampling_prob[batch] on the device, so that
 * the launch has no per-update argument and can be replayed from a captured graph. */
int dra_td_loss(const float* q, const float* q_next_target, const float* q_next_online, const void* action,
                int action_is_i64, const float* reward, const float* mask, int batch, int n_actions, float gamma_n,
                const float* sampling_prob, float beta, float replay_eps, float replay_alpha, float* out_loss,
                float* out_dq, float* out_delta, float* out_prio, float* out_weights, void* stream);
/* deep_rl/agent/CategoricalDQN_agent.py:60-89 on LOGITS [batch][n_actions][n_atoms] (softmax folded in). */
int dra_c51_loss(const float* logits, const float* logits_next_target, const float* logits_next_online,
                 const void* action, int action_is_i64, const float* reward, const float* mask, int batch,
                 int n_actions, int n_atoms, float gamma_n, float v_min, float v_max, const float* atoms,
                 float* out_kl, float* out_dlogits, const float* weights, void* stream);
/* deep_rl/agent/QuantileRegressionDQN_agent.py:55-77 + utils/torch_utils.py:47-48; workspace f32[batch*n_q]. */
int dra_qr_loss(const float* theta, const float* theta_next_target, const void* action, int action_is_i64,
                const float* reward, const float* mask, int batch, int n_actions, int n_quantiles, float gamma_n,
                float* workspace, float* out_loss_vec, float* out_loss, float* out_dtheta, void* stream);
/* DQN_agent.py:121-127 applied to any loss vector. */
int dra_per_weights(const float* loss_vec, const float* sampling_prob, int batch, float beta, float replay_eps,
                    float replay_alpha, float* out_prio, float* out_weights, void* stream);
int dra_weighted_mean(const float* x, const float* w, int n, float* out, void* stream);
/* deep_rl/network/network_heads.py:240-255 (CategoricalActorCriticNet: Categorical(logits) -> sample / log_prob / entropy).
 * action_in NULL: actions are sampled by inverse CDF from uniform[batch] into action_out.  n_actions <= 64. */
int dra_categorical_fwd(const float* logits, int batch, int n_actions, const int64_t* action_in, const float* uniform,
                        int64_t* action_out, float* log_pi_a, float* entropy, void* stream);
/* out_dlogits [batch, n_actions] = d(g_log_pi_a . log_pi_a + g_entropy . entropy) / d logits for the given actions (g_* may be
 * NULL = zero).  An action outside [0, n_actions) behaves as the nearest valid one, in dra_categorical_fwd and here alike: the
 * gradient is the derivative of the value the forward returned. */
int dra_categorical_bwd(const float* logits, int batch, int n_actions, const int64_t* action, const float* g_log_pi_a,
                        const float* g_entropy, float* out_dlogits, void* stream);
/* rank-invariant Categorical(logits).sample() for the data-parallel on-policy agents: action[i] = argmax_a
 * (logits[i][a] + Gumbel noise hashed from (seed, *step_dev, lo + i, a)), lo = first GLOBAL environment of this rank; the
 * kernel advances *step_dev (device int64), so the launch replays from a captured rollout graph.  n_actions <= 64. */
int dra_gumbel_sample(const float* logits, int n_local, int n_actions, uint64_t seed, int64_t* step_dev, int64_t lo,
                      int64_t* action_out, void* stream);
/* deep_rl/agent/PPO_agent.py:77-86: out3 = {policy_loss, value_loss, approx_kl}. */
int dra_ppo_loss(const float* log_pi_a, const float* entropy, const float* v, const float* old_log_pi_a,
                 const float* adv, const float* ret, int m, float ratio_clip, float entropy_weight, float* out3,
                 float* g_log_pi_a, float* g_entropy, float* g_v, void* stream);
/* deep_rl/agent/A2C_agent.py:55-62: out4 = {total, policy, value, entropy}. */
int dra_a2c_loss(const float* log_pi_a, const float* entropy, const float* v, const float* adv, const float* ret,
                 int m, float entropy_weight, float value_loss_weight, float* out4, float* g_log_pi_a,
                 float* g_entropy, float* g_v, void* stream);

/* ---- return / advantage recurrences: PPO_agent.py:51-61, A2C_agent.py:43-53, NStepDQN_agent.py:56-60 */
/* reward, mask [t_len][n_env]; value [t_len+1][n_env]; outputs [t_len][n_env]. */
int dra_gae(const float* reward, const float* mask, const float* value, int t_len, int n_env, float gamma, float tau,
            int use_gae, float* out_adv, float* out_ret, void* stream);
int dra_adv_normalize(float* adv, int64_t n, void* stream); /* PPO_agent.py:66 */

/* ---- network contractions: deep_rl/network/network_bodies.py:10-33,50-73 + network_heads.py heads */
/* layer 1..3 of NatureConvBody; nz batched (input, weights) sets per launch. */
int dra_conv_fwd(int layer, int nz, const void* const* x, const float* const* w, const float* const* bias,
                 float* const* y, int batch, int x_is_u8, double u8_coef, int act, void* stream);
int dra_conv_bwd_w(int layer, const float* dy, const void* x, float* dw, float* db, int64_t slab_stride, int ksplit,
                   int batch, int x_is_u8, double u8_coef, void* stream);
int dra_conv_bwd_x(int layer, const float* dy, const float* w, const float* xact, float* dx, int batch, int act,
                   void* stream);
/* KOC weight layout ([K=(c,kh,kw)][OC]; conv_v2.hip): one-round-trip forward, and the matching gradients. */
int dra_conv_fwd_koc(int layer, int nz, const void* const* x, const float* const* wt, const float* const* bias,
                     float* const* y, int batch, int x_is_u8, double u8_coef, int act, void* stream);
/* conv1 of a batch-1 forward whose 4-frame uint8 stack is read straight from the ring (newest slot on device);
 * stack_age_dev (optional, device int32): channel c reads slot newest - min(3 - c, *stack_age_dev) (episode start:
 * the first frame repeated, dra_dqn_step_params.stack_age); null = the last 4 ring frames */
int dra_conv1_fwd_koc_ring(const void* frames, const int64_t* newest_slot_dev, const int32_t* stack_age_dev, int64_t capacity, const float* wt,
                           const float* bias, float* y, double u8_coef, int act, void* stream);
/* same, the slot taken from entry (*seq_dev mod n_entries) of an array of parameter blocks stride_bytes apart;
 * newest_frame (optional, device uint8[84*84]): the newest channel comes from this not-yet-committed observation */
int dra_conv1_fwd_koc_ring_seq(const void* frames, const int64_t* slot_field_dev, const int32_t* stack_age_field_dev, const unsigned* seq_dev, int n_entries,
                               int64_t stride_bytes, int64_t capacity, const void* newest_frame, const float* wt,
                               const float* bias, float* y, double u8_coef, int act, void* stream);
int dra_conv_bwd_w_koc(int layer, const float* dy, const void* x, float* dw, float* db, int64_t slab_stride, int ksplit,
                       int batch, int x_is_u8, double u8_coef, void* stream);
int dra_conv_bwd_x_koc(int layer, const float* dy, const float* wt, const float* xact, float* dx, int batch, int act,
                       void* stream);
int dra_transpose_f32(const float* in, float* out, int rows, int cols, void* stream);
int dra_act_bwd(const float* dy, const float* y, float* dpre, int64_t n, int act, void* stream);
int dra_linear_fwd(int nz, const float* const* x, const float* const* w, const float* const* bias, float* const* y,
                   int batch, int in_features, int out_features, int act, float* workspace, int64_t workspace_floats,
                   void* stream);
/* two heads of different width on the same features in one launch (network_heads.py:241-243: fc_action / fc_critic of the
 * actor-critic nets on phi), one wave per input row; in_features <= 512; same per-output arithmetic as dra_linear_fwd */
int dra_linear_fwd_pair(const float* x, const float* w0, const float* b0, float* y0, int out0, const float* w1, const float* b1,
                        float* y1, int out1, int batch, int in_features, int act, void* stream);
/* a rollout step's policy head (network_heads.py:240-255 under no_grad, action = None) in one launch: logits = x W0^T + b0
 * [batch, n_actions <= 64], v = x w1^T + b1 [batch], then Categorical(logits): action by inverse CDF from uniform[b], log_pi_a,
 * entropy -- dra_linear_fwd_pair + dra_categorical_fwd, bit for bit; out_logits may be NULL */
int dra_policy_heads_sample(const float* x, const float* w0, const float* b0, const float* w1, const float* b1,
                            const float* uniform, int batch, int in_features, int n_actions, int64_t* out_action,
                            float* out_log_pi_a, float* out_entropy, float* out_v, float* out_logits, void* stream);
/* the same head for GIVEN actions (the update's forward): log_pi_a / entropy of action[b], v, and the logits [batch, n_actions] */
int dra_policy_heads_given(const float* x, const float* w0, const float* b0, const float* w1, const float* b1,
                           const int64_t* action, int batch, int in_features, int n_actions, float* out_log_pi_a,
                           float* out_entropy, float* out_v, float* out_logits, void* stream);
/* ... with the finish of the 512-feature layer below in front: features = relu(fold_bias + sum of the n_slabs (8 or 14) K-slice
 * partial sums slabs [n_slabs][batch][512] of dra_linear_fwd_slabs_one, slab 0 first), written to out_phi [batch][512] */
int dra_policy_heads_given_fold(const float* slabs, int n_slabs, const float* fold_bias, const float* w0, const float* b0,
                                const float* w1, const float* b1, const int64_t* action, int batch, int n_actions,
                                float* out_log_pi_a, float* out_entropy, float* out_v, float* out_logits, float* out_phi, void* stream);
/* a rollout step's head with the finish of fc4's 28-slice one-pass forward in front: features = relu(fold_bias + sum of slabs
 * [28][batch][512], slab 0 first); one workgroup per row; then as dra_policy_heads_sample */
int dra_policy_heads_sample_fold28(const float* slabs, const float* fold_bias, const float* w0, const float* b0, const float* w1,
                                   const float* b1, const float* uniform, int batch, int n_actions, int64_t* out_action,
                                   float* out_log_pi_a, float* out_entropy, float* out_v, void* stream);
/* its backward in one launch (dra_categorical_bwd + dra_linear_bwd_pair [+ dra_act_bwd], same sums in the same order): from the
 * gradients of log_pi_a / entropy / v [batch] (any may be NULL = zero) -> dx [batch, in_features] (optional; relu_mask != 0:
 * times [x > 0], x being a fused-ReLU output), dW0 [n_actions, in_features], db0, dW1 [1, in_features], db1; batch <= 8192.
 * An action outside [0, n_actions) behaves as the nearest valid one, as in dra_policy_heads_given: the gradients are those of
 * the log_pi_a the forward returned. */
int dra_policy_heads_bwd(const float* logits, const int64_t* action, const float* g_log_pi_a, const float* g_entropy,
                         const float* g_v, const float* x, const float* w0, const float* w1, float* dx, float* dw0, float* db0,
                         float* dw1, float* db1, int batch, int in_features, int n_actions, int relu_mask, void* stream);
/* backward of that pair in one launch: dx [B, K] (optional) = g0 W0 + g1 W1, dW_h = g_h^T x, db_h = column sums of g_h */
int dra_linear_bwd_pair(const float* g0, const float* g1, const float* x, const float* w0, const float* w1, float* dx, float* dw0,
                        float* db0, float* dw1, float* db1, int batch, int in_features, int out0, int out1, void* stream);
/* both gradients of a 512-output linear layer (fc4 of NatureConvBody) in one launch: dx [batch, in_features] = dy W (times
 * [x > 0] when x is a fused-ReLU output), dW [512, in_features] = dy^T x, db [512] (optional) = column sums of dy; in_features >= 1024 */
int dra_linear_bwd_xw_one512(const float* dy, const float* w, const float* x, int x_is_relu_output, float* dx, float* dw, float* db,
                             int batch, int in_features, void* stream);
/* raw split-K partial sums [nz][ksplit][batch][out] (no bias / activation): the consumer reduces them. */
int dra_linear_fwd_slabs(int nz, const float* const* x, const float* const* w, int batch, int in_features,
                         int out_features, int ksplit, float* slabs, void* stream);
int dra_linear_bwd_w(const float* dy, const float* x, float* dw, float* db, int batch, int in_features,
                     int out_features, void* stream);
int dra_linear_bwd_x(const float* dy, const float* w, const float* xact, float* dx, int batch, int in_features,
                     int out_features, int act, void* stream);

/* ---- Rainbow's noisy layers (csrc/noisy.hip): deep_rl/network/network_utils.py:31-83 (NoisyLinear; :54-62 forward, :73-83
 * reset_noise / transform_noise).  y = act(x W^T + b), W = w_mu + w_sigma * (f(noise_out_weight) f(noise_in)^T),
 * b = b_mu + b_sigma * f(noise_out_bias), f(e) = sign(e) sqrt|e|, straight from the three RAW noise vectors: neither W nor
 * weight_epsilon is written to memory, w_mu and w_sigma are read once per launch.  x [rows <= 1024][in], w_* [out][in], all f32;
 * act in {DRA_ACT_NONE, DRA_ACT_RELU}.  Fixed summation order (no atomics): repeated calls give the same bits.
 * workspace: dra_noisy_workspace_floats(rows, in, out) floats of scratch (split-K / split-N slabs), 16-byte aligned. */
int dra_noisy_workspace_floats(int rows, int in_features, int out_features, int64_t* fwd_floats, int64_t* bwd_floats);
int dra_noisy_linear_fwd(const float* x, const float* w_mu, const float* w_sigma, const float* b_mu, const float* b_sigma,
                         const float* noise_in, const float* noise_out_weight, const float* noise_out_bias, float* y, int rows,
                         int in_features, int out_features, int act, float* workspace, int64_t workspace_floats, void* stream);
/* DQN_agent.py:26-33 for the `rows` <= 8 transitions of one agent step: reset_noise() runs before each forward, the parameters
 * are the same, so row r of x goes through the layer under ITS OWN draw: noise_in [rows][in], noise_out_weight / noise_out_bias
 * [rows][out], rows noise_stride floats apart (0: dense).  One pass over w_mu / w_sigma serves every row; row r has the bits of
 * dra_noisy_linear_fwd(rows = 1) on row r with row r's noise. */
int dra_noisy_linear_fwd_rows(const float* x, const float* w_mu, const float* w_sigma, const float* b_mu, const float* b_sigma,
                              const float* noise_in, const float* noise_out_weight, const float* noise_out_bias,
                              int64_t noise_stride, float* y, int rows, int in_features, int out_features, int act, void* stream);
/* network_heads.py:79-86 + CategoricalDQN_agent.py:21-24 + torch_utils.py:51-58 at epsilon = 0 (DQN_agent.py:34-35), per row:
 * dueling combination (dra_dueling_atoms_fwd's expression), softmax over the atoms, q[a] = sum_z prob[a][z] atoms[z] (ascending z),
 * action = first maximum of q (np.argmax).  value [rows][atoms], advantage [rows][actions][atoms], rows <= 8, actions and atoms
 * <= 64; action i64 [rows]; q [rows][actions] or NULL. */
int dra_rainbow_act_rows(const float* value, const float* advantage, const float* atoms, int rows, int n_actions, int n_atoms,
                         int64_t* action, float* q, void* stream);
/* backward of the same from g = dL/d(pre-activation) [rows][out]: dw_mu = g^T x, dw_sigma = dw_mu * weight_epsilon (one contraction,
 * two stores), db_mu = sum_rows g, db_sigma = db_mu * f(noise_out_bias), dx = g w_mu + ((g * f(noise_out_weight)) w_sigma) *
 * f(noise_in), plus dx_add [rows][in] when given (the input gradient of another head on the same features), times [x_relu > 0]
 * when x_relu (the layer's input, a fused-ReLU output) is given.  dw_* / db_* (pairwise) and dx may be NULL. */
int dra_noisy_linear_bwd(const float* g, const float* x, const float* w_mu, const float* w_sigma, const float* noise_in,
                         const float* noise_out_weight, const float* noise_out_bias, const float* x_relu, const float* dx_add,
                         float* dw_mu, float* dw_sigma, float* db_mu, float* db_sigma, float* dx, int rows, int in_features,
                         int out_features, float* workspace, int64_t workspace_floats, void* stream);
/* network_heads.py:79-86 (RainbowNet.forward): logits[b][a][z] = value[b][z] + (advantage[b][a][z] - mean_a advantage[b][.][z]),
 * and its transpose: d_value = sum_a g, d_advantage = g - d_value / n_actions. */
int dra_dueling_atoms_fwd(const float* value, const float* advantage, int batch, int n_actions, int n_atoms, float* logits,
                          void* stream);
int dra_dueling_atoms_bwd(const float* g_logits, int batch, int n_actions, int n_atoms, float* d_value, float* d_advantage,
                          void* stream);
/* DQN_agent.py:121-127: dra_per_weights with the importance exponent read from *beta_dev (a device word), so that the launch
 * has no per-update argument and replays from a captured graph.  Same arithmetic, same bits. */
int dra_per_weights_dev(const float* loss_vec, const float* sampling_prob, int batch, const float* beta_dev, float replay_eps,
                        float replay_alpha, float* out_prio, float* out_weights, void* stream);

/* ---- Atari frame preprocessing (csrc/preproc.hip): deep_rl/component/envs.py:39-47 -> baselines' MaxAndSkipEnv (max of the
 * last two raw frames) + WarpFrame (cv2 RGB2GRAY, cv2.resize INTER_AREA to 84x84), restated from OpenCV's published
 * algorithms; parity unpinned by the reference (cv2 / baselines are not in the image).  dra_resize_area_tab builds one
 * axis' (source index, weight) table on the HOST (offs has dsize + 1 entries; returns the entry count); the kernel takes
 * device copies of the two tables.  raw: [n_env][2][height][width][3] uint8, out: [n_env][out_h][out_w] uint8. */
int dra_resize_area_tab(int ssize, int dsize, int* si, float* alpha, int* offs, int max_entries);
int dra_atari_preprocess(const uint8_t* raw, int n_env, int height, int width, int out_h, int out_w, const int* x_si,
                         const float* x_alpha, const int* x_off, const int* y_si, const float* y_alpha, const int* y_off,
                         uint8_t* out, void* stream);

/* ---- horizontally fused backward launches + one-pass contractions (csrc/fused.hip, csrc/oneshot.h): the autograd
 * backward behind DQN_agent.py:129 for VanillaNet(NatureConvBody).  `variant` / tuning bits: */
#define DRA_VAR_FUSED_BWD 1      /* learner: a layer's weight- and input-gradient kernels share one launch */
#define DRA_VAR_ONESHOT_DGRAD 2  /* one-pass input gradients (conv2, conv3, fc4) */
#define DRA_VAR_ONESHOT_FWD 4    /* one-pass fc4 forward partial sums */
#define DRA_VAR_ONESHOT_WGRAD 8  /* one-pass conv weight gradients, one slab per (sample, row chunk) */
#define DRA_VAR_PINNED_IDX 16    /* learner: the gather reads minibatch indices from pinned host memory */
#define DRA_VAR_ACTOR_V2 32      /* learner: 5-kernel actor step (ring-direct conv1, GEMV fc4, head + env) */
#define DRA_VAR_ACTOR_PARAMS 64  /* learner: async actor reads a double-buffered parameter copy */
#define DRA_VAR_ACTOR_V3 512     /* learner: the actor graph's first kernel reads its parameter block from a pinned ring
                                    (no copy command in front of the graph) */
#define DRA_VAR_ACTOR_FUSED_HEAD 1024 /* with ACTOR_V3: fc4 + head + env step as one kernel (last-workgroup ticket) */
#define DRA_VAR_GATHER_IN_GRAPH 2048 /* learner, async: a call carries transitions AND indices of the same step; actor
                                    transitions + gather are one graph, the update issued is the previous step's */
#define DRA_VAR_ACTOR_RING 4096  /* learner, async pipelined: the actor's parameter blocks are pushed K steps ahead into a
                                    device ring (dra_dqn_learner_actor_ring_push); no per-step copy command, the last actor
                                    kernel of a step produces the next step's first frame */
#define DRA_VAR_ACTOR_FUSED_CONV1 8192 /* with ACTOR_RING: the head of env step e-1 and the environment step run in front of
                                          conv1 of step e in one launch (4 launches per env step instead of 5) */
#define DRA_VAR_GATHER_ON_UPDATE 16384 /* learner, async pipelined: the gather runs on the UPDATE stream (the actor chain is the
                                       * longer one); the rare step whose minibatch touches the ring slots the next actor
                                       * graph overwrites makes that graph wait for the update (decided on the host) */
#define DRA_VAR_RING_DIRECT 32768  /* learner, async pipelined (with GATHER_ON_UPDATE's host-decided waits): NO gather -- conv1
                                    * (forward of every net, weight gradient) reads the uint8 frames of the sampled
                                    * transitions straight from the replay ring and the head kernel their action / n-step
                                    * reward / mask: one launch, 1.8 MB of writes and 1.8 MB of re-reads less per update */
/* (bit 65536 was DRA_VAR_COOP_OPT, the one-launch fold + norm + optimiser behind a grid barrier: measured 14 % slower than the
 * two launches, removed in round 4; the bit is ignored) */
#define DRA_VAR_IDX_PREFETCH 131072 /* learner (with RING_DIRECT): a step-tagged copy of the minibatch indices goes to the device by
                                    * an unordered async copy when the step is enqueued; conv1 takes an element from there when
                                    * its tag is this update's (no PCIe read in front of its frame loads), else from pinned memory */
#define DRA_VAR_DGRAD_SCATTER 262144 /* dra_conv_bwd_fused, layers 2 / 3, batch >= 256 (with ONESHOT_DGRAD + ONESHOT_WGRAD): the
                                    * input gradient in scatter form -- the contraction runs over the OUTPUT positions (no padded
                                    * (pixel, tap) columns: conv3 1.96x -> 1.14x, conv2 1.58x -> 1.19x issued MFMAs), col2im
                                    * by in-order read-add-write into an LDS image of dX; deterministic (csrc/dgrad_scatter.h).  Below 256 samples
                                    * the bit is ignored.  (Until round 4 this bit was DRA_VAR_WGRAD_ACC, a removed experiment.)
                                    * network_bodies.py:10-33 */
#define DRA_VAR_LATE_FOLD 524288  /* learner (with ONESHOT_WGRAD + FUSED_BWD): no gradient-norm launch -- sums of squares come
                                   * from the kernels that write each gradient, conv3 / conv2 slabs are folded by spare
                                   * workgroups of the NEXT layer's backward launch, conv1's by the first workgroups of the
                                   * optimizer launch (dra_clip_step_late) */
#define DRA_VAR_ACTOR_MEGA 1048576 /* learner (with ACTOR_RING + ACTOR_FUSED_CONV1): an env step of the device actor -- head of the
                                   * previous step, environment step, conv1, conv2, conv3, fc4 -- is ONE launch whose workgroups
                                   * hand their outputs over through arrival counters (4 launches per agent step + the tail
                                   * kernel instead of 17): weights are prefetched before a layer's input exists */
#define DRA_VAR_MEASURE_DGRAD_ONLY 2097152 /* measurement aid (tools/conv_big_bwd.py): dra_conv_bwd_fused launches ONLY the
                                          * input-gradient role -- the weight-gradient slabs are NOT written */
#define DRA_VAR_MEASURE_WGRAD_ONLY 4194304 /* ... ONLY the weight-gradient role -- dx is NOT written */
#define DRA_VAR_DEFER_FC4 8388608 /* learner (RING_DIRECT + LATE_FOLD + ACTOR_MEGA, VanillaNet + RMSprop): the optimizer launch of the
                                   * pipelined graphs steps everything but fc4's weights (95 % of the parameters, 51 of its 54 MB);
                                   * that segment is stepped by rider workgroups in the NEXT update's conv1 / conv2 forward
                                   * launches -- nothing reads it before that graph's fc4 forward, the actor's copy of it is guarded
                                   * by a device word -- with the same arithmetic (same bits).  dra_dqn_learner_flush steps a
                                   * pending segment at once; every entry that reads parameters outside those graphs does so itself */
#define DRA_VAR_ACTOR_PERSIST 16777216 /* learner (with ACTOR_RING + ACTOR_FUSED_CONV1 + ACTOR_MEGA, VanillaNet): ALL env steps of an agent
                                    * step of the device actor as ONE launch of 32 co-resident workgroups -- activations cross
                                    * workgroups as 8-byte {value, tag} words (no launch boundary, no arrival counter), fc4's and the
                                    * convolutions' weights stay in registers / LDS for the whole agent step, conv1's workgroups keep
                                    * their rows of the frame stack in LDS.  Same arithmetic as the multi-launch env step: bit-identical
                                    * actions, action values and ring contents.  Needs >= 32 CUs on the actor's stream
                                    * (dra_dqn_learner_set_actor_cus), else the multi-launch form runs.  DQN_agent.py:24-45 */
#define DRA_VAR_FWD_CHAIN 33554432 /* learner (RING_DIRECT, VanillaNet, two nets, batch 17..32): conv1 + conv2 + conv3 of the update's
                                    * forward pass as ONE launch in dependency order -- a workgroup of layer L + 1 waits (arrival
                                    * counter per (net, sample), weights requested first) for the workgroups of ITS sample in layer L
                                    * instead of for the whole layer and a launch boundary.  Same arithmetic: bit-identical.  Carries
                                    * no riders: DRA_VAR_DEFER_FC4 is off with it.  DQN_agent.py:81-99, network_bodies.py:10-33 */
#define DRA_VAR_BWD_CHAIN 67108864 /* learner (as FWD_CHAIN, with LATE_FOLD): conv3's, conv2's and conv1's backward launches as ONE launch
                                    * in dependency order -- a workgroup of layer L - 1 waits for the input-gradient workgroups of ITS
                                    * sample in layer L, the slab folds for the weight-gradient workgroups of their layer.  Same
                                    * arithmetic: bit-identical gradients.  DQN_agent.py:129-134 */
#define DRA_VAR_FLAG_SYNC 134217728 /* learner (RING_DIRECT + ACTOR_RING + ACTOR_PERSIST + FWD_CHAIN, plain uniform replay): the steady-state
                                    * pipelined step records no event and waits for none.  The update graph's first launch counts
                                    * itself in a device word when it STARTS (= the previous update is complete and written back);
                                    * the actor launch polls that word for the number the host left for it in a pinned ring; the
                                    * host paces itself (three calls ahead) on a pinned count the actor launch publishes.  An event
                                    * record behind a graph replay costs 4.9 us of the update stream, the other stream's wait on it
                                    * 9.4 us more (tools/ubench/graph_gap.hip).  Every other entry point drains both streams first.
                                    * Same launches on the same data: bit-identical.  DQN_agent.py:101-138, BaseAgent.py:108-182 */
#define DRA_VAR_LANE_EAGER 268435456 /* learner (with FLAG_SYNC): in the event-free lane the update is issued as its six plain launches
                                    * instead of one graph replay (a replay costs 6 us before its first kernel, a plain dependent
                                    * launch 1.3 us; the host pays the launches instead).  Same launches: bit-identical */
#define DRA_VAR_TARGET_AHEAD 536870912 /* learner (with FLAG_SYNC + LANE_EAGER + BWD_CHAIN, an ahead stream set): target(next_states) of
                                    * update t + 1 (DQN_agent.py:85-88: conv1-3 + fc4 of the target net, which depend on the target
                                    * parameters and the replay ring only) is issued one call early on its own stream and runs UNDER
                                    * update t; the update's forward chain then carries the online net alone and its head kernel folds
                                    * the target's fc4 partial sums from a stash.  Needs the next minibatch's indices one call early
                                    * (dra_dqn_learner_stage_next_indices); an update without a stash computes its target in line.
                                    * Same kernels on the same data: bit-identical.  DQN_agent.py:114-127 */
#define DRA_VAR_BWD_CHAIN_FC 1073741824 /* learner (with BWD_CHAIN): fc4's and the head's backward (input gradient, fc4 weight gradient,
                                    * head weight gradient) lead the chained backward launch; conv3's roles wait for the
                                    * input-gradient workgroups instead of for a launch boundary.  Same arithmetic: bit-identical
                                    * gradients.  OPT-IN, measured SLOWER on MI355X (92.4 -> 97.5 us per step): a launch's register
                                    * and LDS footprint is the maximum over its roles -- fc4's input gradient (152 + 32 registers,
                                    * 65.7 KB of LDS) takes the whole launch from three workgroups per CU to two.
                                    * DQN_agent.py:129-134 */
#define DRA_VAR_HEAD_CHAIN 65536 /* learner (with FWD_CHAIN, VanillaNet head, uniform replay, batch <= 32): the head launch (fc4 fold, head,
                                    * TD error, dq, dh4) and fc4's + the head's backward launch as ONE launch in dependency order: the
                                    * backward roles request fc4's weights / conv3's activations first, then wait for the head role's
                                    * workgroups on one arrival counter.  Same arithmetic: bit-identical.  DQN_agent.py:85-99,131 */
#define DRA_VAR_CU_PARTITION 256 /* host: actor stream and update stream own disjoint CU sets (dra_stream_create_masked) */
#define DRA_VAR_PIPE_GATHER 128  /* learner, async: gather on the actor stream into a double-buffered minibatch,
                                    body + optimizer as one graph -- no cross-stream wait on either chain */
/* process-wide default variant mask used by learners created afterwards */
int dra_set_tuning(int mask);
int dra_get_tuning(int* mask);
int dra_conv_wgrad_slabs(int layer, int batch, int ksplit, int variant, int* n_slabs);
int dra_conv_bwd_fused(int layer, const float* dy, const void* x, const float* wt, const float* xact, float* dw,
                       float* db, int64_t slab_stride, int ksplit, float* dx, int batch, int x_is_u8, double u8_coef,
                       int act, int variant, void* stream);
int dra_fc_bwd_fused(const float* dq, const float* h4, const float* dh4, const float* x3, const float* w4, float* dwh,
                     float* dbh, float* dw4, float* db4, float* dx3, int batch, int n_actions, int in_features, int act,
                     int variant, void* stream);
int dra_linear_fwd_slabs_one(int nz, const float* const* x, const float* const* w, int batch, int in_features,
                             int out_features, int ksplit, float* slabs, void* stream);

/* ---- clip + optimiser: DQN_agent.py:130-134 with the optimisers of examples.py:67-68,139,204,370,508-509,534 */
int dra_norm_partials(void); /* doubles needed per dra_grad_sqnorm call */
int dra_grad_sqnorm(float* grad, int64_t n, const float* slabs, int n_slabs, int64_t slab_stride, double* partials,
                    void* stream);
/* segmented norm + fold (one launch): each segment of the flat gradient is the fixed-order sum of its own
 * n_slabs split-K slabs (slab s of element i at slabs[s*slab_stride + (i - begin)]); the rest of grad is read as is. */
#define DRA_MAX_FOLD_SEGS 4
typedef struct dra_fold_seg {
  int64_t begin, count;     /* floats, multiples of 4 */
  const float* slabs;       /* 16-byte aligned */
  int64_t slab_stride;      /* floats, multiple of 4 */
  int32_t n_slabs, reserved;
} dra_fold_seg;
int dra_norm_partials_max(void);
int dra_grad_sqnorm_segs(float* grad, int64_t n, const dra_fold_seg* segs, int n_segs, double* partials,
                         int* n_partials, void* stream);
int dra_grad_sqnorm_segs_blocks(int64_t n, const dra_fold_seg* segs, int n_segs, int* blocks); /* its workgroups = partials (host only) */
/* the late-fold form (DRA_VAR_LATE_FOLD): every tensor's sum of squares was left in partials[0, n_prior) by the kernels
 * that produced its gradient, except ONE segment (starting at element 0, n_slabs <= 256: conv1, whose weight gradient is the
 * last kernel of the backward) that is still in slabs.  The launch's first dra_clip_step_late_blocks() (<= 256) workgroups
 * fold it and publish their sums of squares into partials[n_prior ...], which must hold -1.0 at launch: the value IS the
 * arrival flag.  Every workgroup loads its operands and the earlier partials, waits for those slots to turn non-negative
 * (bounded: timeout_flag as above), reduces all partials in the fixed order and applies the step.  No gradient-norm launch,
 * no ticket counter. */
int dra_clip_step_late_blocks(const dra_fold_seg* seg, int* fold_blocks);
int dra_clip_step_late(float* param, float* grad, float* state1, float* state2, int64_t n, const dra_fold_seg* seg,
                       double* partials, int n_prior, int* timeout_flag, int optimizer, float max_norm, const float* hyper,
                       int centered, const int64_t* step_dev, float* out_norm, float* param_copy, void* stream);
int dra_rmsprop_step(float* param, const float* grad, float* square_avg, float* grad_avg, int64_t n,
                     const double* partials, int n_partials, float max_norm, float lr, float alpha, float eps,
                     int centered, float* out_norm, void* stream);
int dra_rmsprop_step_copy(float* param, const float* grad, float* square_avg, float* grad_avg, int64_t n,
                          const double* partials, int n_partials, float max_norm, float lr, float alpha, float eps,
                          int centered, float* out_norm, float* param_copy, void* stream);
int dra_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  const double* partials, int n_partials, float max_norm, float lr, float beta1, float beta2, float eps,
                  int64_t step, float* out_norm, void* stream);
/* graph-replayable Adam: the step-dependent scalars {lr/(1-b1^t), 1/sqrt(1-b2^t)} (dra_adam_hyper, host) are read
 * from device memory, every kernel argument is constant across steps */
int dra_adam_hyper(float lr, float beta1, float beta2, int64_t step, float* out2);
int dra_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                      const double* partials, int n_partials, float max_norm, float beta1, float beta2, float eps,
                      const float* hyper_dev, float* out_norm, void* stream);
/* Adam whose 1-based step count is read from DEVICE memory (a learner graph bumps it), with an optional mirror of the
 * updated parameters (the async actor's copy) */
int dra_adam_step_counter(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                          const double* partials, int n_partials, float max_norm, float lr, float beta1, float beta2,
                          float eps, const int64_t* step_dev, float* out_norm, float* param_copy, void* stream);
int dra_copy_f32(float* dst, const float* src, int64_t n, void* stream); /* DQN_agent.py:136-138 */
/* Seed lanes (seed_batch.py: n_lanes independent agents of one configuration in the same launches; 1 <= n_lanes <= 64).  A lane
 * table is an array of n_lanes structs that the HOST and the DEVICE both read at the address passed: pinned host memory that the
 * device maps (hipHostMalloc, torch's pin_memory()).  The entry checks every lane on the host before it launches anything;
 * workgroup (x, lane) reads its struct with scalar loads.  Lanes never wait for each other.
 * dra_clip_rmsprop_step_lanes: per lane, dra_grad_sqnorm's partial sums, the clip coefficient and dra_rmsprop_step's update (centred or
 * not) over the lane's flat buffers of n floats (4 <= n <= 65536, equal in every lane, 16-byte aligned) in ONE launch -- the same
 * partition over dra_norm_partials() blocks folded in the same order, so a lane's parameters, running averages and *out_norm carry
 * the bits of the two single launches on that lane.  max_norm <= 0: no clipping, out_norm is not written.
 * dra_copy_f32_lanes: dst[i] = src[i], i < n, per lane (the target sync of every lane). */
typedef struct dra_optim_lane {
  float* param;          /* [n] (in/out) */
  const float* grad;     /* [n] */
  float* square_avg;     /* [n] (in/out) */
  float* grad_avg;       /* [n] (in/out; centred only) */
  float* out_norm;       /* [1]: the lane's gradient norm before clipping */
  int64_t n;
} dra_optim_lane;
typedef struct dra_copy_lane {
  float* dst;
  const float* src;
  int64_t n;
} dra_copy_lane;
int dra_clip_rmsprop_step_lanes(const dra_optim_lane* lanes, int n_lanes, float max_norm, float lr, float alpha, float eps,
                                int centered, void* stream);
int dra_copy_f32_lanes(const dra_copy_lane* lanes, int n_lanes, void* stream);
/* polyak averaging of the target network (DDPG_agent.py:26-30, TD3_agent.py:28-32) over the two networks' flat parameter
 * buffers (16-byte aligned): target[i] = target[i] * keep + src[i] * mix with keep = f32(1 - mix); each product is rounded
 * before the add, as the reference's `target_param * (1.0 - mix) + param * mix` is.  One launch. */
int dra_soft_update(float* target, const float* src, int64_t n, float keep, float mix, void* stream);

/* ---- minibatch rows of an on-policy rollout (PPO_agent.py:77-80: entries[batch_indices] over state / action / log_pi_a / ret /
 * advantage): dst[q][r] = src[q][idx[r]] for n_fields <= DRA_GATHER_MAX_FIELDS row-major device arrays of row_bytes[q] bytes per
 * row, one launch for all of them; idx_dev int64 [n_rows] (negative = from the end, as torch indexes), n_src_rows rows per source */
#define DRA_GATHER_MAX_FIELDS 8
int dra_gather_rows(int n_fields, const void* const* src, void* const* dst, const int64_t* row_bytes, const int64_t* idx_dev,
                    int n_rows, int64_t n_src_rows, void* stream);

/* ---- device-resident synthetic vector environment (on-policy agents; A2C_agent.py:26-34, PPO_agent.py:33-47): the uint8
 * [n_env][history][84*84] observations of one rollout step from per-environment frame counters / episode ages / stream
 * seeds (device arrays of n_env).  Frames are the counter-hash frames of dra_ring_fill_synthetic. */
int dra_synth_stacks(const int64_t* counter_dev, const int32_t* age_dev, const int64_t* seed_dev, int n_env, int history,
                     void* out_u8, void* stream);

/* ---- an A2C / PPO rollout step over NatureConvBody at 8-32 device-resident environments as four launches (agents._PixelRollout;
 * A2C_agent.py:26-34 / PPO_agent.py:33-47 under no_grad): [conv1 of step t | the policy head of step t-1], conv2, conv3
 * (dra_conv_fwd_koc), fc4 (dra_linear_fwd).  Same arithmetic as the separate launches, bit for bit. */
/* conv1 (+ ReLU) of uint8 frames [batch][4][84][84] -> y1 [batch][32][20][20]; and, when phi_prev != NULL, the policy head of the
 * previous step (workgroups of their own in the same launch: the observations do not depend on the previous step's actions):
 * fold_bias == NULL: dra_policy_heads_sample of the features phi_prev [batch][512]; fold_bias != NULL: phi_prev is the
 * [28][batch][512] K-slice partial sums of fc4 (dra_linear_fwd_slabs_one, ksplit 28) and the head folds them first
 * (dra_policy_heads_sample_fold28) */
int dra_rollout_conv1_heads(const void* frames_u8, const float* wt1, const float* b1, float* y1, int batch, double u8_coef,
                            const float* phi_prev, const float* fold_bias, const float* w_a, const float* b_a, const float* w_v,
                            const float* b_v, const float* uniform, int n_actions, int64_t* out_action, float* out_log_pi_a,
                            float* out_entropy, float* out_v, void* stream);
/* the same launch; out_phi != NULL (needs fold_bias): the head's workgroups also store the previous step's folded features
 * relu(sum of the 28 slices + bias) [batch][512] -- fc4's forward output, kept for an A2C update that backpropagates through the
 * rollout's own activations (A2C_agent.py:29-64) */
int dra_rollout_conv1_heads_phi(const void* frames_u8, const float* wt1, const float* b1, float* y1, int batch, double u8_coef,
                                const float* phi_prev, const float* fold_bias, const float* w_a, const float* b_a, const float* w_v,
                                const float* b_v, const float* uniform, int n_actions, int64_t* out_action, float* out_log_pi_a,
                                float* out_entropy, float* out_v, float* out_phi, void* stream);

/* ---- n-step DQN on pixels over a device-resident rollout (NStepDQN_agent.py:12-67; agents.NStepDQNAgent): each rollout step is
 * the four launches above with a Q head in place of the policy head, exploration planned on the host in the reference's draw
 * order (epsilon_greedy, torch_utils.py:51-59: randint(A, size=N), then rand(N); explore = dice < epsilon), then the target
 * network's forward of the last observation, its max head, and the update's loss + Q-head backward in one launch. */
/* conv1 (+ ReLU) of uint8 frames [batch][4][84][84] -> y1, and, when slabs_prev != NULL, the Q head of the previous step in the
 * same launch (NStepDQN_agent.py:33-36): phi = relu(fold_bias + sum of fc4's 28 K-slice partial sums slabs_prev [28][batch][512],
 * slab 0 first -- the A2C head's fold, bit for bit) -> out_phi [batch][512] (optional), q = phi W^T + b [batch][n_actions <= 64]
 * -> out_q (optional), action = explore[b] ? random_action[b] : the first index of the row's maximum (np.argmax) -> out_action */
int dra_rollout_conv1_qheads(const void* frames_u8, const float* wt1, const float* b1, float* y1, int batch, double u8_coef,
                             const float* slabs_prev, const float* fold_bias, const float* w_q, const float* b_q,
                             const uint8_t* explore, const int64_t* random_action, int n_actions, float* out_q,
                             int64_t* out_action, float* out_phi, void* stream);
/* the same Q head on its own (the last step of a rollout), one workgroup per row; every output optional: out_q, out_action (needs
 * explore / random_action), out_phi, and out_max [batch] = max_a q -- the "max" mode that bootstraps from the target network
 * (NStepDQN_agent.py:56-57) */
int dra_q_heads_fold28(const float* slabs, const float* fold_bias, const float* w_q, const float* b_q, const uint8_t* explore,
                       const int64_t* random_action, int batch, int n_actions, float* out_q, int64_t* out_action, float* out_phi,
                       float* out_max, void* stream);
/* the update of one rollout (NStepDQN_agent.py:56-67) in one launch over R = t_len x n_env <= 2048 rows (t-major): ret [t_len][n_env]
 * by the reference's recurrence ret = r + gamma m ret backwards from bootstrap [n_env]; out_loss [1] = 0.5 mean (q[r][a_r] - ret_r)^2
 * (q [R][n_actions], action i64 [R]); the gradient of that loss through the Q head on the rollout's features phi [R][512]:
 * dw_q [n_actions][512], db_q [n_actions] (fixed-order sums over the rows, no atomics) and dphi [R][512] times [phi > 0] (fc4's
 * ReLU) for fc4's backward */
int dra_nstep_q_loss_bwd(const float* q, const int64_t* action, const float* reward, const float* mask, const float* bootstrap,
                         double gamma, const float* phi, const float* w_q, int t_len, int n_env, int n_actions, float* out_ret,
                         float* out_loss, float* dw_q, float* db_q, float* dphi, void* stream);

/* ---- option-critic on pixels over a device-resident rollout (OptionCritic_agent.py:29-119, network_heads.py:105-127;
 * agents.OptionCriticAgent): each rollout step is the four launches above with the option-critic head in place of the policy head
 * (q [O], beta = sigmoid(z_beta) [O], the O x A intra-option logits, fc_pi row o*A + a = action a of option o), the option and
 * action chosen on the device by inverse CDF from given uniforms [batch][3] (fresh option, continued option, action: the reference
 * draws them with Categorical(...).sample()), then the target network's forward of the last observation, its bootstrap head, and
 * the update's three losses + the heads' backward in one launch.  O <= 8 options, A <= 18 actions. */
/* conv1 (+ ReLU) of uint8 frames [batch][4][84][84] -> y1, and, when slabs_prev != NULL, the option-critic head of the previous
 * step in the same launch (OptionCritic_agent.py:29-63): phi = relu(fold_bias + sum of fc4's 28 K-slice partial sums slabs_prev
 * [28][batch][512], slab 0 first: the A2C head's fold, bit for bit) -> out_phi; q -> out_q [batch][O], beta -> out_beta [batch][O];
 * sample_option (:29-49) with eps [1] (this step's option epsilon): option = is_initial ? invCDF(pi_opt, u0) : invCDF(pi_hat, u1),
 * each row divided by its sum first as Categorical(probs=) does -> out_option; Categorical of the chosen option's logits (-> out_logits [batch][A]) with u2 -> out_action, out_log_pi_a,
 * out_entropy.  The carried state is read and replaced in place: prev_option [batch] <- option, is_initial [batch] (u8) <-
 * (mask [batch] == 0); out_prev_option / out_init record what this step read.  The per-row outputs are optional. */
int dra_rollout_conv1_ocheads(const void* frames_u8, const float* wt1, const float* b1, float* y1, int batch, double u8_coef,
                              const float* slabs_prev, const float* fold_bias, const float* w_q, const float* b_q,
                              const float* w_beta, const float* b_beta, const float* w_pi, const float* b_pi,
                              const float* uniform, const float* eps, const float* mask, int64_t* prev_option,
                              uint8_t* is_initial, int n_options, int n_actions, float* out_q, float* out_beta,
                              float* out_logits, int64_t* out_option, int64_t* out_action, float* out_log_pi_a,
                              float* out_entropy, int64_t* out_prev_option, float* out_init, float* out_phi, void* stream);
/* the same head on its own (the last step of a rollout), one workgroup per row.  out_boot != NULL selects the bootstrap mode of the
 * target network over observation T (OptionCritic_agent.py:87-93): out_boot [batch] = (1 - beta[prev]) q[prev] + beta[prev] max q,
 * prev = prev_option[b] (left as it is); only w_q / w_beta are read then (w_pi, uniform, eps, mask, is_initial may be NULL) */
int dra_oc_heads_fold28(const float* slabs, const float* fold_bias, const float* w_q, const float* b_q, const float* w_beta,
                        const float* b_beta, const float* w_pi, const float* b_pi, const float* uniform, const float* eps,
                        const float* mask, int64_t* prev_option, uint8_t* is_initial, int batch, int n_options, int n_actions,
                        float* out_q, float* out_beta, float* out_logits, int64_t* out_option, int64_t* out_action,
                        float* out_log_pi_a, float* out_entropy, int64_t* out_prev_option, float* out_init, float* out_phi,
                        float* out_boot, void* stream);
/* the update of one rollout (OptionCritic_agent.py:95-117) in one launch over R = t_len x n_env <= 2048 rows (t-major): ret by
 * ret = r + gamma m ret backwards from ret_boot [n_env], adv = ret - q[option], beta_adv = q[prev] - (max q (1 - eps_t) + mean q
 * eps_t) + termination_regularizer (eps [t_len]); out_loss [4] = (pi_loss + q_loss + beta_loss, q_loss, pi_loss, beta_loss); the
 * gradient of that sum through the three heads on the rollout's features phi [R][512]: dw_q / db_q [O][512] / [O], dw_pi / db_pi
 * [O*A][512] / [O*A], dw_beta / db_beta (fixed-order sums over the rows, no atomics) and dphi [R][512] times [phi > 0] (fc4's
 * ReLU) for fc4's backward.  q / beta [R][O], logits [R][A] (the chosen option's), option / action / prev_option i64 [R], init /
 * log_pi_a / entropy / reward / mask f32 [R] */
int dra_oc_loss_bwd(const float* q, const float* beta, const float* logits, const int64_t* option, const int64_t* action,
                    const int64_t* prev_option, const float* init, const float* log_pi_a, const float* entropy, const float* reward,
                    const float* mask, const float* ret_boot, const float* eps, double gamma, double termination_regularizer,
                    double entropy_weight, const float* phi, const float* w_q, const float* w_pi, const float* w_beta, int t_len,
                    int n_env, int n_options, int n_actions, float* out_ret, float* out_adv, float* out_beta_adv, float* out_loss,
                    float* dw_q, float* db_q, float* dw_pi, float* db_pi, float* dw_beta, float* db_beta, float* dphi,
                    void* stream);

/* ---- fused DQN learner + device-resident actor: DQN_agent.py:24-45 (actor step), :114-138 (update) for
 * VanillaNet(NatureConvBody).  All five flat buffers are caller-owned f32[n_params] with the tensor order
 * conv1.w, conv1.b, conv2.w, conv2.b, conv3.w, conv3.b, fc4.w, fc4.b, head.w, head.b at `offset[]` (16-byte
 * aligned); [0, conv_end) is the conv segment whose split-K slabs are folded in the norm pass. */
typedef struct dra_dqn_config {
  int32_t batch, n_actions, double_q, ksplit, centered, env_done_period;
  float gamma_n, gradient_clip, lr, alpha, eps, replay_eps, replay_alpha;
  int32_t variant;          /* DRA_VAR_* mask, or < 0 = the process default (dra_set_tuning) */
  double u8_coef;
  int64_t n_params, conv_end, ring_capacity;
  uint64_t env_seed;        /* synthetic frame source (dra_ring_fill_synthetic stream) used by the device actor */
  int64_t offset[10];
  /* head on top of NatureConvBody's 512 features (network_heads.py): DRA_HEAD_VANILLA = VanillaNet (n_actions outputs,
   * MSE TD loss, DQN_agent.py:81-99); DRA_HEAD_CATEGORICAL = CategoricalNet (n_actions x n_atoms logits over
   * linspace(v_min, v_max, n_atoms), CategoricalDQN_agent.py:60-89); DRA_HEAD_QUANTILE = QuantileNet (n_actions x n_atoms
   * quantiles, QuantileRegressionDQN_agent.py:55-77).  head.w is [n_actions * n_atoms][512], action-major. */
  int32_t head_kind, n_atoms;
  float v_min, v_max;
  /* DRA_OPT_RMSPROP (lr, alpha, eps, centered above) or DRA_OPT_ADAM (lr, beta1, beta2, eps; state1 = exp_avg,
   * state2 = exp_avg_sq; examples.py:139,204) */
  int32_t optimizer;
  float beta1, beta2;
  int32_t reserved;
} dra_dqn_config;
#define DRA_HEAD_VANILLA 0
#define DRA_HEAD_CATEGORICAL 1
#define DRA_HEAD_QUANTILE 2
#define DRA_OPT_RMSPROP 0
#define DRA_OPT_ADAM 1
/* per-agent-step arguments: the device actor's kernels read them from a device copy, so the 4 env steps of a
 * DQN agent step replay as one captured graph.  All randomness is drawn by the HOST in the reference's order
 * (torch_utils.py:51-58: randint(A) then rand()), so the np.random stream is the reference's. */
typedef struct dra_dqn_step_params {
  int64_t slot[8];           /* ring slot of each env transition (frame / action / reward / mask live there) */
  int64_t counter[8];        /* >= 0: synthesise frame `counter` (+ hashed reward / mask) into the slot; < 0: frame already there */
  int64_t rcounter[8];       /* counter whose hashes give the reward / mask stored WITH the slot: the transition that leaves
                                this observation (envs.py:140-141: the counter of the NEXT frame); = counter for a plain stream */
  int32_t random_action[8];  /* np.random.randint(A) drawn by the host */
  int32_t store_action[8];   /* write the chosen action into the slot's action record */
  float dice[8];             /* np.random.rand() drawn by the host */
  float epsilon[8];
  int32_t stack_age[8];      /* observations of the same episode before this one, capped at history-1: channel c of the
                                actor's frame stack is ring slot  slot - min(history-1-c, stack_age)  (after a reset the
                                first frame is repeated, envs.py FrameStack.reset); history-1 = plain "last 4 ring frames" */
  int32_t n_env, reserved;
  int64_t idx[1024];         /* minibatch indices of this step's update (first `batch` used) */
} dra_dqn_step_params;
typedef struct dra_dqn_learner dra_dqn_learner;
int dra_dqn_learner_create(dra_dqn_learner** out, dra_ring* ring, const dra_dqn_config* cfg, float* params,
                           float* target, float* grad, float* state1, float* state2);
int dra_dqn_learner_destroy(dra_dqn_learner* learner);
int dra_dqn_learner_buffers(dra_dqn_learner* learner, void** idx, void** sampling_prob, void** loss, void** norm,
                            void** q, void** delta, void** prio, void** actor_q);
/* one gradient update on the int64[batch] indices in the learner's idx buffer; use_graph replays a captured
 * hipGraph (stream must not be the NULL stream); per != 0 adds the PER branch (DQN_agent.py:120-127). */
int dra_dqn_learner_update(dra_dqn_learner* learner, int use_graph, int per, float beta, void* stream);
/* PER for the in-order dra_dqn_learner_step (stream_actor == NULL): importance weights from the learner's sampling_prob
 * buffer with exponent beta, new priorities into its prio buffer (DQN_agent.py:120-127) */
int dra_dqn_learner_set_per(dra_dqn_learner* learner, int per, float beta);
/* PER: sampling probabilities (host f64[batch], converted to f32) + importance exponent -> the learner's sampling_prob
 * buffer on `stream`, through the learner's own pinned staging (DQN_agent.py:120-127's tensor(sampling_prob)) */
int dra_dqn_learner_upload_sampling_prob(dra_dqn_learner* learner, const double* prob_host, int n, float beta, void* stream);
/* minibatch indices (host int64[batch], replay.py:92-103's sampled_indices) -> the learner's idx buffer on `stream`, through
 * the learner's own pinned staging (n must equal the learner's batch) */
int dra_dqn_learner_upload_indices(dra_dqn_learner* learner, const int64_t* idx_host, int n, void* stream);
/* DRA_VAR_RING_DIRECT: also gather the minibatch into the learner's buffers (dra_dqn_learner_last_minibatch) -- for
 * checkers; the update itself keeps reading the ring */
int dra_dqn_learner_keep_minibatch(dra_dqn_learner* learner, int keep);
/* PER in the pipelined step: the update is issued as [forward passes + loss] [backward + optimizer]; `stream` waits for the
 * first half of the update issued last, i.e. until its TD errors / new priorities exist (the write-back to the sum tree and
 * the next prioritized draw then run under the backward pass) */
int dra_dqn_learner_wait_loss(dra_dqn_learner* learner, void* stream);
/* measurement aid: one eager update with a HIP event in front of every kernel group; out_ms[k] = milliseconds of group k
 * (dra_dqn_learner_kernel_count groups, names from _kernel_name).  With n_out > count, out_ms[count] = the same event pair
 * with NOTHING in between (the bracket's own cost, to be subtracted).  Synchronises. */
int dra_dqn_learner_profile(dra_dqn_learner* learner, float* out_ms, int n_out, void* stream);
/* how many compute units the stream the actor launches are issued on may use (a CU-masked stream: DRA_VAR_CU_PARTITION; 0 = the
 * whole device, the default).  DRA_VAR_ACTOR_PERSIST's launch needs 32 co-resident workgroups of one per CU: with fewer CUs the
 * learner keeps the multi-launch env step.  Call before the first step (the choice is baked into the captured actor graphs). */
int dra_dqn_learner_set_actor_cus(dra_dqn_learner* learner, int n_cus);
/* DRA_VAR_DEFER_FC4: step a pending fc4 segment of the optimizer step now, on `stream` (ordered behind the update that left it).
 * Call before reading parameters / optimizer state / actor copies from outside the library (a synchronise alone does not
 * complete the step); a no-op when nothing is pending.  DQN_agent.py:133 (optimizer.step() is ONE call in the reference). */
int dra_dqn_learner_flush(dra_dqn_learner* learner, void* stream);
/* test aid: the rider code that steps a deferred fc4 segment (RMSprop, csrc/common.h fc4_rider_run) ALONE, as one launch on the
 * caller's flat f32 buffers: elements [4 * begin4, 4 * (begin4 + count4)) of p / s1 / (centered) s2 are stepped with gradient g and
 * the clip coefficient *coef, and the new parameters also go to p_copy (may be NULL) -- if *pending (device int) is non-zero,
 * otherwise nothing is written.  write_through != 0: the form the chained forward launch carries (DRA_VAR_FWD_CHAIN: the stores
 * are written through), 0: the plain form of dra_dqn_learner_flush; same bits.  Bases 16-byte aligned and 4 * (begin4 + count4)
 * < 2^29, else DRA_EINVAL before anything is launched.  DQN_agent.py:133 */
int dra_fc4_rider_test(float* p, const float* g, float* s1, float* s2, float* p_copy, int64_t begin4, int64_t count4,
                       const float* coef, const int* pending, float lr, float alpha, float eps, int centered, int write_through,
                       void* stream);
/* measurement aid: kernel group `kernel` (index as in _kernel_name) of the update ALONE, `reps` dependent launches in ONE
 * captured graph between two events: out_us[0] = microseconds per launch (kernel + one in-graph launch boundary), out_us[1] =
 * the same for an empty kernel (the boundary alone).  Their difference is the kernel's own duration -- the quantity rocprofv3
 * reports -- measured live.  Runs on the workspaces of the last update; refuses the optimizer group.  Synchronises. */
int dra_dqn_learner_kernel_replay(dra_dqn_learner* learner, int kernel, int reps, float* out_us, void* stream);
/* measurement aid: the chained launches the timed pipeline runs under DRA_VAR_FWD_CHAIN / DRA_VAR_BWD_CHAIN, ALONE -- which = 0:
 * conv1 + conv2 + conv3 forward of both nets (network_bodies.py:10-33, online(states) and target(next_states) of
 * DQN_agent.py:114-127); which = 1: conv3 / conv2 / conv1 backward + the two slab folds (DQN_agent.py:131).  `reps` x [the launch,
 * a one-thread launch advancing the chains' epoch word as the update's head kernel does] in ONE captured graph between two
 * events: out_us[0] = microseconds per repetition, out_us[1] = the same with an empty kernel in the launch's place; the
 * difference is the chained kernel's own duration (rocprofv3's figure for it, less the deferred fc4 optimizer segment's riders:
 * a replay never steps parameters, a pending segment is flushed first).  Runs on the workspaces of the last update.  Synchronises. */
int dra_dqn_learner_chain_replay(dra_dqn_learner* learner, int which, int reps, float* out_us, void* stream);
/* test aid: the chained launches hand data between workgroups through 32-bit arrival counters that are never reset (a wait is for
 * epoch x arrivals-per-epoch arrivals, compared modulo 2^32).  Puts this learner's chains where they stand after `epoch` (< 2^32)
 * updates: synchronises (pending fc4 segment flushed, event-free lane left), sets the epoch word of the update's chains and of
 * the target-ahead chains, and every arrival counter to (unsigned)(epoch x its arrivals per epoch).  arrivals[0..8) (n_arrivals >=
 * 8) = arrivals per epoch on one counter of each class, 0 where this learner's launches do not use the class: [0] forward conv1 ->
 * conv2, [1] forward conv2 -> conv3, [2] backward conv3 / [3] conv2 input gradient (per sample), [4] conv3 / [5] conv2 weight
 * gradient, [6] fc4 input gradient (DRA_VAR_BWD_CHAIN_FC), [7] 1 = target-ahead chains set too.  Changes no numerics.  DRA_EINVAL
 * on a learner without chained launches (tests/test_gpu_chain_counter_wrap.py). */
int dra_dqn_learner_chain_set_epoch(dra_dqn_learner* learner, uint64_t epoch, int64_t* arrivals, int n_arrivals, void* stream);
/* the minibatch the most recently issued update consumed (device pointers into the learner's buffers: u8 states /
 * next states [B][4][84][84], int64 actions [B], f32 rewards / masks [B]); for checkers, after a synchronise */
int dra_dqn_learner_last_minibatch(dra_dqn_learner* learner, void** state, void** next_state, void** action, void** reward,
                                   void** mask);
int dra_dqn_learner_kernel_name(int k, char* out, int n);
int dra_dqn_learner_kernel_count(void);
int dra_dqn_learner_sync_target(dra_dqn_learner* learner, void* stream); /* DQN_agent.py:136-138 */
/* the parameters were written from outside (checkpoint load, BaseAgent.py:29-33): reseed the async actor's copies */
int dra_dqn_learner_invalidate_actor_copy(dra_dqn_learner* learner);
/* DQNActor._transition on device for prm->n_env transitions (graph replay when use_graph). */
int dra_dqn_learner_act(dra_dqn_learner* learner, const dra_dqn_step_params* prm, int use_graph, void* stream);
/* DQNActor._transition's forward (DQN_agent.py:29-33) for a HOST environment: state_host = uint8 [4][84][84]
 * observation, q_host = float[n_actions] out.  The observation is read in place from the learner's mapped host staging, the
 * batch-1 forward of the online parameters is one captured graph whose last kernel publishes q and a completion word to
 * mapped host memory; returns when that word arrives (like the reference's to_np(q)); DRA_ETIMEDOUT after 10 s. */
int dra_dqn_learner_q_host(dra_dqn_learner* learner, const uint8_t* state_host, float* q_host, void* stream);
/* PrioritizedReplay.sample() on the device (dra_sumtree_per_chain2; needs the ring-direct pipeline): _set_per_chain2 once
 * before the first prioritized update; _per_chain2_seed hands the NEXT update's minibatch over from the host (first update,
 * resume); _per_chain2_wait spins until rotation slot `slot`'s block shows launch number >= seq (DRA_ETIMEDOUT after
 * timeout_us).  dra_dqn_learner_step_update / _step_actor are dra_dqn_learner_step (async mode) in two calls: the update of
 * this agent step on device-resident indices (prm: n_env only), then the NEXT step's actor transitions, prm->idx = the
 * indices of the update just issued (read back from the chain kernel's block) for the ring-slot hazard check. */
int dra_dqn_learner_set_per_chain2(dra_dqn_learner* l, dra_sumtree* tree, double* stat_dev, dra_per_chain2_io* io0,
                                   dra_per_chain2_io* io1, dra_per_chain2_io* io2, dra_per_chain2_io* io3,
                                   const uint32_t* rng_words_pinned);
int dra_dqn_learner_per_chain2_seed(dra_dqn_learner* l, const int64_t* tree_idx, const int64_t* data_idx, const double* prob,
                                    float beta, uint64_t rng_cursor, uint64_t seq, void* stream);
int dra_dqn_learner_per_chain2_wait(dra_dqn_learner* l, int slot, uint64_t seq, int64_t timeout_us);
int dra_dqn_learner_step_update(dra_dqn_learner* learner, const dra_dqn_step_params* prm, void* stream_update, void* stream_actor);
int dra_dqn_learner_step_actor(dra_dqn_learner* learner, const dra_dqn_step_params* prm, void* stream_update, void* stream_actor);
int dra_dqn_learner_next_slot(dra_dqn_learner* l, int* slot);
int dra_dqn_learner_sync_loss(dra_dqn_learner* l);
/* Async actor over a HOST environment (BaseAgent.py:142-162 with a real emulator; needs DRA_VAR_ACTOR_PARAMS):
 * _update_async = dra_dqn_learner_update whose optimizer also mirrors the new parameters into actor copy (t mod 2);
 * _q_host_async = dra_dqn_learner_q_host on `stream_actor`, reading the copy the update BEFORE the most recent one wrote --
 * the forward for agent step t+1 overlaps update t and never races with its optimizer. */
int dra_dqn_learner_update_async(dra_dqn_learner* l, int use_graph, int per, float beta, void* stream_update);
int dra_dqn_learner_q_host_async(dra_dqn_learner* l, const uint8_t* state_host, float* q_host, void* stream_actor,
                                 void* stream_update);
/* True resume (optimizer + ring + RNG state; the reference's save() keeps weights only, BaseAgent.py:24-33):
 * the learner-internal state a bit-exact continuation needs beyond what the host owns.  _resume_buffer enumerates device
 * buffers (index 0 .. _resume_buffer_count() - 1; *ptr null when this configuration has no such buffer); _resume_counters reads
 * (restore = 0) or installs (restore = 1, into a FRESH learner of the same configuration before its first step) the
 * pipelines' host-side counters (n >= 16).  Call with the learner synchronised, between agent steps. */
int dra_dqn_learner_resume_buffer_count(void);
int dra_dqn_learner_resume_buffer(dra_dqn_learner* l, int index, void** ptr, int64_t* bytes, char* name, int name_len);
int dra_dqn_learner_resume_counters(dra_dqn_learner* l, int64_t* io, int n, int restore);
/* DRA_VAR_ACTOR_RING: upload the parameter blocks of the next `n` agent steps (consumed in order, one per actor launch;
 * at most 32 may be pending).  With the ring, dra_dqn_learner_step / _act take the transitions from it and use only
 * n_env and idx of the block passed to them. */
int dra_dqn_learner_actor_ring_push(dra_dqn_learner* learner, const dra_dqn_step_params* blocks, int n, void* stream);
/* DQNAgent.step: prm->n_env actor transitions + one update on prm->idx.  stream_actor == NULL: in-order on
 * stream_update (async_actor=False semantics).  stream_actor != NULL: this call's transitions belong to the NEXT
 * step and overlap this step's update (async_actor=True; config.lock becomes HIP events). */
int dra_dqn_learner_step(dra_dqn_learner* learner, const dra_dqn_step_params* prm, int do_update, void* stream_update,
                         void* stream_actor);

/* host-side accounting of dra_dqn_learner_step since the last reset: out[0] calls, out[1] seconds in the call,
 * out[2] seconds of that blocked on a pinned staging slot (GPU back-pressure). */
int dra_dqn_learner_host_stats(dra_dqn_learner* learner, double* out, int reset);

/* DRA_VAR_TARGET_AHEAD: the stream the ahead sequences run on (on the update's CU partition; not owned by the learner; null
 * = switch the variant off).  The learner must have been created with the variant bit (workspaces).  Leaves the lane. */
int dra_dqn_learner_set_ahead_stream(dra_dqn_learner* learner, void* stream);
/* DRA_VAR_TARGET_AHEAD: the indices UniformReplay.sample (replay.py:92-110) will return for the update AFTER the coming
 * dra_dqn_learner_step call (n = batch).  The coming call issues target_network(next_states) of that minibatch
 * (DQN_agent.py:85-88) under its own update; the call after it uses the result if prm->idx equals these indices and
 * computes the target in line otherwise.  A no-op without the variant. */
int dra_dqn_learner_stage_next_indices(dra_dqn_learner* learner, const int64_t* idx_next, int n);
/* out[5]: updates whose target came from the stash, updates that computed it in line, ahead sequences skipped for a ring-slot
 * hazard, stashes dropped for an index mismatch, 1 if the variant is active. */
int dra_dqn_learner_ahead_stats(dra_dqn_learner* learner, int64_t* out);
/* DRA_VAR_FLAG_SYNC accounting since creation, out[12]: out[0] steps issued in the event-free lane, out[1] times the lane was entered,
 * out[2] steps whose actor launch waited for one more count (it overwrites slots the step's own minibatch reads), out[3] steps
 * whose update made the host wait for the actor stream (the minibatch reads slots an unfinished actor launch writes);
 * out[4..8] host nanoseconds inside those calls: pacing wait + hazard checks, index staging (+ the tagged copy command), the update's
 * launches, the actor launch, the whole call; out[9..11] reserved (0). */
int dra_dqn_learner_lane_stats(dra_dqn_learner* learner, int64_t* out);
/* Read-only, for checkers: the code paths this learner resolved, out[12].  Decided at creation: out[0] late fold (no gradient-norm
 * launch), out[1] deferred fc4 step, out[2] chained conv forward, out[3] chained conv backward, out[4] event-free lane, out[5]
 * target-ahead (after dra_dqn_learner_set_ahead_stream).  As of the last launch issued or captured: out[6] the prioritized draw
 * rode in the backward launches, out[7] the VanillaNet head launch was the chained one (head + fc4 backward roles), out[8] it
 * carried the spare workgroups that prefetch fc4's weights, out[9] VanillaNet head launches issued or captured since creation;
 * out[10] the resolved DRA_VAR_* mask; out[11] 1 once a bounded device-side wait gave up (every later step / update returns
 * DRA_ETIMEDOUT).  Changes nothing an update does. */
int dra_dqn_learner_path_flags(dra_dqn_learner* learner, int64_t* out);

/* HIP stream restricted to the compute units whose bit is set in cu_mask (n_words x 32 bits): the async agent step
 * gives the actor chain and the update chain disjoint CU partitions (DRA_VAR_CU_PARTITION, host side). */
int dra_stream_create_masked(void** out_stream, const uint32_t* cu_mask, int n_words);
int dra_stream_destroy(void* stream);
/* placement probe: out[2*wg] = XCC (XCD) id, out[2*wg+1] = HW_ID register of workgroup wg (device uint32[2*n]) */
int dra_probe_hw_id(uint32_t* out, int n_workgroups, void* stream);

/* timeline of the pipelined async step without a profiler: arms 5 timing events per step for the next n_steps
 * steps (actor stream: before gather, after gather, after the actor graph; update stream: before / after the
 * update graph); trace_read returns milliseconds relative to the first event, out[step*5 + slot]. */
int dra_dqn_learner_trace(dra_dqn_learner* learner, int n_steps);
int dra_dqn_learner_trace_read(dra_dqn_learner* learner, float* out_ms, int max_steps, int* n_steps);

/* ---- comm: RCCL gradient all-reduce for the data-parallel on-policy agents (SURVEY.md 8b "comm", 8e).  The reference
 * has no collective; A2C / PPO (A2C_agent.py:55-64, PPO_agent.py:77-99) shard their environments over the GPUs of a node
 * and exchange ONE flat fp32 gradient per optimizer step.  One process per GPU; rank 0 creates the id, the host ships
 * its DRA_COMM_ID_BYTES to the other ranks, every rank calls init_rank (collective). */
#define DRA_COMM_ID_BYTES 256
typedef struct dra_comm dra_comm;
int dra_comm_unique_id(void* id_bytes);
int dra_comm_init_rank(dra_comm** out, int n_ranks, int rank, const void* id_bytes);
int dra_comm_destroy(dra_comm* comm);
int dra_comm_info(dra_comm* comm, int* n_ranks, int* rank); /* as RCCL reports them (ncclCommCount / ncclCommUserRank) */
/* flat_grad <- sum over ranks of (this rank's scale * this rank's flat_grad), in place, asynchronous on stream: the scale is
 * applied BEFORE the sum, so ranks may pass different scales (PPO: rows here / rows of the global minibatch); 1/n_ranks on
 * every rank gives the gradient of the global mean over equal shards */
int dra_allreduce_grads(float* flat_grad, int64_t count, float scale, dra_comm* comm, void* stream);
/* a few fp64 scalars summed over ranks (PPO's global advantage statistics, PPO_agent.py:66) */
int dra_allreduce_f64(double* values, int count, dra_comm* comm, void* stream);

/* ---- ppo_mlp: BASELINE configs[2] (PPO on HalfCheetah shapes, examples.py:497-523) end to end on the device.
 * GaussianActorCriticNet (network_heads.py:173-214) with two separate tanh FCBody(state_dim, (H, H)) networks, H in
 * {16, 32, 64}, state_dim <= 64, action_dim <= 16, separate Adam optimisers (examples.py:508-509), mini_batch_size <= 64. */
/* deep_rl/utils/normalizer.py:28-51 (MeanStdNormalizer over baselines' RunningMeanStd, restated in
 * deeprl_amd/normalizers.py): x f64 [n][d] (device); mean / var f64 [d], count f64 [1] (device, updated when update != 0:
 * batch moments over axis 0, Chan merge, the host class's operation order); outputs clip((x - mean) / sqrt(var + epsilon),
 * +-clip) as f32 and / or f64 (either may be NULL). */
int dra_rms_normalize(const double* x, int n, int d, double* mean, double* var, double* count, int update, double epsilon,
                      double clip, float* out_f32, double* out_f64, void* stream);
/* network_heads.py:205-206 (dist.sample() = mean + scale * standard normal) with counter-hash normals: row r of mean [n][a_dim]
 * is GLOBAL environment env0 + r of n_global; *step_dev (device int64) is the sampler's position, advanced by one per call. */
int dra_gauss_sample(const float* mean, const float* scale, int n, int a_dim, uint64_t noise_seed, int64_t* step_dev,
                     int64_t n_global, int64_t env0, float* out_action, void* stream);
/* one step of n synthetic continuous environments (deeprl_amd/envs.py SyntheticContinuous, csrc/cont_env.h), auto reset on
 * done (envs.py:126-150): state f64 [n][s_dim] and counter i64 [n] are updated in place; action f32 [n][a_dim] is clipped to
 * [-1, 1] (envs.py:186-189); out_reward f64 [n], out_done i32 [n]. */
int dra_cont_env_step(double* state, int64_t* counter, const int64_t* seed, const float* action, int n, int s_dim, int a_dim,
                      int64_t horizon, double* out_reward, int32_t* out_done, void* stream);
typedef struct dra_ppo_mlp_net {     /* one of the two networks with its Adam optimiser (optim.FusedOptimizer's buffers) */
  float* param;                      /* flat parameters (device) */
  float* exp_avg;                    /* Adam first / second moments, same layout */
  float* exp_avg_sq;
  int64_t* step_dev;                 /* device: optimizer steps taken so far; advanced by every step the kernel applies */
  int32_t off_w1, off_b1, off_w2, off_b2, off_w3, off_b3, off_std, reserved;  /* float offsets; off_std < 0: no std (critic) */
  float lr, beta1, beta2, eps;
} dra_ppo_mlp_net;
typedef struct dra_ppo_mlp_cfg {
  int32_t state_dim, action_dim, hidden, mini_batch;
  float ratio_clip, entropy_weight;
  double kl_limit;                   /* the actor steps while approx_kl <= kl_limit = 1.5 * target_kl (PPO_agent.py:88) */
} dra_ppo_mlp_cfg;
int dra_ppo_mlp_supported(int state_dim, int action_dim, int hidden1, int hidden2, int mini_batch);   /* 0 = yes */
/* PPO_agent.py:72-76: the rows of every minibatch of every epoch, gathered once.  state [n][S], action [n][A], log_pi_a /
 * advantage / ret [n] (f32 device), perm i64 [epochs][n] (the np.random permutations, device) -> out_packed: one image per
 * minibatch (epochs x ceil(n / mini_batch) of them, *floats in total) in the layout the update kernel keeps in LDS:
 * 64 x (16 ceil(S / 16) + 4) observations, zero padded, then 64 x 20 = action | log_pi_a, advantage, ret at columns 16..18. */
int dra_ppo_mlp_packed_floats(int n, int epochs, int mini_batch, int s_dim, int64_t* floats);
int dra_ppo_mlp_pack(const float* state, const float* action, const float* log_pi_a, const float* advantage, const float* ret,
                     const int64_t* perm, int n, int epochs, int mini_batch, int s_dim, int a_dim, float* out_packed, void* stream);
/* PPO_agent.py:71-99 for shared_repr = False: epochs x ceil(n / mini_batch) minibatch updates in ONE launch of two persistent
 * workgroups (actor: forward, clipped-ratio loss, approx-KL gate, backward, Adam; critic: forward, value loss, backward, Adam),
 * weights and Adam moments resident in registers / LDS from the first minibatch to the last.  out3 (device f32 [3]) = policy
 * loss, value loss, approx_kl of the LAST minibatch; out_counts (device i64 [2]) = actor / critic steps applied by this launch.
 * dbg: NULL, or device f32 [DRA_PPO_MLP_DBG_FLOATS] receiving the first minibatch's intermediates (tests). */
#define DRA_PPO_MLP_DBG_FLOATS 65536
int dra_ppo_mlp_update(const dra_ppo_mlp_cfg* cfg, const dra_ppo_mlp_net* actor, const dra_ppo_mlp_net* critic,
                       const float* packed, int n, int epochs, float* out3, int64_t* out_counts, float* dbg, void* stream);
/* measurement aid: the same launch (hidden = 64) with shader-clock cycles per phase of the minibatch loop accumulated by thread 0
 * of each workgroup into cycles (device i64 [2][16]: actor row, critic row); tools/prof_ppo_mlp.py names the phases. */
int dra_ppo_mlp_update_profile(const dra_ppo_mlp_cfg* cfg, const dra_ppo_mlp_net* actor, const dra_ppo_mlp_net* critic,
                               const float* packed, int n, int epochs, float* out3, int64_t* out_counts, int64_t* cycles,
                               void* stream);
/* PPO_agent.py:32-49 over device-resident synthetic environments: t_len x [store normalised observation, no-grad forward of
 * both networks, action = mean + softplus(std) * noise, log-probability, environment step, reward / mask, running
 * observation statistics + normalisation] and the bootstrap forward, in ONE launch of one persistent workgroup. */
typedef struct dra_ppo_mlp_rollout_io {
  double* env_state;        /* [n_env][S] raw observations (in/out) */
  int64_t* env_counter;     /* [n_env] (in/out) */
  const int64_t* env_seed;  /* [n_env] */
  double* rms;              /* mean [S], var [S], count [1] (in/out; not updated when rms_update == 0) */
  float* cur_state;         /* [n_env][S] normalised observation the rollout starts from (in) / the next one starts from (out) */
  int64_t* sampler_step;    /* device int64: position of the action-noise stream (advanced by t_len + 1) */
  float* out_state;         /* [t_len][n_env][S] */
  float* out_action;        /* [t_len][n_env][A] */
  float* out_log_pi_a;      /* [t_len][n_env] */
  float* out_v;             /* [t_len + 1][n_env] */
  float* out_reward;        /* [t_len][n_env]  f32(reward * reward_coef) */
  float* out_mask;          /* [t_len][n_env]  1 - done */
  int64_t env0, n_global;   /* first GLOBAL environment index of this rank / global environment count (noise stream) */
  uint64_t noise_seed;
  int64_t horizon;
  double reward_coef, rms_epsilon, rms_clip;
  int32_t rms_update, t_len, n_env, reserved;
} dra_ppo_mlp_rollout_io;
int dra_ppo_mlp_rollout(const dra_ppo_mlp_cfg* cfg, const dra_ppo_mlp_net* actor, const dra_ppo_mlp_net* critic,
                        const dra_ppo_mlp_rollout_io* io, void* stream);
/* measurement aid: the same launch (hidden = 64) with thread 0's shader-clock cycles per phase of the step loop (cycles: device
 * i64 [8]: F1, F2, heads, environment, statistics, normalisation, trailing barrier) */
int dra_ppo_mlp_rollout_profile(const dra_ppo_mlp_cfg* cfg, const dra_ppo_mlp_net* actor, const dra_ppo_mlp_net* critic,
                                const dra_ppo_mlp_rollout_io* io, int64_t* cycles, void* stream);

/* ---- a2c_mlp: a2c_continuous (examples.py:384-404) over device-resident synthetic environments.  GaussianActorCriticNet
 * (network_heads.py:173-214) with an identity phi_body and two FCBody(state_dim, (H, H)) networks of one gate (relu or tanh),
 * H in {32, 64}, state_dim <= 64, action_dim <= 16, n_env <= 64, all parameters in ONE flat buffer (one optimiser). */
typedef struct dra_a2c_mlp_net {
  const float* param;                /* the optimiser's flat parameter buffer (device); read only */
  int32_t a_w1, a_b1, a_w2, a_b2, a_w3, a_b3;   /* actor_body.layers[0..1], fc_action: float offsets into param */
  int32_t c_w1, c_b1, c_w2, c_b2, c_w3, c_b3;   /* critic_body.layers[0..1], fc_critic */
  int32_t off_std;                   /* std [action_dim] */
  int32_t gate;                      /* 1 relu, 2 tanh */
  int32_t state_dim, action_dim, hidden, reserved;
} dra_a2c_mlp_net;
/* A2C_agent.py:22-41 in ONE launch of one workgroup: for t < t_len [normalise the current observation (normalizer.py:28-51:
 * statistics folded first when rms_update != 0; the identity is mean 0, var 1, epsilon 0, clip inf), store it, forward both
 * networks, action = tanh(fc_action(.)) + softplus(std) * noise(noise_seed, *sampler_step + t, n_global, env0 + env, dim),
 * environment step (csrc/cont_env.h), reward * reward_coef, mask = 1 - done], then the bootstrap observation's normalisation
 * and value.  The fields are those of dra_ppo_mlp_rollout_io without the log-probability; cur_state is an OUTPUT here. */
typedef struct dra_a2c_mlp_rollout_io {
  double* env_state;        /* [n_env][S] raw observations (in/out) */
  int64_t* env_counter;     /* [n_env] (in/out) */
  const int64_t* env_seed;  /* [n_env] */
  double* rms;              /* mean [S], var [S], count [1] (in; out when rms_update != 0) */
  float* cur_state;         /* [n_env][S] normalised observation the bootstrap value was computed from (out) */
  int64_t* sampler_step;    /* device int64: position of the action-noise stream (advanced by t_len + 1: A2C_agent.py:41's
                             * bootstrap forward samples an action too) */
  float* out_state;         /* [t_len][n_env][S] */
  float* out_action;        /* [t_len][n_env][A] */
  float* out_v;             /* [t_len + 1][n_env] */
  float* out_reward;        /* [t_len][n_env]  f32(reward * reward_coef) */
  float* out_mask;          /* [t_len][n_env]  1 - done */
  int64_t env0, n_global;   /* first GLOBAL environment index / global environment count (noise stream) */
  uint64_t noise_seed;
  int64_t horizon;
  double reward_coef, rms_epsilon, rms_clip;
  int32_t rms_update, t_len, n_env, reserved;
} dra_a2c_mlp_rollout_io;
int dra_a2c_mlp_supported(int state_dim, int action_dim, int hidden, int n_env, int gate);   /* 0 = yes */
int dra_a2c_mlp_rollout(const dra_a2c_mlp_net* net, const dra_a2c_mlp_rollout_io* io, void* stream);
/* network_heads.py:200-214 behind fc_action, for given actions: z [n][a_dim] = fc_action's output, std [a_dim], action
 * [n][a_dim] -> mean = tanh(z) [n][a_dim]; scale = softplus(std) (linear above 20); log_pi_a [n] = sum_d (-(a - mean)^2 /
 * (2 scale^2) - log scale - log sqrt(2 pi)); entropy [n] = sum_d (0.5 + 0.5 log(2 pi) + log scale).  a_dim <= 64; evaluated
 * in fp64, rounded once. */
int dra_gauss_head_fwd(const float* z, const float* std, const float* action, int n, int a_dim, float* mean, float* log_pi_a,
                       float* entropy, void* stream);
/* its gradient for g_log_pi_a, g_entropy [n] (A2C_agent.py:55-61's losses reach the head through these two): dz [n][a_dim]
 * (through the tanh), dstd [a_dim] (through the softplus; rows summed in a fixed order -- the same bits on every launch). */
int dra_gauss_head_bwd(const float* z, const float* std, const float* action, const float* g_log_pi_a, const float* g_entropy,
                       int n, int a_dim, float* dz, float* dstd, void* stream);

/* ---- dpg_mlp: the DDPG / TD3 update (DDPG_agent.py:62-100, TD3_agent.py:62-108) as a few eager launches ("dpg": deterministic
 * policy gradient).  Networks: an actor S -> H1 -> H2 -> A with tanh on the head and n_critics (1: DDPG, 2: TD3) critics
 * S + A -> H1 -> H2 -> 1, one gate (1 relu, 2 tanh) on every hidden layer, plain Linear layers with biases, all parameters of a
 * network in ONE flat fp32 buffer.  1 <= batch <= 128, S <= 64, A <= 16, H1, H2 <= 512; no size needs to be a multiple of
 * anything.  Every entry point returns -EINVAL outside that range. */
typedef struct dra_dpg_net {
  float* param;              /* flat parameter buffer (device); stepped in place by the two *_update calls (online network) */
  int32_t actor[6];          /* float offsets into param of w1 [H1][S], b1, w2 [H2][H1], b2, w3 [A][H2], b3; any order, gaps allowed */
  int32_t critic[2][6];      /* per critic: w1 [H1][S + A], b1, w2 [H2][H1], b2, w3 [1][H2], b3; critic[1] is ignored when n_critics == 1 */
  int32_t state_dim, action_dim, h1, h2;
  int32_t gate, n_critics;
} dra_dpg_net;
typedef struct dra_dpg_batch {
  const void* state;         /* [batch][state_dim], rows state_stride elements apart; fp32, or fp64 when in_f64 != 0 (narrowed to */
  const void* next_state;    /*   fp32 when loaded: the replay ring hands back the stored dtype) */
  const void* action;        /* [batch][action_dim], same dtype */
  const float* reward;       /* [batch] */
  const float* mask;         /* [batch]  1 - done */
  const float* noise;        /* optional [batch][action_dim] standard normals for TD3's target-policy smoothing; NULL: the counter-
                              * hash stream gauss_noise(noise_seed, noise_counter, batch, row, dim) of csrc/cont_env.h */
  int64_t state_stride, next_state_stride, action_stride;
  int32_t batch, in_f64;
} dra_dpg_batch;
typedef struct dra_dpg_step {
  float* exp_avg;            /* Adam moments, laid out like the ONLINE flat parameter buffer (the actor's and the critics' */
  float* exp_avg_sq;         /*   optimisers own disjoint ranges of it) */
  float step_size, inv_sqrt_bc2;   /* dra_adam_hyper(lr, beta1, beta2, t) of the optimiser this call steps */
  float beta1, beta2, eps;
  float discount;
  float td3_noise, td3_noise_clip, action_low, action_high;   /* n_critics == 2 only */
  uint64_t noise_seed;
  int64_t noise_counter;     /* position t of the smoothing-noise stream (the caller's update counter) */
} dra_dpg_step;
int dra_dpg_supported(int batch, int state_dim, int action_dim, int h1, int h2, int gate, int n_critics);   /* 0 = yes */
/* floats of workspace the update calls need.  Its head is fixed: y [batch], q [2][batch] (online Q_i(s, a) before the step), the
 * per-row critic loss [batch] (0.5 (q - y)^2, or (q1 - y)^2 + (q2 - y)^2); activations and dz of every layer follow. */
int dra_dpg_workspace_floats(int batch, int state_dim, int action_dim, int h1, int h2, int n_critics, int64_t* out);
/* two launches: [target actor + critics -> y; online critics forward, dq = (q - y) / batch (x 2 for two critics: mse + mse), dz
 * chain] over 16-row tiles, then [weight / bias gradient over all rows + Adam in place] per 16 x 16 parameter tile. */
int dra_dpg_critic_update(const dra_dpg_net* online, const dra_dpg_net* target, const dra_dpg_batch* batch,
                          const dra_dpg_step* step, float* workspace, void* stream);
/* two launches, after dra_dpg_critic_update on the same batch and workspace (the states are read from it): [a = actor(s),
 * critic 1 on (s, a), dq = -1 / batch back to da, the actor's dz chain], then the actor's gradient + Adam.  Critic parameters
 * are not touched.  `step` carries the ACTOR optimiser's scalars. */
int dra_dpg_actor_update(const dra_dpg_net* online, const dra_dpg_batch* batch, const dra_dpg_step* step, float* workspace,
                         void* stream);
/* out_action [n][action_dim] = tanh(actor(state)) for n <= 128 rows: one launch */
int dra_dpg_act(const dra_dpg_net* net, const void* state, int64_t state_stride, int in_f64, int n, float* out_action,
                void* stream);
/* ONE agent transition of DDPG_agent.py:62-74 / TD3_agent.py:62-71 over ONE device-resident environment in ONE launch of one
 * workgroup: the observation of the environment narrowed to float32 through the online actor (dra_dpg_act's forward on one row:
 * out_action has its bits), the behaviour action in fp64 from the staged vector v --
 *   *mode 0 (warm-up): v;   1 (Gaussian): (double)a + v;   2 (Ornstein-Uhlenbeck): x = (x + ((ou_theta (ou_mu - x)) ou_dt)) + v,
 *   (double)a + x, with x = ou_x [A] carried in device memory
 * -- clipped to [bounds[0], bounds[1]]; ring row *slot = (the fp64 observation the action was chosen on, the fp64 action [A], the
 * fp64 reward, 1 - done); the environment step with the auto reset; for an episode that ended one appended row of ep_ring
 * (*step_counter, 0, episodic return) and ou_x <- ou_x0 (in every mode).  *step_counter advances by one.  A *slot outside
 * [0, capacity) is taken as 0 and counted in *err.  No parameter is written.
 * env_kind 0: the pendulum of csrc/pendulum_env.h (env_state [2] = theta, theta'; state_dim 3, action_dim 1);
 * env_kind 1: the synthetic continuous environment of csrc/cont_env.h (env_state [state_dim]; ep_steps is not used). */
typedef struct dra_dpg_env_act_io {
  double* env_state;            /* (in/out) */
  int64_t* env_counter;         /* [1] (in/out) */
  int32_t* ep_steps;            /* [1] (in/out) */
  double* ep_return;            /* [1] (in/out) */
  const int64_t* env_seed;      /* [1] */
  int64_t* step_counter;        /* [1] (in/out) */
  int64_t* ep_count;            /* [1] (in/out) */
  double* ep_ring;              /* [ring_cap][3] */
  const int64_t* mode;          /* [1] staged */
  const int64_t* slot;          /* [1] staged: the replay's cursor before the step */
  const double* bounds;         /* [2] staged: the action space's low and high */
  const double* v;              /* [action_dim] staged */
  double* ou_x;                 /* [action_dim] (in/out) */
  const double* ou_x0;          /* [action_dim] */
  double* ring_frames;          /* [capacity][state_dim] */
  double* ring_actions;         /* [capacity][action_dim] */
  double* ring_rewards;         /* [capacity] */
  int32_t* ring_masks;          /* [capacity] */
  float* out_action;            /* [action_dim]: tanh(actor(observation)) */
  int32_t* err;                 /* [1] (in/out): staged words that were out of range */
  int64_t horizon, ring_cap, capacity;
  double ou_theta, ou_mu, ou_dt;
  int32_t env_kind, reserved;
} dra_dpg_env_act_io;
int dra_dpg_env_act_supported(int env_kind, int state_dim, int action_dim, int h1, int h2, int gate);   /* 0 = yes; host only */
int dra_dpg_env_act(const dra_dpg_net* net, const dra_dpg_env_act_io* io, void* stream);
/* Evaluation of a DDPG / TD3 actor (BaseAgent.py:60-77: config.eval_episodes greedy episodes of config.eval_env) over a
 * device-resident pendulum (csrc/pendulum_env.h) in ONE launch of ceil(n_episodes / 16) workgroups.  The pendulum ends an episode at
 * the step limit only and draws its reset state from its total step counter, so episode e begins at pendulum_reset(c0 + e horizon),
 * c0 = *env_counter -- whatever env_state, *ep_steps and *ep_return held does not survive, as with Task.reset() -- and the episodes
 * run in lockstep as rows of dra_dpg_act's forward: every action has dra_dpg_act's bits for its observation.  out_return [e] is the
 * in-order fp64 sum of the episode's rewards.  The environment is left as the host loop leaves it after its last auto reset:
 * counter c0 + n_episodes horizon, the reset state at that counter, episode steps 0, episode return 0; *out_steps = n_episodes
 * horizon.  Those words depend on c0 alone and are written once, by the workgroup that is the last to have read c0 (*arrive counts
 * them and is left 0): no workgroup waits for another.  out_state / out_action are filled only when given.  No parameter is written.
 * 1 <= n_episodes <= 128, horizon >= 1, n_episodes * horizon <= 65536, state_dim 3, action_dim 1, h1 / h2 / gate as for
 * dra_dpg_env_act; anything else, or a null required pointer, is -EINVAL with nothing written. */
typedef struct dra_dpg_eval_io {
  double* env_state;            /* [2] (out) */
  int64_t* env_counter;         /* [1] (in/out) */
  int32_t* ep_steps;            /* [1] (out) */
  double* ep_return;            /* [1] (out) */
  const int64_t* env_seed;      /* [1] */
  double* out_return;           /* [n_episodes] */
  int64_t* out_steps;           /* [1] */
  int32_t* arrive;              /* [1] (in/out): 0 before the first launch; every launch leaves it 0 */
  double* out_state;            /* optional [n_episodes][horizon + 1][2]: the state before each step and the last one */
  float* out_action;            /* optional [n_episodes][horizon] */
  int64_t horizon;
  int32_t n_episodes, reserved;
} dra_dpg_eval_io;
int dra_dpg_eval_supported(int n_episodes, int64_t horizon, int state_dim, int action_dim, int h1, int h2, int gate);   /* 0 = yes; host only */
int dra_dpg_eval(const dra_dpg_net* net, const dra_dpg_eval_io* io, void* stream);

/* ---- cat_mlp: a2c_feature (examples.py:340-358) over device-resident cart-pole environments (csrc/cartpole_env.h,
 * deeprl_amd/envs.py CartPole: the same function bit for bit).
 * one step of n environments with DummyVecEnv's auto reset: state f64 [n][4] (x, x', theta, theta'), counter i64 [n] (total
 * steps: the reset stream's position), ep_steps i32 [n] and ep_return f64 [n] are updated in place; action i64 [n] (1 pushes
 * right, anything else left); out_reward f64 [n] (1.0), out_done i32 [n]. */
int dra_cartpole_step(double* state, int64_t* counter, int32_t* ep_steps, double* ep_return, const int64_t* seed,
                      const int64_t* action, int n, int64_t horizon, double* out_reward, int32_t* out_done, void* stream);
/* CategoricalActorCriticNet (network_heads.py:217-255) over a two-layer FCBody phi_body of one width (tanh or relu), identity
 * actor / critic bodies, biased Linear heads; every parameter in ONE flat buffer (one optimiser).  state_dim 4, 2 actions,
 * hidden in {16, 32, 64}, n_env <= 64. */
typedef struct dra_cat_mlp_net {
  const float* param;                /* the optimiser's flat parameter buffer (device); read only */
  int32_t w1, b1, w2, b2;            /* phi_body.layers[0..1]: float offsets into param */
  int32_t wa, ba, wc, bc;            /* fc_action [n_actions][hidden], fc_critic [1][hidden] */
  int32_t gate;                      /* 1 relu, 2 tanh */
  int32_t state_dim, n_actions, hidden;
} dra_cat_mlp_net;
/* A2C_agent.py:22-41 in ONE launch of one workgroup: for t < t_len [observation narrowed to float32 and stored, body, logits
 * and v, action = argmax_a (logit_a + Gumbel noise of (noise_seed, *sampler_step + t, env0 + env, a)) -- dra_gumbel_sample's
 * stream, bit for bit --, environment step, reward * reward_coef, mask = 1 - done, and for every episode that ended one
 * appended row of ep_ring], then the bootstrap observation's value.  *sampler_step advances by t_len + 1.
 * ep_ring row (*ep_count mod ring_cap) = (sampler step of the end, global environment, episodic return); *ep_count counts
 * every episode ever ended.  Rows are appended in (step, environment) order with vector stores. */
typedef struct dra_cat_mlp_rollout_io {
  double* env_state;        /* [n_env][4] (in/out) */
  int64_t* env_counter;     /* [n_env] (in/out) */
  int32_t* ep_steps;        /* [n_env] (in/out) */
  double* ep_return;        /* [n_env] (in/out) */
  const int64_t* env_seed;  /* [n_env] */
  int64_t* sampler_step;    /* [1] (in/out) */
  int64_t* ep_count;        /* [1] (in/out) */
  double* ep_ring;          /* [ring_cap][3] */
  float* out_state;         /* [t_len][n_env][4] */
  int64_t* out_action;      /* [t_len][n_env] */
  float* out_v;             /* [t_len + 1][n_env] */
  float* out_reward;        /* [t_len][n_env] */
  float* out_mask;          /* [t_len][n_env] */
  int64_t env0, n_global;   /* first GLOBAL environment of this rollout, global environment count */
  uint64_t noise_seed;
  int64_t horizon, ring_cap;
  double reward_coef;
  int32_t t_len, n_env;
} dra_cat_mlp_rollout_io;
int dra_cat_mlp_supported(int state_dim, int n_actions, int hidden, int n_env, int gate);   /* 0 = yes */
int dra_cat_mlp_rollout(const dra_cat_mlp_net* net, const dra_cat_mlp_rollout_io* io, void* stream);

/* ---- q_mlp: n_step_dqn_feature (examples.py:408-424, NStepDQN_agent.py:13-67) over device-resident cart-pole environments.
 * VanillaNet(action_dim, FCBody(state_dim)): a two-layer FCBody of one width (relu or tanh) under a plain biased fc_head.  The
 * online and the target network live in two flat buffers of EQUAL layout (one set of offsets).  state_dim 4, 2 actions, hidden
 * in {16, 32, 64}. */
typedef struct dra_q_mlp_net {
  const float* param;                /* the optimiser's flat parameter buffer (device): the ONLINE network; read only */
  const float* target;               /* the TARGET network's flat buffer, same offsets; read only (the update does not read it) */
  int32_t w1, b1, w2, b2;            /* body.layers[0..1]: float offsets into param / target (and the flat gradient buffer) */
  int32_t wq, bq;                    /* fc_head [n_actions][hidden], [n_actions] */
  int32_t gate;                      /* 1 relu, 2 tanh */
  int32_t state_dim, n_actions, hidden;
} dra_q_mlp_net;
/* NStepDQN_agent.py:31-57 in ONE launch of one workgroup: for t < t_len [observation narrowed to float32 and stored, body, q
 * stored, action = random_action[t][e] where explore[t][e] else the FIRST maximum of q (np.argmax), environment step, reward *
 * reward_coef, mask = 1 - done, and for every episode that ended one appended row of ep_ring], then bootstrap[e] = max_a of the
 * TARGET network's q on the last observation.  No parameter is written.  *step_counter advances by t_len; ep_ring row
 * (*ep_count mod ring_cap) = (*step_counter + t of the end, environment, episodic return), appended in (step, environment)
 * order with vector stores; *ep_count counts every episode ever ended.  n_env <= 64. */
typedef struct dra_q_mlp_rollout_io {
  double* env_state;            /* [n_env][4] (in/out) */
  int64_t* env_counter;         /* [n_env] (in/out) */
  int32_t* ep_steps;            /* [n_env] (in/out) */
  double* ep_return;            /* [n_env] (in/out) */
  const int64_t* env_seed;      /* [n_env] */
  int64_t* step_counter;        /* [1] (in/out) */
  int64_t* ep_count;            /* [1] (in/out) */
  double* ep_ring;              /* [ring_cap][3] */
  const uint8_t* explore;       /* [t_len][n_env]: nonzero = take random_action */
  const int64_t* random_action; /* [t_len][n_env] */
  float* out_state;             /* [t_len][n_env][4] */
  float* out_q;                 /* [t_len][n_env][2] */
  int64_t* out_action;          /* [t_len][n_env] */
  float* out_reward;            /* [t_len][n_env] */
  float* out_mask;              /* [t_len][n_env] */
  float* bootstrap;             /* [n_env] */
  int64_t horizon, ring_cap;
  double reward_coef;
  int32_t t_len, n_env;
} dra_q_mlp_rollout_io;
/* NStepDQN_agent.py:58-65 and the whole backward in ONE launch of one workgroup: ret[t][e] = reward + (discount * mask) * ret
 * backwards from bootstrap (the reference's loop and operation order, fp32), the forward recomputed from the stored states with
 * the ONLINE parameters, loss = 0.5 * mean_r (q[r][a_r] - ret_r)^2 and its gradient with respect to w1 b1 w2 b2 wq bq, written
 * (every element, nothing between the tensors) into `grad` at the parameters' offsets.  Fixed summation order, no atomics.
 * rows = t_len * n_env <= 1024 (dra_q_mlp_update_supported). */
typedef struct dra_q_mlp_update_io {
  const float* state;           /* [t_len][n_env][4] */
  const int64_t* action;        /* [t_len][n_env] (1 = the second action, anything else the first) */
  const float* reward;          /* [t_len][n_env] */
  const float* mask;            /* [t_len][n_env] */
  const float* bootstrap;       /* [n_env] */
  float* grad;                  /* the flat gradient buffer (device) */
  float* out_ret;               /* [t_len][n_env] */
  float* out_loss;              /* [1] */
  double discount;
  int32_t t_len, n_env;
} dra_q_mlp_update_io;
int dra_q_mlp_supported(int state_dim, int n_actions, int hidden, int n_env, int gate);         /* the rollout; 0 = yes */
int dra_q_mlp_update_supported(int state_dim, int n_actions, int hidden, int rows, int gate);   /* the update; 0 = yes */
int dra_q_mlp_rollout(const dra_q_mlp_net* net, const dra_q_mlp_rollout_io* io, void* stream);
int dra_q_mlp_update(const dra_q_mlp_net* net, const dra_q_mlp_update_io* io, void* stream);

/* ---- oc_mlp: option_critic_feature (examples.py:450-468, OptionCritic_agent.py:11-119) over device-resident cart-pole
 * environments.  OptionCriticNet(FCBody(state_dim), action_dim, num_options): a two-layer FCBody of one width (relu or tanh)
 * under three plain biased heads, fc_q [O][hidden], fc_pi [O * A][hidden] (row o * A + a: action a of option o) and fc_beta
 * [O][hidden] (network_heads.py:105-127).  The online and the target network live in two flat buffers of EQUAL layout.
 * state_dim 4, 2 actions, hidden in {16, 32, 64}, 2 <= n_options <= 8 (one option is refused: the reference's initial
 * prev_options = ones, OptionCritic_agent.py:26, is out of range there). */
typedef struct dra_oc_mlp_net {
  const float* param;                /* the optimiser's flat parameter buffer (device): the ONLINE network; read only */
  const float* target;               /* the TARGET network's flat buffer, same offsets; read only (the update does not read it) */
  int32_t w1, b1, w2, b2;            /* body.layers[0..1]: float offsets into param / target (and the flat gradient buffer) */
  int32_t wq, bq;                    /* fc_q [n_options][hidden], [n_options] */
  int32_t wp, bp;                    /* fc_pi [n_options * n_actions][hidden], [n_options * n_actions] */
  int32_t wb, bb;                    /* fc_beta [n_options][hidden], [n_options] */
  int32_t gate;                      /* 1 relu, 2 tanh */
  int32_t state_dim, n_actions, hidden, n_options;
} dra_oc_mlp_net;
/* OptionCritic_agent.py:55-93 in ONE launch of one workgroup: for t < t_len [observation narrowed to float32 and stored, body,
 * q, beta = sigmoid(.) and the intra-option logits of the ONLINE network, sample_option (OptionCritic_agent.py:29-49) with
 * eps[t]: g = the FIRST maximum of q, pi_opt = eps / O with 1 - eps + eps / O at g, pi_hat = (1 - beta) 1[o == prev] + beta
 * pi_opt, option = is_initial ? invCDF(pi_opt, uniform[t][e][0]) : invCDF(pi_hat, uniform[t][e][1]) (each row divided by its sum
 * first, as Categorical(probs=) does), action / log pi(a) / entropy from the chosen option's logits by inverse CDF at
 * uniform[t][e][2], environment step, reward * reward_coef, mask = 1 - done, prev_option <- option, is_initial <- done, and for
 * every episode that ended one appended row of ep_ring], then from the TARGET network's q and beta on the last observation
 * bootstrap[e] = (1 - beta[prev]) q[prev] + beta[prev] max q with prev the option of step t_len - 1.  No parameter is written.
 * prev_option / is_initial are read at the start (values outside [0, n_options) are clamped) and replaced at the end;
 * *step_counter advances by t_len; ep_ring as in dra_q_mlp_rollout.  n_env <= 64. */
typedef struct dra_oc_mlp_rollout_io {
  double* env_state;            /* [n_env][4] (in/out) */
  int64_t* env_counter;         /* [n_env] (in/out) */
  int32_t* ep_steps;            /* [n_env] (in/out) */
  double* ep_return;            /* [n_env] (in/out) */
  const int64_t* env_seed;      /* [n_env] */
  int64_t* step_counter;        /* [1] (in/out) */
  int64_t* ep_count;            /* [1] (in/out) */
  double* ep_ring;              /* [ring_cap][3] */
  const float* eps;             /* [t_len]: random_option_prob of each step */
  const float* uniform;         /* [t_len][n_env][3]: fresh option, continued option, action */
  int64_t* prev_option;         /* [n_env] (in/out) */
  uint8_t* is_initial;          /* [n_env] (in/out) */
  float* out_state;             /* [t_len][n_env][4] */
  float* out_q;                 /* [t_len][n_env][n_options] */
  float* out_beta;              /* [t_len][n_env][n_options] */
  float* out_logits;            /* [t_len][n_env][2]: the chosen option's */
  int64_t* out_option;          /* [t_len][n_env] */
  int64_t* out_prev_option;     /* [t_len][n_env]: what the step read */
  int64_t* out_action;          /* [t_len][n_env] */
  float* out_init;              /* [t_len][n_env]: what the step read, 0 / 1 */
  float* out_log_pi_a;          /* [t_len][n_env] */
  float* out_entropy;           /* [t_len][n_env] */
  float* out_reward;            /* [t_len][n_env] */
  float* out_mask;              /* [t_len][n_env] */
  float* bootstrap;             /* [n_env] */
  int64_t horizon, ring_cap;
  double reward_coef;
  int32_t t_len, n_env;
} dra_oc_mlp_rollout_io;
/* OptionCritic_agent.py:95-116 and the whole backward in ONE launch of one workgroup: ret[t][e] = reward + (discount * mask) *
 * ret backwards from bootstrap (fp32, the reference's operation order), adv = ret - q[option], v = max q (1 - eps_t) + mean q
 * eps_t, beta_adv = q[prev_option] - v + termination_regularizer -- all from the rollout's STORED q / beta / logits --, the body
 * recomputed from the stored states with the ONLINE parameters, and the gradient of pi_loss + q_loss + beta_loss (q_loss = mean
 * 0.5 (q[option] - ret)^2, pi_loss = mean (-log pi(a) adv - entropy_weight entropy), beta_loss = mean beta[prev_option] beta_adv
 * (1 - init)) with respect to w1 b1 w2 b2 wq bq wp bp wb bb, written (every element, nothing between the tensors) into `grad`
 * at the parameters' offsets.  Fixed summation order, no atomics.  loss [4] = (total, q_loss, pi_loss, beta_loss).
 * rows = t_len * n_env <= 1024 (dra_oc_mlp_update_supported). */
typedef struct dra_oc_mlp_update_io {
  const float* state;           /* [t_len][n_env][4] */
  const float* q;               /* [t_len][n_env][n_options] */
  const float* beta;            /* [t_len][n_env][n_options] */
  const float* logits;          /* [t_len][n_env][2] */
  const int64_t* option;        /* [t_len][n_env] */
  const int64_t* prev_option;   /* [t_len][n_env] */
  const int64_t* action;        /* [t_len][n_env] */
  const float* init;            /* [t_len][n_env] */
  const float* log_pi_a;        /* [t_len][n_env] */
  const float* entropy;         /* [t_len][n_env] */
  const float* reward;          /* [t_len][n_env] */
  const float* mask;            /* [t_len][n_env] */
  const float* bootstrap;       /* [n_env] */
  const float* eps;             /* [t_len] */
  float* grad;                  /* the flat gradient buffer (device) */
  float* out_ret;               /* [t_len][n_env] */
  float* out_adv;               /* [t_len][n_env] */
  float* out_beta_adv;          /* [t_len][n_env] */
  float* out_loss;              /* [4] */
  double discount, termination_regularizer, entropy_weight;
  int32_t t_len, n_env;
} dra_oc_mlp_update_io;
int dra_oc_mlp_supported(int state_dim, int n_actions, int hidden, int n_env, int gate, int n_options);         /* the rollout; 0 = yes */
int dra_oc_mlp_update_supported(int state_dim, int n_actions, int hidden, int rows, int gate, int n_options);   /* the update; 0 = yes */
int dra_oc_mlp_rollout(const dra_oc_mlp_net* net, const dra_oc_mlp_rollout_io* io, void* stream);
int dra_oc_mlp_update(const dra_oc_mlp_net* net, const dra_oc_mlp_update_io* io, void* stream);

/* ---- dqn_mlp: dqn_feature (examples.py:11-52, DQN_agent.py:14-138) over ONE device-resident cart-pole environment and the HBM
 * replay ring (dra_ring_pointers: fp64 observations of 32 bytes, int64 actions, fp64 rewards, int32 masks).  The networks are
 * dra_q_mlp_net's: VanillaNet over a two-layer FCBody of one width, online and target in two flat buffers of equal layout.
 * Everything that changes from agent step to agent step -- the first ring slot, the exploration draws, the sampled indices -- is
 * read from device memory, so a captured launch sees the values staged last.
 *
 * DQN_agent.py:23-45, t_len times, in ONE launch of one workgroup: q of the ONLINE network on the observation narrowed to float32,
 * action = random_action[k] where explore[k] else the FIRST maximum of q (np.argmax), environment step with the auto reset, and
 * ring row (*slot0 + k) % capacity = (the fp64 observation the action was chosen on, action, reward_coef * reward, 1 - done);
 * for every episode that ended one appended row of ep_ring, as dra_q_mlp_rollout appends it (environment 0).  No parameter is
 * written.  *step_counter advances by t_len.  A *slot0 outside [0, capacity) is taken as 0 and counted in *err. */
typedef struct dra_dqn_mlp_act_io {
  double* env_state;            /* [1][4] (in/out) */
  int64_t* env_counter;         /* [1] (in/out) */
  int32_t* ep_steps;            /* [1] (in/out) */
  double* ep_return;            /* [1] (in/out) */
  const int64_t* env_seed;      /* [1] */
  int64_t* step_counter;        /* [1] (in/out) */
  int64_t* ep_count;            /* [1] (in/out) */
  double* ep_ring;              /* [ring_cap][3] */
  const uint8_t* explore;       /* [t_len]: nonzero = take random_action */
  const int64_t* random_action; /* [t_len] */
  const int64_t* slot0;         /* [1]: the replay's cursor before the step */
  double* ring_frames;          /* [capacity][4] */
  int64_t* ring_actions;        /* [capacity] */
  double* ring_rewards;         /* [capacity] */
  int32_t* ring_masks;          /* [capacity] */
  float* out_q;                 /* [t_len][2] */
  int64_t* out_action;          /* [t_len] */
  int32_t* err;                 /* [1] (in/out): staged words that were out of range */
  int64_t horizon, ring_cap, capacity;
  double reward_coef;
  int32_t t_len, n_env;         /* 1 <= t_len <= 8, n_env == 1 */
} dra_dqn_mlp_act_io;
/* DQN_agent.py:81-99, 128-133 and the whole backward in ONE launch of one workgroup: for b < batch the ring rows at idx[b] (state
 * = frame idx, next state = frame idx + 1, both narrowed to float32, action, reward and mask narrowed to float32), q_next = max_a
 * of the TARGET network on the next state -- double_q: the target's value at the FIRST maximum of the ONLINE network's --,
 * q_target = reward + ((discount * q_next) * mask) in fp32, td = q_target - q[a] of the ONLINE network on the state, loss = 0.5
 * mean td^2 and its gradient with respect to w1 b1 w2 b2 wq bq, written (every element, nothing between the tensors) into `grad`
 * at the parameters' offsets.  Fixed summation order, no atomics.  An idx outside [0, capacity - 2] is clamped into it and
 * counted in *err.  1 <= batch <= 256 (dra_dqn_mlp_update_supported). */
typedef struct dra_dqn_mlp_update_io {
  const double* ring_frames;    /* [capacity][4] */
  const int64_t* ring_actions;  /* [capacity] (1 = the second action, anything else the first) */
  const double* ring_rewards;   /* [capacity] */
  const int32_t* ring_masks;    /* [capacity] */
  const int64_t* idx;           /* [batch] */
  float* grad;                  /* the flat gradient buffer (device) */
  float* out_q_target;          /* [batch] */
  float* out_td;                /* [batch] */
  float* out_loss;              /* [1] */
  int32_t* err;                 /* [1] (in/out) */
  int64_t capacity;
  double discount;
  int32_t batch, double_q;
} dra_dqn_mlp_update_io;
int dra_dqn_mlp_supported(int state_dim, int n_actions, int hidden, int t_len, int gate);          /* the acting launch; 0 = yes */
int dra_dqn_mlp_update_supported(int state_dim, int n_actions, int hidden, int batch, int gate);   /* the update; 0 = yes */
int dra_dqn_mlp_act(const dra_q_mlp_net* net, const dra_dqn_mlp_act_io* io, void* stream);
int dra_dqn_mlp_update(const dra_q_mlp_net* net, const dra_dqn_mlp_update_io* io, void* stream);
/* The two launches over n_lanes independent agents of ONE network shape (seed lanes, above: the tables' memory, 1 <= n_lanes <= 64): workgroup (0, lane) runs dra_dqn_mlp_act / dra_dqn_mlp_update on nets[lane] and ios[lane], to the bit.
 * DRA_EINVAL, and nothing is launched, for a null table, an n_lanes outside the range, a lane the single entry refuses, or a lane
 * whose state_dim / n_actions / hidden / gate are not lane 0's. */
int dra_dqn_mlp_lanes_supported(int state_dim, int n_actions, int hidden, int t_len, int batch, int gate, int n_lanes);   /* 0 = yes */
int dra_dqn_mlp_act_lanes(const dra_q_mlp_net* nets, const dra_dqn_mlp_act_io* ios, int n_lanes, void* stream);
int dra_dqn_mlp_update_lanes(const dra_q_mlp_net* nets, const dra_dqn_mlp_update_io* ios, int n_lanes, void* stream);
/* dra_dqn_mlp_update over an n-step window with optional priorities (dqn_feature with n_step > 1 and / or a PrioritizedReplay:
 * config.fused_dqn_replay_feature), ONE launch of one workgroup: for b < batch the n-step transition at DATA index idx[b]
 * (replay.py:112-140): state = frame idx, next state = frame idx + n_step, action of row idx, reward = the fold cum = r_i + (m_i *
 * step_discount) * cum over i = n_step - 1 .. 0 in fp64 narrowed to float32, mask = the product of the n_step masks; q_next,
 * q_target (discount = config.discount ** n_step) and td as in dra_dqn_mlp_update.  With prob set (DQN_agent.py:120-127): prio[b] =
 * (|td[b]| + replay_eps) ** replay_alpha of the UNWEIGHTED td (sqrtf where replay_alpha is 0.5), weights[b] = (prob[b] * batch +
 * 1e-6) ** -*beta divided by their maximum over the whole minibatch, loss = 0.5 mean (td weights)^2, d loss / d q[a] = -(td weights)
 * weights / batch.  With prob NULL no weight is applied and beta, out_prio and out_weights are not touched (they may be NULL); with
 * n_step 1 on top every output and every gradient element has dra_dqn_mlp_update's bits.  The gradient is written as there.  An idx
 * outside [0, capacity - 1 - n_step] is clamped into it and counted in *err.  1 <= batch <= 256, 1 <= n_step <= 8
 * (dra_dqn_replay_mlp_update_supported). */
typedef struct dra_dqn_replay_mlp_update_io {
  const double* ring_frames;    /* [capacity][4] */
  const int64_t* ring_actions;  /* [capacity] (1 = the second action, anything else the first) */
  const double* ring_rewards;   /* [capacity] */
  const int32_t* ring_masks;    /* [capacity] */
  const int64_t* idx;           /* [batch]: data indices */
  const float* prob;            /* [batch]: sampling probabilities, or NULL (no priorities: a uniform replay) */
  const float* beta;            /* [1] (device): read when the launch runs; NULL allowed where prob is NULL */
  float* grad;                  /* the flat gradient buffer (device) */
  float* out_q_target;          /* [batch] */
  float* out_td;                /* [batch]: the unweighted td */
  float* out_loss;              /* [1] */
  float* out_prio;              /* [batch]: the new priorities, in sample order (prob set) */
  float* out_weights;           /* [batch] (prob set) */
  int32_t* err;                 /* [1] (in/out) */
  int64_t capacity;
  double discount;              /* the bootstrap factor: config.discount ** n_step */
  double step_discount;         /* the fold's: the replay's discount */
  double replay_eps, replay_alpha;
  int32_t batch, double_q, n_step, reserved;
} dra_dqn_replay_mlp_update_io;
int dra_dqn_replay_mlp_update_supported(int state_dim, int n_actions, int hidden, int batch, int gate, int n_step);   /* 0 = yes */
int dra_dqn_replay_mlp_update(const dra_q_mlp_net* net, const dra_dqn_replay_mlp_update_io* io, void* stream);
/* The window's update over n_lanes independent agents of ONE network shape and ONE window (seed lanes, above: the tables' memory,
 * 1 <= n_lanes <= 64; seed_batch.DQNReplayFeatureSeeds): workgroup (0, lane) runs dra_dqn_replay_mlp_update on nets[lane] and
 * ios[lane], to the bit.  prob is each lane's own: lanes with and without priorities may share a launch.  The acting and
 * evaluation launches of such lanes are dra_dqn_mlp_act_lanes and dra_dqn_mlp_eval_lanes as they are (acting writes 1-step rows).
 * DRA_EINVAL, and nothing is launched, for a null table, an n_lanes outside the range, a lane the single entry refuses, a lane
 * whose state_dim / n_actions / hidden / gate are not lane 0's, or a lane whose n_step is not lane 0's.
 * dra_dqn_replay_mlp_lanes_supported: dra_dqn_mlp_supported (t_len), dra_dqn_replay_mlp_update_supported (batch, n_step) and the
 * lane count. */
int dra_dqn_replay_mlp_lanes_supported(int state_dim, int n_actions, int hidden, int t_len, int batch, int gate, int n_step,
                                       int n_lanes);   /* 0 = yes */
int dra_dqn_replay_mlp_update_lanes(const dra_q_mlp_net* nets, const dra_dqn_replay_mlp_update_io* ios, int n_lanes, void* stream);

/* ---- dist_mlp: categorical_dqn_feature (examples.py:164-193, CategoricalDQN_agent.py) and quantile_regression_dqn_feature
 * (examples.py:101-127, QuantileRegressionDQN_agent.py) over ONE device-resident cart-pole environment and the HBM replay ring:
 * dqn_mlp's two launches with a distributional head.  CategoricalNet / QuantileNet over a two-layer FCBody of one width, the
 * head one plain biased layer of n_actions * n_atoms outputs (row a * n_atoms + j: atom / quantile j of action a); online and
 * target in two flat buffers of equal layout.  state_dim 4, 2 actions, hidden in {16, 32, 64}, 2 <= n_atoms <= 51. */
typedef struct dra_dist_mlp_net {
  const float* param;                /* the optimiser's flat parameter buffer (device): the ONLINE network; read only */
  const float* target;               /* the TARGET network's flat buffer, same offsets; read only (the acting launch does not read it) */
  int32_t w1, b1, w2, b2;            /* body.layers[0..1]: float offsets into param / target (and the flat gradient buffer) */
  int32_t wq, bq;                    /* the head [n_actions * n_atoms][hidden], [n_actions * n_atoms] */
  int32_t gate;                      /* 1 relu, 2 tanh */
  int32_t state_dim, n_actions, hidden;
  int32_t head;                      /* 1 categorical (C51), 2 quantile (QR-DQN) */
  int32_t n_atoms;                   /* atoms / quantiles per action */
  double v_min, v_max;               /* categorical: the support, z = linspace(v_min, v_max, n_atoms) in fp64 narrowed to float32 */
} dra_dist_mlp_net;
/* The acting launch is dra_dqn_mlp_act's with dra_dqn_mlp_act_io as it is; the action values (out_q [t_len][2]) are sum_j
 * softmax(logits)_j z_j (categorical) or the mean of the quantiles (quantile).
 *
 * The update, ONE launch of one workgroup: for b < batch the ring rows at idx[b] as in dra_dqn_mlp_update; the TARGET network's
 * head on the next state; a_next = the FIRST maximum of its action values (categorical + double_q: of the ONLINE network's;
 * quantile: of the quantile sums, double_q is not read).
 *   categorical  Tz_j = clamp(reward + (discount * mask) * z_j, v_min, v_max); target_i = sum_j clamp(1 - |Tz_j - z_i| / delta, 0, 1)
 *                p_next[a_next][j]; loss_vec[b] = sum_i target_i log(target_i + 1e-5) - target_i log_softmax(logits[a])_i;
 *                loss = mean_b loss_vec.
 *   quantile     target_j = reward + (discount * mask) * theta_next[a_next][j]; d = target_j - theta[a]_i; loss_vec[j] = mean_b
 *                sum_i huber(d) |tau_i - 1[d < 0]|, tau_i = (2 i + 1) / (2 n_atoms); loss = mean_j loss_vec.
 * and the gradient of loss with respect to w1 b1 w2 b2 wq bq, written (every element, nothing between the tensors) into `grad`
 * at the parameters' offsets.  Fixed summation order, no atomics.  An idx outside [0, capacity - 2] is clamped into it and counted
 * in *err.  1 <= batch <= 256 (dra_dist_mlp_update_supported: what fits the workgroup's 160 KiB of LDS). */
typedef struct dra_dist_mlp_update_io {
  const double* ring_frames;    /* [capacity][4] */
  const int64_t* ring_actions;  /* [capacity] (1 = the second action, anything else the first) */
  const double* ring_rewards;   /* [capacity] */
  const int32_t* ring_masks;    /* [capacity] */
  const int64_t* idx;           /* [batch] */
  float* grad;                  /* the flat gradient buffer (device) */
  float* out_loss;              /* [1] */
  float* out_loss_vec;          /* categorical [batch]; quantile [n_atoms] */
  float* out_q_next;            /* [batch][2]: the TARGET network's action values of the next states */
  float* out_target;            /* [batch][n_atoms] */
  int32_t* err;                 /* [1] (in/out) */
  int64_t capacity;
  double discount;
  int32_t batch, double_q;
} dra_dist_mlp_update_io;
int dra_dist_mlp_supported(int state_dim, int n_actions, int hidden, int t_len, int gate, int head, int n_atoms);          /* 0 = yes */
int dra_dist_mlp_update_supported(int state_dim, int n_actions, int hidden, int batch, int gate, int head, int n_atoms);   /* 0 = yes */
int dra_dist_mlp_act(const dra_dist_mlp_net* net, const dra_dqn_mlp_act_io* io, void* stream);
int dra_dist_mlp_update(const dra_dist_mlp_net* net, const dra_dist_mlp_update_io* io, void* stream);
/* The two launches over n_lanes independent agents of ONE network shape (seed lanes, above: the tables' memory, 1 <= n_lanes <= 64):
 * workgroup (0, lane) runs dra_dist_mlp_act / dra_dist_mlp_update on nets[lane] and ios[lane], to the bit.  v_min / v_max are each
 * lane's own.  DRA_EINVAL, and nothing is launched, for a null table, an n_lanes outside the range, a lane the single entry
 * refuses, or a lane whose state_dim / n_actions / hidden / gate / head / n_atoms are not lane 0's (the launch's LDS size follows
 * from lane 0's n_atoms). */
int dra_dist_mlp_lanes_supported(int state_dim, int n_actions, int hidden, int t_len, int batch, int gate, int head, int n_atoms,
                                 int n_lanes);   /* 0 = yes */
int dra_dist_mlp_act_lanes(const dra_dist_mlp_net* nets, const dra_dqn_mlp_act_io* ios, int n_lanes, void* stream);
int dra_dist_mlp_update_lanes(const dra_dist_mlp_net* nets, const dra_dist_mlp_update_io* ios, int n_lanes, void* stream);

/* ---- np_mt: the seed lanes' draws taken on the device from numpy's own stream (seed_batch.py, device_draws=True; csrc/np_mt.h has
 * the protocol).  A lane owns a legacy np.random.RandomState: dra_np_mt_state is its get_state() -- key[624], then pos (624 = the
 * key is regenerated before the next word) --, DRA_NP_MT_STATE_WORDS uint32 per lane, 16-byte aligned.  One step of a lane is, in
 * the order of support.plan_actor_epsilon_greedy then replay.draw_uniform_indices: per transition randint(n_actions, size=1) and
 * rand(1) < eps[j] in float64; then, if learn, the rejection loop of randint(0, ring_size) until `batch` indices are valid at
 * history_length = n_step = 1.  The values go into the lane's block where the act / update lane kernels read them: int64 first
 * slot at 0, int64 idx[batch] at idx_off, int64 random actions[k] at rand_off, uint8 flags[k] at flag_off (seed_batch.lane_layout;
 * idx is left alone when learn is 0); the state ends where numpy's ends.  What the lanes share in a step comes from
 * dra_np_mt_common, read when the launch RUNS (a captured launch sees what was uploaded last).
 * No lane spins: a step makes no further attempt once it has taken more than 4096 words; the draws it gave up on are 0 and
 * DRA_NP_MT_ERR_BUDGET is or-ed into the lane's err word (the act / update kernels count into the same word).
 * dra_np_mt_draw_lanes: workgroup (0, lane) of 64 threads per lane; states [n_lanes][DRA_NP_MT_STATE_WORDS], out_blocks n_lanes
 * blocks block_stride bytes apart, err [n_lanes], all device memory.  1 <= n_lanes <= 64, 1 <= k <= 8, 1 <= batch <= 256,
 * 1 <= n_actions, ring capacity 2 .. 2^32 - 1 (dra_np_mt_lanes_supported: 0 = yes).
 * dra_np_mt_draw_host: the same step of ONE lane, serially, over host memory -- no device is touched.  It states the protocol for
 * the CPU tests and is the kernel's debugging twin, not a path of the product.  DRA_EINVAL also for a ring state with no valid
 * index (learn != 0) and for a pos outside 0 .. 624.
 * The *_window_* entries are the same step over an n-step window (the lanes of dqn_feature with n_step > 1,
 * seed_batch.DQNReplayFeatureSeeds): an index v is valid iff v + n_step < ring_pos or (v >= ring_pos and v + n_step < ring_size),
 * UniformReplay.valid_index at history_length = 1; max(ring_pos - n_step, 0) + max(ring_size - n_step - ring_pos, 0) slots are.
 * 1 <= n_step <= 8, ring capacity n_step + 1 .. 2^32 - 1 (dra_np_mt_window_lanes_supported: 0 = yes); everything else as above.  The
 * entries without a window ARE these with n_step 1 (the same launch, the same bits).  A ring state with no window-valid index is
 * the host's to refuse before the step (dra_np_mt_draw_window_host: DRA_EINVAL); a launch over one ends within its budget, sets
 * DRA_NP_MT_ERR_BUDGET and writes index 0. */
#define DRA_NP_MT_STATE_WORDS 628
#define DRA_NP_MT_ERR_BUDGET 1073741824
typedef struct dra_np_mt_state {
  uint32_t key[624];
  int32_t pos;
  int32_t reserved[3];
} dra_np_mt_state;
typedef struct dra_np_mt_common {
  int64_t slot0;       /* the ring slot of the step's first transition */
  int64_t ring_pos;    /* the ring's pos and size AFTER the step's k appends */
  int64_t ring_size;
  double eps[8];       /* [k]: epsilon of transition j (1.0 below exploration_steps) */
} dra_np_mt_common;
int dra_np_mt_lanes_supported(int n_lanes, int k, int batch, int n_actions, int64_t capacity);   /* 0 = yes */
int dra_np_mt_draw_lanes(void* states, void* out_blocks, const dra_np_mt_common* common, int* err, int n_lanes, int k, int batch,
                         int n_actions, int learn, int idx_off, int rand_off, int flag_off, int block_stride, void* stream);
int dra_np_mt_draw_host(void* state, void* out_block, const dra_np_mt_common* common, int* err, int k, int batch, int n_actions,
                        int learn, int idx_off, int rand_off, int flag_off);
int dra_np_mt_window_lanes_supported(int n_lanes, int k, int batch, int n_actions, int64_t capacity, int n_step);   /* 0 = yes */
int dra_np_mt_draw_window_lanes(void* states, void* out_blocks, const dra_np_mt_common* common, int* err, int n_lanes, int k,
                                int batch, int n_actions, int learn, int idx_off, int rand_off, int flag_off, int block_stride,
                                int n_step, void* stream);
int dra_np_mt_draw_window_host(void* state, void* out_block, const dra_np_mt_common* common, int* err, int k, int batch,
                               int n_actions, int learn, int idx_off, int rand_off, int flag_off, int n_step);

/* ---- rainbow_mlp: rainbow_feature (examples.py:231-280: CategoricalDQNAgent, RainbowNet over FCBody(noisy_linear=True), n-step
 * PrioritizedReplay, double_q) over ONE device-resident cart-pole environment and the HBM replay ring: dist_mlp's two launches
 * over four NoisyLinear layers and the dueling head.  A layer's effective parameters are formed in the kernels from its RAW noise
 * vectors: W = w_mu + w_sigma * (f(e_out) (x) f(e_in)), b = b_mu + b_sigma * f(e_b), f(x) = sign(x) sqrt|x| (network_utils.py:66-83).
 * state_dim 4, 2 actions, hidden in {16, 32, 64}, 2 <= n_atoms <= 51. */
typedef struct dra_rainbow_mlp_layer {
  int32_t w_mu, w_sigma, b_mu, b_sigma;   /* float offsets into param / target (and the flat gradient buffer) */
  int32_t e_in, e_out, e_b;               /* float offsets of noise_in, noise_out_weight, noise_out_bias in a noise row */
  int32_t reserved;
} dra_rainbow_mlp_layer;
typedef struct dra_rainbow_mlp_net {
  const float* param;                /* the optimiser's flat parameter buffer (device): the ONLINE network; read only */
  const float* target;               /* the TARGET network's flat buffer, same offsets; read only (the acting launch does not read it) */
  const float* noise;                /* the ONLINE network's raw noise: acting [t_len] rows noise_stride floats apart (transition k
                                        runs under row k), the update one row; read when the launch runs, so a captured launch
                                        sees the draw uploaded last */
  const float* target_noise;         /* the TARGET network's raw noise, one row of the same layout (the update alone reads it) */
  dra_rainbow_mlp_layer l1, l2;      /* body.layers[0] [hidden][4], body.layers[1] [hidden][hidden] */
  dra_rainbow_mlp_layer value;       /* fc_value [n_atoms][hidden] */
  dra_rainbow_mlp_layer advantage;   /* fc_advantage [n_actions * n_atoms][hidden] (row a * n_atoms + j: atom j of action a) */
  int32_t noise_stride;              /* floats between two noise rows of the acting launch */
  int32_t gate;                      /* 1 relu, 2 tanh */
  int32_t state_dim, n_actions, hidden, n_atoms;
  double v_min, v_max;               /* the support, z = linspace(v_min, v_max, n_atoms) in fp64 narrowed to float32 */
} dra_rainbow_mlp_net;
/* The acting launch is dra_dqn_mlp_act's with dra_dqn_mlp_act_io as it is; the action values (out_q [t_len][2]) are sum_j
 * softmax(v + adv_a - mean_a adv)_j z_j under noise row k.  (Under noisy layers epsilon is 0, DQN_agent.py:34-35: the host stages
 * explore = 0.)
 *
 * The update, ONE launch of one workgroup: for b < batch the n-step transition at DATA index idx[b] (replay.py:112-140): state =
 * frame idx, next state = frame idx + n_step, action of row idx, reward = the fold cum = r_i + (m_i * step_discount) * cum over i =
 * n_step - 1 .. 0 in fp64 narrowed to float32, mask = the product of the n_step masks.  The TARGET network under target_noise on the
 * next states; a_next = the FIRST maximum of its action values (double_q: of the ONLINE network's under `noise`); Tz_j = clamp(reward
 * + (discount * mask) * z_j, v_min, v_max); target_i = sum_j clamp(1 - |Tz_j - z_i| / delta, 0, 1) p_next[a_next][j]; loss_vec[b] =
 * sum_i target_i log(target_i + 1e-5) - target_i log_softmax(logits[a])_i of the ONLINE network under the same `noise` on the state;
 * prio[b] = (|loss_vec[b]| + replay_eps) ** replay_alpha; weights[b] = (prob[b] * batch + 1e-6) ** -*beta divided by their maximum
 * (DQN_agent.py:120-127); loss = mean_b loss_vec[b] weights[b], and its gradient with respect to the sixteen tensors (w_mu, w_sigma,
 * b_mu, b_sigma of the four layers), written (every element, nothing between the tensors) into `grad` at the parameters' offsets.
 * Fixed summation order, no atomics.  An idx outside [0, capacity - 1 - n_step] is clamped into it and counted in *err.
 * 1 <= batch <= 64, 1 <= n_step <= 8 (dra_rainbow_mlp_update_supported: what fits the workgroup's 160 KiB of LDS). */
typedef struct dra_rainbow_mlp_update_io {
  const double* ring_frames;    /* [capacity][4] */
  const int64_t* ring_actions;  /* [capacity] (1 = the second action, anything else the first) */
  const double* ring_rewards;   /* [capacity] */
  const int32_t* ring_masks;    /* [capacity] */
  const int64_t* idx;           /* [batch]: data indices */
  const float* prob;            /* [batch]: sampling probabilities */
  const float* beta;            /* [1] (device): read when the launch runs */
  float* grad;                  /* the flat gradient buffer (device) */
  float* out_loss;              /* [1] */
  float* out_loss_vec;          /* [batch]: the unweighted KL */
  float* out_prio;              /* [batch]: the new priorities, in sample order */
  float* out_weights;           /* [batch] */
  float* out_q_next;            /* [batch][2]: the TARGET network's action values of the next states */
  float* out_target;            /* [batch][n_atoms] */
  int32_t* err;                 /* [1] (in/out) */
  int64_t capacity;
  double discount;              /* the bootstrap factor: config.discount ** n_step */
  double step_discount;         /* the fold's: the replay's discount */
  double replay_eps, replay_alpha;
  int32_t batch, double_q, n_step, reserved;
} dra_rainbow_mlp_update_io;
int dra_rainbow_mlp_supported(int state_dim, int n_actions, int hidden, int t_len, int gate, int n_atoms);                        /* 0 = yes */
int dra_rainbow_mlp_update_supported(int state_dim, int n_actions, int hidden, int batch, int gate, int n_atoms, int n_step);    /* 0 = yes */
int dra_rainbow_mlp_act(const dra_rainbow_mlp_net* net, const dra_dqn_mlp_act_io* io, void* stream);
int dra_rainbow_mlp_update(const dra_rainbow_mlp_net* net, const dra_rainbow_mlp_update_io* io, void* stream);

/* ---- evaluation of the three kinds above (BaseAgent.py:60-77: config.eval_episodes greedy episodes of config.eval_env) in ONE
 * launch of one workgroup over ONE device-resident cart-pole that is not the actor's.  The launch first does what Task.reset()
 * does (a reset at *env_counter, episode steps and return 0: whatever ep_steps / ep_return held does not survive), then steps
 * the environment under the FIRST maximum of the ONLINE network's action values (no exploration word is read, no replay-ring or
 * episode-ring row and no step counter is written; net->target is not read) with the auto reset on done, until n_episodes
 * episodes have ended: episode e leaves out_return[e] and out_length[e].  The environment's words are left as the last auto
 * reset left them, *out_steps is the number of environment steps taken (the sum of the lengths).  out_q, where given, takes the
 * action values of step k in row k; rows behind *out_steps are not written.  dra_rainbow_mlp_eval forms the effective weights
 * ONCE, from net->noise as ONE row (the online network's own buffers: what its module forward uses between two reset_noise()).
 * 1 <= n_episodes <= 256, horizon >= 1, n_episodes * horizon <= 65536 (dra_mlp_eval_supported); anything else is DRA_EINVAL and
 * nothing is written. */
typedef struct dra_mlp_eval_io {
  double* env_state;            /* [1][4] (in/out) */
  int64_t* env_counter;         /* [1] (in/out) */
  int32_t* ep_steps;            /* [1] (in/out) */
  double* ep_return;            /* [1] (in/out) */
  const int64_t* env_seed;      /* [1] */
  double* out_return;           /* [n_episodes] */
  int32_t* out_length;          /* [n_episodes] */
  int64_t* out_steps;           /* [1] */
  float* out_q;                 /* [n_episodes * horizon][2], or null */
  int64_t horizon;
  int32_t n_episodes, reserved;
} dra_mlp_eval_io;
int dra_mlp_eval_supported(int n_episodes, int64_t horizon);                                       /* 0 = yes */
int dra_dqn_mlp_eval(const dra_q_mlp_net* net, const dra_mlp_eval_io* io, void* stream);
int dra_dist_mlp_eval(const dra_dist_mlp_net* net, const dra_mlp_eval_io* io, void* stream);
int dra_rainbow_mlp_eval(const dra_rainbow_mlp_net* net, const dra_mlp_eval_io* io, void* stream);

/* The evaluation of n_lanes independent agents of ONE network shape in ONE launch (seed lanes, above: the tables' memory,
 * 1 <= n_lanes <= 64): workgroup (0, lane) runs dra_dqn_mlp_eval / dra_dist_mlp_eval on nets[lane] and ios[lane], to the bit.
 * n_episodes and horizon are the lane's own and may differ between lanes; a lane leaves when ITS episodes have ended and waits for
 * no other.  DRA_EINVAL, and nothing is launched or written, for a null table, an n_lanes outside the range, a lane the single
 * entry refuses, or a lane whose network shape is not lane 0's.  dra_rainbow_mlp_eval has no lane form. */
int dra_mlp_eval_lanes_supported(int n_episodes, int64_t horizon, int n_lanes);                   /* 0 = yes */
int dra_dqn_mlp_eval_lanes(const dra_q_mlp_net* nets, const dra_mlp_eval_io* ios, int n_lanes, void* stream);
int dra_dist_mlp_eval_lanes(const dra_dist_mlp_net* nets, const dra_mlp_eval_io* ios, int n_lanes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
