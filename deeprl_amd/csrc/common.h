// Shared helpers for the deeprl_amd HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/deeprl_amd.h"  // exported signatures are checked against the public header

#define DRA_OK 0
#define DRA_EINVAL (-22)
#define DRA_ENOMEM (-12)
#define DRA_ETIMEDOUT (-110)   // a bounded device-side wait gave up (late_step arrival slots, actor hand-over): the results are invalid

// Every export returns 0 or an error code; nothing throws or aborts across the C ABI.
#define DRA_HIP(expr)                                  \
  do {                                                 \
    hipError_t _e = (expr);                            \
    if (_e != hipSuccess) return (int)_e;              \
  } while (0)

#define DRA_LAUNCH_CHECK()                             \
  do {                                                 \
    hipError_t _e = hipGetLastError();                 \
    if (_e != hipSuccess) return (int)_e;              \
  } while (0)

#define DRA_API extern "C" __attribute__((visibility("default")))

static inline hipStream_t dra_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// ---- one RMSprop element (torch.optim.RMSprop, centered or not; g already the raw gradient, coef the clip coefficient) -- the
// ONE statement of the arithmetic for optim.hip's step kernels and for the riders below
__device__ __forceinline__ void rmsprop_elem(float& p, float g, float& s, float& a, float coef, float alpha, float oma,
                                             float lr, float eps, int centered) {
  const float gk = g * coef;
  s = s * alpha + oma * gk * gk;
  float avg;
  if (centered) {
    a = a * alpha + oma * gk;
    avg = sqrtf(s - a * a) + eps;
  } else {
    avg = sqrtf(s) + eps;
  }
  p = p - lr * (gk / avg);
}

// ---- 16-byte hand-over accesses (round 6) -------------------------------------------------------------------------------------
// A 4-byte write-through store is one fabric write of its own and an 8-byte agent-scope load runs at 0.54-0.70x the 16-byte
// rate; a 16-byte write-through store costs what a plain one does.  mega_ld4<true> / mega_st4<true> are ONE
// buffer_load_dwordx4 ... sc1 / buffer_store_dwordx4 ... sc1 (the raw-buffer builtins with the sc1 bit: the compiler counts
// them in vmcnt like any other access).  `base` is WAVE-UNIFORM (it becomes the buffer resource, in scalar registers), the
// per-lane part is a 32-bit index: every buffer handed over inside a launch is far below 4 GB.
// DRA_EXP_WIDE_HANDOVER is the A/B switch of every site that uses them (`make exp EXPFLAGS=-DDRA_EXP_WIDE_HANDOVER=0` builds
// the 4- / 8-byte forms): bit 0 = 16-byte loads (slab folds, dy staging), bit 1 = the forward chain's conv1 -> conv2 planes
// (conv_v2.hip).  (The weight-gradient slab stores as 16-byte stores -- each MFMA register group transposed inside its quad of
// lanes -- measured slower than the 4-byte ones and were removed: DESIGN_HISTORY.md round 6, row 29.)
#ifndef DRA_EXP_WIDE_HANDOVER
#define DRA_EXP_WIDE_HANDOVER 3
#endif
constexpr bool kWideLd4 = (DRA_EXP_WIDE_HANDOVER & 1) != 0;
constexpr bool kWideFwdPlanes = (DRA_EXP_WIDE_HANDOVER & 2) != 0;
typedef float dra_f4 __attribute__((ext_vector_type(4)));
typedef unsigned dra_u4 __attribute__((ext_vector_type(4)));
constexpr int kBufSc1 = 16;             // aux bit of the raw-buffer builtins that sets sc1 on gfx950
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mega_rsrc(const void* base) {
  // raw buffer (stride 0), no bound (the callers clamp their indices).  Word 3 = 0x00020000 (DATA_FORMAT 32) with the dst-sel /
  // num-format fields left zero: only the untyped raw_buffer_load / store builtins use this resource, which ignore them
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, -1, 0x00020000);
}
// float4 number `idx4` behind the wave-uniform, 16-byte aligned `base`.  The 16-byte coherent form addresses with a 32-bit byte
// offset: idx4 < 2^27 there (the launchers of the chained kernels check what is not a compile-time size); the other forms keep
// 64-bit pointer arithmetic
template <bool COH> __device__ __forceinline__ dra_f4 mega_ld4(const dra_f4* base, int64_t idx4) {
  if constexpr (COH && kWideLd4) {
    const dra_u4 u = __builtin_amdgcn_raw_buffer_load_b128(mega_rsrc(base), (int)idx4 * 16, 0, kBufSc1);
    dra_f4 v;
    v.x = __uint_as_float(u.x); v.y = __uint_as_float(u.y); v.z = __uint_as_float(u.z); v.w = __uint_as_float(u.w);
    return v;
  } else if constexpr (COH) {   // two 8-byte relaxed atomic loads
    const unsigned long long* q = reinterpret_cast<const unsigned long long*>(base + idx4);
    const unsigned long long a = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long b = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    dra_f4 v;
    v.x = __uint_as_float((unsigned)a); v.y = __uint_as_float((unsigned)(a >> 32));
    v.z = __uint_as_float((unsigned)b); v.w = __uint_as_float((unsigned)(b >> 32));
    return v;
  } else {
    return base[idx4];
  }
}
// v to the four floats that start `off` floats (a multiple of 4, < 2^29) behind the wave-uniform, 16-byte aligned `base`.  (A
// primitive: which sites store 16 bytes is decided by the caller's DRA_EXP_WIDE_HANDOVER bit, not here.)
template <bool COH> __device__ __forceinline__ void mega_st4(float* base, int off, dra_f4 v) {
  if constexpr (COH) {
    dra_u4 u;
    u.x = __float_as_uint(v.x); u.y = __float_as_uint(v.y); u.z = __float_as_uint(v.z); u.w = __float_as_uint(v.w);
    __builtin_amdgcn_raw_buffer_store_b128(u, mega_rsrc(base), off * 4, 0, kBufSc1);
  } else {
    *reinterpret_cast<dra_f4*>(base + off) = v;
  }
}

// ---- DRA_VAR_DEFER_FC4 (round 6): the fc4 segment of the DQN learner's optimizer step, deferred ------------------------------
// fc4's weights are 95 % of the parameters: 51 of the 54 MB the optimizer launch moves, on the update's critical path for ~8 of
// its ~15 us.  Nothing reads them before fc4's forward of the NEXT update (the fourth launch of its graph, ~31 us in) -- and
// the actor reads its copy of them ~16 us after that graph starts.  So the optimizer launch steps everything BUT that segment,
// leaves the clip coefficient in device memory and raises `pending`; the segment is stepped by RIDER workgroups -- extra
// z-slices of the next update's conv1 / conv2 forward launches (conv_v2.hip), memory-bound work beside latency-bound work --
// with the arithmetic above, hence the same bits.  The launch after the riders' lowers `pending` and marks the actor copy the
// riders completed as valid (the actor's fc4 waits for that word before it requests the weights).  Anything that reads the
// parameters outside the pipelined graphs flushes first (learner.hip flush_fc4): the same rider code as a launch of its own.
struct DraFc4Rider {
  float *p, *g, *s1, *s2, *p_copy;    // flat buffers (p_copy: the actor copy the deferred step also has to reach; may be null)
  int64_t begin4, count4;             // the segment, in float4 units
  const float* coef;                  // clip coefficient left by the optimizer launch
  const int* pending;                 // != 0: the segment has not been stepped yet
  float lr, alpha, eps;
  int centered;
};
// DRA_EXP_RIDER_WT: how the riders of the chained forward launch (fc4_rider_run<true>) store.  Their launch announces their
// completion itself, so the actor copy has to be written through; as four 4-byte agent-scope stores per float4 that is one fabric
// write per float (1.6 M per update), and what the riders store plainly (p, s1, s2: 19.3 MB) is still dirty in the L2 when the
// launch ends, in front of fc4's forward.  Levels (`make exp EXPFLAGS=-DDRA_EXP_RIDER_WT=n` builds the others for an A/B):
//   0  the copy as four 4-byte write-through stores, p / s1 / s2 as plain float4 stores
//   1  the copy as ONE mega_st4<true> (buffer_store_dwordx4 ... sc1) per float4
//   2  level 1 + s1 and (centered) s2 as mega_st4<true>
//   3  level 2 + p
// The arithmetic, the grid and the completion protocol (vmcnt(0), barrier, count) are the same at every level: same bits.  The
// plain form (fc4_rider_run<false>: the flush kernel, the per-layer launches' riders) does not change with the switch.
// Measured (profiles/rider_wt_ab.jsonl, six interleaved alternations of bench.py --steps 2000 on one box): level 0 11 010-11 062
// updates/s, level 1 11 248-11 344, level 2 11 284-11 406, level 3 11 256-11 394 -- the copy's width is the gain (+2.5 %), levels
// 2 and 3 are inside each other's spread; 3 is the default.  (DRA_EXP_RIDER_NT, the riders' gradient / state / copy traffic as
// non-temporal accesses, measured 11 094-11 229 in the same session and was removed: below every level here, and a non-temporal
// store of the copy is not written through.)
#ifndef DRA_EXP_RIDER_WT
#define DRA_EXP_RIDER_WT 3
#endif
constexpr int kRiderNV = 3;           // float4 per thread of a rider workgroup (256 threads)
__host__ __device__ inline int fc4_rider_blocks(int64_t count4) { return (int)((count4 + 256 * kRiderNV - 1) / (256 * kRiderNV)); }
// what a launcher of fc4_rider_run<true> checks: mega_st4 addresses with a 32-bit float offset below 2^29 behind 16-byte aligned bases
static inline bool fc4_rider_wt_ok(const DraFc4Rider& r) {
  if (r.begin4 < 0 || r.count4 < 1 || r.begin4 >= ((int64_t)1 << 27) || r.count4 >= ((int64_t)1 << 27)) return false;
  if (4 * (r.begin4 + r.count4) >= ((int64_t)1 << 29)) return false;
  return (((uintptr_t)r.p | (uintptr_t)r.g | (uintptr_t)r.s1 | (uintptr_t)r.s2 | (uintptr_t)r.p_copy) & 15) == 0;
}

// rider workgroup `rb` of `nrb` (nrb * 256 * kRiderNV >= count4).  COPY_WT: the actor copy is written THROUGH (agent-scope stores) --
// for riders whose completion is announced from inside their own launch (the forward chain: no launch boundary writes the L2 back
// before the actor, on another XCD, is told that the copy is complete)
template <bool COPY_WT = false>
__device__ __forceinline__ void fc4_rider_run(const DraFc4Rider& r, int rb) {
  constexpr int WT = COPY_WT ? DRA_EXP_RIDER_WT : 0;
  if (*r.pending == 0) return;
  const int64_t i0 = (int64_t)rb * (256 * kRiderNV) + threadIdx.x;
  float4 P[kRiderNV], G[kRiderNV], S[kRiderNV], A[kRiderNV];
  const float4* p4 = reinterpret_cast<const float4*>(r.p) + r.begin4;
  const float4* g4 = reinterpret_cast<const float4*>(r.g) + r.begin4;
  const float4* s4 = reinterpret_cast<const float4*>(r.s1) + r.begin4;
  const float4* a4 = reinterpret_cast<const float4*>(r.centered ? r.s2 : r.s1) + r.begin4;
#pragma unroll
  for (int v = 0; v < kRiderNV; ++v) {
    const int64_t i = i0 + 256 * v, ic = i < r.count4 ? i : r.count4 - 1;
    P[v] = p4[ic]; G[v] = g4[ic]; S[v] = s4[ic]; A[v] = a4[ic];
  }
  const float coef = *r.coef, oma = 1.f - r.alpha;
#pragma unroll
  for (int v = 0; v < kRiderNV; ++v) {
    const int64_t i = i0 + 256 * v;
    if (i < r.count4) {
      float* pp = &P[v].x; const float* gg = &G[v].x; float* ss = &S[v].x; float* aa = &A[v].x;
#pragma unroll
      for (int k = 0; k < 4; ++k) rmsprop_elem(pp[k], gg[k], ss[k], aa[k], coef, r.alpha, oma, r.lr, r.eps, r.centered);
      // (the bases are kernel arguments, hence wave-uniform; the launcher checked fc4_rider_wt_ok: off + 3 < 2^29)
      const int off = 4 * (int)(r.begin4 + i);
      const dra_f4 pv = {P[v].x, P[v].y, P[v].z, P[v].w}, sv = {S[v].x, S[v].y, S[v].z, S[v].w}, av = {A[v].x, A[v].y, A[v].z, A[v].w};
      if constexpr (WT >= 3) mega_st4<true>(r.p, off, pv);
      else reinterpret_cast<float4*>(r.p)[r.begin4 + i] = P[v];
      if (r.p_copy) {
        if constexpr (WT >= 1) {
          mega_st4<true>(r.p_copy, off, pv);
        } else if constexpr (COPY_WT) {
          float* pc = r.p_copy + 4 * (r.begin4 + i);
#pragma unroll
          for (int k = 0; k < 4; ++k) __hip_atomic_store(pc + k, pp[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          reinterpret_cast<float4*>(r.p_copy)[r.begin4 + i] = P[v];
        }
      }
      if constexpr (WT >= 2) {
        mega_st4<true>(r.s1, off, sv);
        if (r.centered) mega_st4<true>(r.s2, off, av);
      } else {
        reinterpret_cast<float4*>(r.s1)[r.begin4 + i] = S[v];
        if (r.centered) reinterpret_cast<float4*>(r.s2)[r.begin4 + i] = A[v];
      }
    }
  }
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel: remember, per device ordinal, the largest
// size already granted (a process that launches on a second GPU after a first -- select_device -- must set it there too;
// ADVICE r5).  One object per kernel instantiation (a function-local static at the launch site).
struct DraLdsAttr {
  size_t granted[32] = {};
};
static inline int dra_grant_lds(DraLdsAttr& a, const void* kernel, size_t bytes) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) dev = 0;
  if (bytes > a.granted[dev]) {
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
    a.granted[dev] = bytes;
  }
  return DRA_OK;
}

constexpr int kWave = 64;  // CDNA4 wavefront

// 64-lane butterfly reductions (wave64: offsets up to 32).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- cross-workgroup hand-over inside ONE launch (the actor's conv3 + fc4 launch, the update's chained launches) ----------------
struct MegaSync {
  unsigned* done = nullptr;        // this role's arrival counter (producers), null = nothing to publish
  const unsigned* wait = nullptr;  // the counter this role waits on (consumers), null = nothing to wait for
  unsigned wait_target = 0;
  int* timeout_flag = nullptr;     // pinned host int
  // optional: counters that are never reset -- the wait is for (*epoch + 1) * wait_target arrivals, `epoch` = launches of this
  // kind completed so far (a LATER launch of the same step bumps it: the update's head kernel for the forward chain)
  const unsigned* epoch = nullptr;
  unsigned epoch_bias = 1;         // (0: the bump has already happened when the waiting launch runs -- the backward chain)
  int slow = 0;                    // != 0: poll every ~0.4 us (hundreds of waiting workgroups on ONE counter: the slab folds)
};
constexpr unsigned long long kMegaWaitTicks = 5000000ull;   // 50 ms of s_memrealtime (100 MHz)

// Has an arrival counter reached `target`?  The counters that are never reset and their targets (epoch x arrivals per epoch) both
// wrap modulo 2^32, so the comparison is by modular distance: a plain `count < target` lets every consumer through in the update
// whose target wraps to a small number (or to 0: a power-of-two arrival count) while the counter is still just below 2^32.  Valid
// while the outstanding distance stays under 2^31 -- it is at most one epoch's arrivals, a few hundred.  The ONE statement of the
// device-side waits (mega_wait); tests/test_chain_counter_wrap_host.py runs it on the host around every wrap.
__host__ __device__ __forceinline__ bool chain_reached(unsigned count, unsigned target) {
  return (unsigned)(count - target) < 0x80000000u;
}

__device__ __forceinline__ void mega_publish(const MegaSync& ms) {
  if (!ms.done) return;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_fetch_add(ms.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void mega_wait(const MegaSync& ms) {
  if (!ms.wait) return;
  if (threadIdx.x == 0) {
    const unsigned long long t0 = wall_clock64();
    const unsigned target = ms.epoch ? (*ms.epoch + ms.epoch_bias) * ms.wait_target : ms.wait_target;
    while (!chain_reached(__hip_atomic_load(ms.wait, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), target)) {
      if (ms.slow) __builtin_amdgcn_s_sleep(16);
      else __builtin_amdgcn_s_sleep(1);
      if (wall_clock64() - t0 > kMegaWaitTicks) {
        if (ms.timeout_flag) __hip_atomic_store(ms.timeout_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        break;
      }
    }
  }
  __syncthreads();
}
template <bool COH> __device__ __forceinline__ float mega_ld(const float* p) {
  if constexpr (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}
template <bool COH> __device__ __forceinline__ void mega_st(float* p, float v) {
  if constexpr (COH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}


// What a ROLE of a chained launch (oneshot.h / oneshot_lin.h roles under fused.hip's bwd_chain_kernel) needs to know about its
// place in the chain: the counters its workgroups wait on / count themselves on, one 128-byte line per sample (stride in
// unsigned; 0 = ONE counter for the whole role: the slab folds wait for every weight-gradient workgroup of a layer).
constexpr int kChainLine = 32;    // unsigned per counter line
struct ChainHook {
  const unsigned* wait = nullptr;
  unsigned wait_target = 0;       // arrivals per launch on one counter
  int wait_stride = 0;
  unsigned* done = nullptr;
  int done_stride = 0;
  const unsigned* epoch = nullptr;
  unsigned epoch_bias = 0;
  int slow = 0;
  int* timeout_flag = nullptr;
  __device__ __forceinline__ MegaSync sync(int sample) const {
    MegaSync ms;
    if (wait) { ms.wait = wait + (int64_t)sample * wait_stride; ms.wait_target = wait_target; }
    if (done) ms.done = done + (int64_t)sample * done_stride;
    ms.epoch = epoch; ms.epoch_bias = epoch_bias; ms.timeout_flag = timeout_flag; ms.slow = slow;
    return ms;
  }
};

// ------------------------------------------------------------------------------------------------
// A given action outside [0, A) behaves as the nearest valid one: the forward takes log_pi_a there, and the backward kernels
// (categorical_bwd_kernel, policy_heads_bwd_kernel) differentiate THAT value -- one statement for all three.
__device__ __forceinline__ int64_t categorical_clamp_action(int64_t action, int A) {
  if (action < 0) return 0;
  if (action >= A) return A - 1;
  return action;
}

// Categorical(logits = x[0..A)) of one sample (network_heads.py:249-254): log-softmax, entropy, and -- when no action is given --
// the inverse-CDF draw from one uniform (first a with cumsum(p)[a] > u; the last action absorbs rounding).  ONE statement shared
// by categorical_fwd_kernel (losses.hip) and the fused rollout head (igemm.hip: policy_heads_sample_kernel), so that both give
// the same bits for the same logits.
__device__ __forceinline__ void categorical_row(const float* x, int A, bool given, int64_t action_in, float ub, int64_t* act_out,
                                                float* log_pi_a, float* entropy) {
  float m = x[0];
  for (int a = 1; a < A; ++a) m = fmaxf(m, x[a]);
  float se = 0.f;
  for (int a = 0; a < A; ++a) se += expf(x[a] - m);
  const float lse = m + logf(se);
  int64_t act = given ? action_in : (int64_t)(A - 1);
  float ent = 0.f, cum = 0.f;
  bool found = given;
  for (int a = 0; a < A; ++a) {
    const float lp = x[a] - lse, p = expf(lp);
    ent -= p * lp;
    cum += p;
    if (!found && cum > ub) { act = a; found = true; }
  }
  act = categorical_clamp_action(act, A);
  *act_out = act;
  *log_pi_a = x[act] - lse;
  *entropy = ent;
}

// Backward of the same: dlogits[a] = g_lp (1[a == action] - p[a]) - g_ent p[a] (logp[a] + entropy), action clamped as the
// forward clamps it (categorical_clamp_action, by the caller).  categorical_row_stats gives
// the row's log-sum-exp and entropy (the sums in ascending a, as the forward forms them); categorical_dlogit one component.
// Shared by categorical_bwd_kernel (losses.hip) and the fused head backward (igemm.hip: policy_heads_bwd_kernel).
__device__ __forceinline__ void categorical_row_stats(const float* x, int A, float* lse_out, float* ent_out) {
  float m = x[0];
  for (int a = 1; a < A; ++a) m = fmaxf(m, x[a]);
  float se = 0.f;
  for (int a = 0; a < A; ++a) se += expf(x[a] - m);
  const float lse = m + logf(se);
  float ent = 0.f;
  for (int a = 0; a < A; ++a) { const float lp = x[a] - lse; ent -= expf(lp) * lp; }
  *lse_out = lse;
  *ent_out = ent;
}
__device__ __forceinline__ float categorical_dlogit(float xa, float lse, float ent, bool is_action, float gl, float ge) {
  const float lp = xa - lse, p = expf(lp);
  return gl * ((is_action ? 1.f : 0.f) - p) - ge * p * (lp + ent);
}

// ------------------------------------------------------------------------------------------------
// XCD-aware workgroup order.  MI355X dispatches the workgroups of a launch round-robin over its 8 XCDs (blockIdx mod 8;
// wgs_per_xcd in every phase trace under profiles/) and every XCD has its own L2: with the natural (sample-major) block
// order the 8-13 workgroups that share one sample's operands land on 8 different XCDs and every L2 fetches that sample
// from the fabric -- conv2's backward launch FETCHED 14.2 MB for 2.4 MB of distinct inputs (profiles/r03e_pmc_traffic_*).
// xcd_order() renumbers the workgroups so that a whole sharing group (all workgroups of one sample / one K slice) runs
// on ONE XCD: workgroup `bid` (first = index of the role's first workgroup in the launch) works on the returned
// virtual index of the natural order.  n_groups groups of per_group workgroups; groups beyond a multiple of 8 keep the
// natural order.  A bijection on [0, n_groups * per_group).
constexpr int kXcds = 8;
__device__ __forceinline__ int xcd_order(int bid, int first, int n_groups, int per_group) {
  const int gpx = n_groups / kXcds;                 // whole groups per XCD
  const int main = gpx * kXcds * per_group;
  if (bid >= main) return bid;
  const int xcd = (bid + first) & (kXcds - 1), j = bid >> 3;      // j < gpx * per_group
  return (xcd * gpx + j / per_group) * per_group + (j % per_group);
}
// (the DRA_XCD_ORDER=0 A/B switch of round 4 is retired: the XCD-aware order is the only one)
static constexpr int dra_xcd_order_enabled() { return 1; }

// ------------------------------------------------------------------------------------------------
// Phase trace (measurement aid, compiled only into libdeeprl_amd_trace.so: `make trace`, -DDRA_TRACE).
// Thread 0 of every workgroup writes a constant-rate (s_memrealtime) time stamp at up to 8 phase
// boundaries into a per-kernel-family region of a trace buffer; tools/phase_trace.py turns the
// stamps into per-phase durations, workgroup start distributions (rounds) and the XCD / CU each
// workgroup ran on.  The product library has no stamps at all (the macros expand to nothing).
enum { TR_GATHER, TR_CONV1_F, TR_CONV2_F, TR_CONV3_F, TR_FC4_F, TR_HEAD, TR_FC_B, TR_CONV3_B, TR_CONV2_B,
       TR_CONV1_B, TR_NORM, TR_STEP, TR_A_CONV1, TR_A_CONV2, TR_A_CONV3, TR_A_FC4, TR_A_HEAD, TR_REGIONS };
constexpr int kTraceWgs = 4096;   // workgroups recorded per region
#ifdef DRA_TRACE
static __device__ unsigned long long* g_dra_trace = nullptr;   // one copy per translation unit
__device__ __forceinline__ void dra_stamp(int region, int k) {
  unsigned long long* p = g_dra_trace;
  if (p && threadIdx.x == 0) {
    unsigned long long t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
    const unsigned wg = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    if (wg < (unsigned)kTraceWgs) {
      unsigned long long* rec = p + ((size_t)region * kTraceWgs + wg) * 8;
      if (k == 7) {   // last slot also carries where the workgroup ran: [63:48] XCC id, [47:32] HW_ID low bits
        unsigned xcc, hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        rec[6] = ((unsigned long long)(xcc & 0xffffu) << 32) | (hw & 0xffffffffu);
      }
      rec[k == 7 ? 7 : k] = t;
    }
  }
}
// every pending vector-memory operation of the calling wave has completed
__device__ __forceinline__ void dra_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
static int dra_trace_set_local(void* p) {
  unsigned long long* v = reinterpret_cast<unsigned long long*>(p);
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_dra_trace), &v, sizeof(v));
  return (int)e;
}
#define DRA_STAMP(region, k) dra_stamp((region), (k))
#define DRA_STAMP_END(region) do { dra_drain(); dra_stamp((region), 7); } while (0)
#else
#define DRA_STAMP(region, k) ((void)0)
#define DRA_STAMP_END(region) ((void)0)
#endif
