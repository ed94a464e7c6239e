// What the seed-lane launches share (dqn_mlp.hip, dist_mlp.hip; seed_batch.py): n_lanes independent agents of ONE shape as
// workgroups (0, lane) of the same launch.  The arguments are two TABLES of n_lanes structs, read by the host (every lane is checked
// as the single entry checks its arguments, ahead of the launch) AND by the kernels, from the same addresses: pinned host memory
// that the device maps (hipHostMalloc, torch's pin_memory()), where HIP keeps a single launch's kernel arguments as well.  Workgroup
// (0, lane) reads its row of each table (uniform addresses: scalar loads, as the single launch reads its kernel arguments) and runs
// the single launch's text, so a lane carries the single launch's bits.  Lanes share nothing and wait for nobody.
//
// Two forms of a lane kernel (mlp_rollout.h's banner: the figures decide which): a kernel of its own over a __forceinline__ body
// that the single kernel runs too (the acting kernels), or a template flag on the single kernel -- lane_arg<LANES, T> as the
// parameter's type, lane_struct() as its first statement; with LANES false both are the struct itself (the update and the evaluation
// kernels).
//
// What a lane form pays beside its registers: a pointer read out of a table is a GENERIC pointer to the compiler (inside a kernel
// argument it is known to be global), so the accesses through it are flat_load / flat_store, which count against the LDS counter
// too (7-11 us in dist_mlp_update_kernel at one lane, attributed).  A cast to address_space(1) and back, or
// __builtin_assume over __builtin_amdgcn_is_shared / is_private, does not change that with this compiler; only an access THROUGH an
// address_space(1) pointer does.
#pragma once
#include "mlp_rollout.h"
#include <type_traits>

namespace {

constexpr int kMaxLanes = 64;

template <bool LANES, typename T> using lane_arg = std::conditional_t<LANES, const T*, T>;
template <typename T> __device__ __forceinline__ const T& lane_struct(const T& v) { return v; }
template <typename T> __device__ __forceinline__ T lane_struct(const T* table) { return table[blockIdx.y]; }

// KERNEL(nets, ios) as n_lanes workgroups (0, lane) of 256 threads, each with `bytes` of dynamic LDS
template <auto KERNEL, typename Net, typename Io>
int launch_lanes(size_t bytes, const Net* nets, const Io* ios, int n_lanes, void* stream) {
  static DraLdsAttr lds_attr;
  if (int rc = dra_grant_lds(lds_attr, reinterpret_cast<const void*>(KERNEL), bytes)) return rc;
  hipLaunchKernelGGL(KERNEL, dim3(1, (unsigned)n_lanes), dim3(256), bytes, dra_stream(stream), nets, ios);
  DRA_LAUNCH_CHECK();
  return DRA_OK;
}

}  // namespace
