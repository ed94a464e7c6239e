// Host-side plumbing of learner.hip that no kernel and no stream order depends on: a captured hipGraph with its ready flag, one
// timed replay of it, and a scope that charges its lifetime to a host-time counter.  Host only; nothing here allocates.
// (DESIGN.md "The learner's host plumbing".)
#pragma once
#include "common.h"
#include <chrono>

// A plain aggregate -- the learner is memset to zero after `new`, and a zeroed CachedGraph is an empty one.
struct CachedGraph {
  hipGraphExec_t exec;
  bool ready;

  void reset() {
    if (ready) (void)hipGraphExecDestroy(exec);
    ready = false;
  }

  // Captures body() -- which returns a DRA_* / HIP code -- on `st` (thread-local mode) and instantiates it.  An exec already held
  // is destroyed first; a capture that began is always ended; the hipGraph_t is destroyed on every path; `ready` is set on full
  // success only.  Returns the first failure in the order begin, body, end, instantiate.
  template <class Body>
  int capture(hipStream_t st, Body&& body) {
    reset();
    DRA_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    hipGraph_t graph = nullptr;
    const int rc = body();
    hipError_t e = hipStreamEndCapture(st, &graph);
    if (rc == DRA_OK && e == hipSuccess) {
      e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
      ready = e == hipSuccess;
    }
    if (graph) (void)hipGraphDestroy(graph);
    return rc != DRA_OK ? rc : (int)e;
  }

  int launch(hipStream_t st) const {
    DRA_HIP(hipGraphLaunch(exec, st));
    return DRA_OK;
  }
};

// One replay of `g` on `st` between two timing events; waits for it; *ms = the events' distance.
static inline int timed_replay(const CachedGraph& g, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, float* ms) {
  DRA_HIP(hipEventRecord(ev0, st));
  DRA_HIP(hipGraphLaunch(g.exec, st));
  DRA_HIP(hipEventRecord(ev1, st));
  DRA_HIP(hipEventSynchronize(ev1));
  DRA_HIP(hipEventElapsedTime(ms, ev0, ev1));
  return DRA_OK;
}

// Adds its lifetime (seconds) to a host-time counter, on every way out of the scope.
struct HostTimeScope {
  double& acc;
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit HostTimeScope(double& a) : acc(a) {}
  HostTimeScope(const HostTimeScope&) = delete;
  HostTimeScope& operator=(const HostTimeScope&) = delete;
  ~HostTimeScope() { acc += seconds(); }
  double seconds() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};
