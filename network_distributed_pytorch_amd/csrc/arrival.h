// Last-arriver tickets: the workgroups of one launch each draw a ticket from a zeroed counter when
// their part is done, and the one that draws the last ticket finishes the job (sums the partials,
// writes the result block).  No workgroup ever waits for another, and there is no floating-point
// atomic: the last arriver adds in a fixed order, so the result is bitwise reproducible.
//
//   No release / acquire fence.  What crosses workgroups goes out as sc1 (write-through) stores
//   (__hip_atomic_store, relaxed, agent scope) and is read back with agent-scope loads; an
//   agent-scope release would write the XCD's whole L2 back (ce_fwd: 11.2 -> 10.0 us at batch 512
//   without it).  Causality runs through the atomics: the stores are DRAINED (s_waitcnt vmcnt(0))
//   before the ticket is drawn, so a partial is in memory before its workgroup's ticket, and that
//   before the last one.  The last arriver's fence is wavefront scope: compiler order only.
//   Re-arming.  The last arriver stores 0 into the counter when it is done, so the next launch, or
//   the next replay of a captured graph, finds it zeroed.
//   Two levels.  Agent-scope atomics on ONE address retire at about 13 ns each (measured with a
//   single counter: 78 us for ResNet-18's 5708 workgroups, 423 us for DistilBERT's 32693, whatever
//   the bytes).  So kArriveGroup consecutive workgroups share a first-level counter, and the last
//   of a group draws the top-level one; the counters lie kArriveCtrStride words (256 B) apart,
//   never in one cache line, and proceed in parallel.
//
// Left alone, because they are other protocols: last_arrival in powersgd.hip is a monotonic modulo
// counter that is never re-armed; the waits in batchnorm.hip (SPLIT > 1) and orth.hip are spins,
// not last-arriver tickets.
#pragma once
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

namespace ndp {

constexpr int kArriveGroup = 64;      // workgroups that share one first-level ticket
constexpr int kArriveCtrStride = 64;  // uint32 between two tickets: 256 B apart, never one cache line
// zeroed uint32 words that arrive_last_grouped needs for a grid of n_blocks workgroups
inline int64_t arrive_ctr_words(int64_t n_blocks) {
  return (int64_t)kArriveCtrStride * (1 + (n_blocks + kArriveGroup - 1) / kArriveGroup);
}

#ifdef __HIPCC__
// One level, one zeroed word, called by every thread of every workgroup of a 1-D grid: drains the
// caller's vector stores, draws the ticket and returns to the whole workgroup whether it is the
// last of `total`.  The last workgroup stores 0 into *ctr when it is done.
__device__ __forceinline__ bool arrive_last(unsigned* ctr, unsigned total) {
  __shared__ int last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0)
    last = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == total - 1;
  __syncthreads();
  if (!last) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // compiler order only: the loads that follow are sc1
  return true;
}

// Two levels, arrive_ctr_words(gridDim.x) zeroed words, called by thread 0 of every workgroup of
// a 1-D grid once whatever another workgroup reads is drained: true for the last arriver of the
// grid.  A group's last arriver re-arms its first-level counter (every member has arrived); the
// top-level one is the caller's, by arrive_rearm once its block is written.
__device__ __forceinline__ bool arrive_last_grouped(unsigned* ctr) {
  const unsigned n = gridDim.x, g = blockIdx.x / kArriveGroup;
  const unsigned members = min((unsigned)kArriveGroup, n - g * kArriveGroup);
  unsigned* const gctr = ctr + (size_t)(1 + g) * kArriveCtrStride;
  if (__hip_atomic_fetch_add(gctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != members - 1) return false;
  __hip_atomic_store(gctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned groups = (n + kArriveGroup - 1) / kArriveGroup;
  return __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == groups - 1;
}

__device__ __forceinline__ void arrive_rearm(unsigned* ctr) {
  __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif

}  // namespace ndp
