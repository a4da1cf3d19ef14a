// Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, error_if_nonfinite=False) over a
// SegEntry table of fp32 gradients, in two launches of one workgroup per table block
// (kSegBlockElems = 2048 elements, the block -> entry search of seg_block.h):
//
//   grad_sqnorm: S = sum v^2 with every square formed and accumulated in fp64 by an explicit
//        fma((double)v, (double)v, acc) (no fp32 overflow: 1e25 has a finite norm; independent of
//        -ffp-contract).  The block partial goes out as an sc1 (write-through) store, the
//        workgroup drains it and draws an arrival ticket; the LAST arriver (the loss.hip idiom:
//        no fence, no workgroup ever waits for another, no floating-point atomic) sums the
//        partials and writes the ClipBlock
//            norm = (float)(sqrt(S) / (double)div)
//            q    = max_norm / (norm + 1e-6f)           (fp32, IEEE division)
//            coef = (q < 1 || q != q) ? q : 1           (a NaN norm gives a NaN coefficient)
//            steps += 1;  clipped += coef != 1
//        and re-arms the ticket (hipGraph-replay safe).  max_norm / div go by value: a captured
//        graph freezes them.
//        The ticket has two levels: kClipGroup consecutive workgroups share a first-level
//        counter, and the last of a group draws the top-level one.  Agent-scope atomics on ONE
//        address retire at about 13 ns each (measured with a single counter: 78 us for
//        ResNet-18's 5708 workgroups, 423 us for DistilBERT's 32693, whatever the bytes), several
//        times the read itself; the groups' counters lie 256 B apart and proceed in parallel.
//   grad_scale:  one scalar load of coef per workgroup; coef == 1: return at once, nothing is
//        written (the gradients stay bitwise as they were, -0 and NaN payloads included);
//        otherwise v = v * coef, one fp32 multiply per element.
//
// Two launches because the scale needs the global norm: one launch would need a grid-wide wait.
//
// Summation order (fixed: bitwise reproducible from run to run and under graph replay).
//   thread:    a vector entry (src 16-byte aligned): for q = 0, 1 the float4 at element
//              base + (q*256 + tid)*4, components 0..3 in order (a float4 that crosses the
//              entry's end: its in-range components, in order);  a scalar entry: for q = 0..7 the
//              element base + q*256 + tid.  base = (blk - first block of the entry) * 2048.
//   wave:      xor butterfly, offsets 32, 16, 8, 4, 2, 1.
//   workgroup: ((w0 + w1) + w2) + w3.
//   grid:      thread t of the last workgroup adds partial[t], partial[t + 256], ... in
//              increasing order; then the wave and workgroup steps above.
// The gradients are read with plain (cached) loads: the P pass or the SGD launch reads them next.
#include <hip/hip_runtime.h>
#include <math.h>

#include "ndp_kernels.h"
#include "seg_block.h"

namespace ndp {

__device__ __forceinline__ double clip_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ((w0 + w1) + w2) + w3 of the workgroup's wave sums; the value is valid on thread 0
__device__ __forceinline__ double clip_block_sum(double v, double* red) {
  v = clip_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ int clip_find_entry(const int64_t* __restrict__ prefix, int n_ent, int64_t blk) {
  int lo = 0, hi = n_ent - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const SegEntry* __restrict__ ents,
                                                          const int64_t* __restrict__ prefix, int n_ent,
                                                          double* __restrict__ partial, unsigned* __restrict__ ctr,
                                                          ClipBlock* __restrict__ clip, float max_norm, float div) {
  const int64_t blk = blockIdx.x;
  const int lo = clip_find_entry(prefix, n_ent, blk);
  const SegEntry E = ents[lo];
  const float NDP_SEG_GLOBAL* const src = (const float NDP_SEG_GLOBAL*)E.src;
  const int64_t base = (blk - prefix[lo]) * kSegBlockElems;
  double acc = 0.0;
  if (E.vec) {
    constexpr int QN = kSegBlockElems / 1024;
    seg_f32x4 v[QN];
#pragma unroll
    for (int q = 0; q < QN; ++q) {  // both loads in flight before the first fma
      const int64_t k = base + (int64_t)(q * 256 + threadIdx.x) * 4;
      if (k + 3 < E.numel) {
        v[q] = seg_ld4(src + k);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[q][j] = k + j < E.numel ? src[k + j] : 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < QN; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = fma((double)v[q][j], (double)v[q][j], acc);
  } else {
    constexpr int QS = kSegBlockElems / 256;
    float v[QS];
#pragma unroll
    for (int q = 0; q < QS; ++q) {
      const int64_t k = base + q * 256 + threadIdx.x;
      v[q] = k < E.numel ? src[k] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < QS; ++q) acc = fma((double)v[q], (double)v[q], acc);
  }
  __shared__ double red[4];
  __shared__ int last;
  const double bsum = clip_block_sum(acc, red);
  if (threadIdx.x == 0) {
    // sc1 (write-through) store, drained before the ticket: read back by the last workgroup
    __hip_atomic_store(partial + blk, bsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // first-level ticket of this group of kClipGroup workgroups; its last arriver re-arms it
    // (every member has arrived) and draws the top-level ticket.  Causality runs through the
    // atomics: a partial is in memory before its workgroup's ticket, that before the group's last.
    const unsigned n = gridDim.x, g = blockIdx.x / kClipGroup;
    const unsigned members = min((unsigned)kClipGroup, n - g * kClipGroup);
    unsigned* const gctr = ctr + (size_t)(1 + g) * kClipCtrStride;
    int l = 0;
    if (__hip_atomic_fetch_add(gctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == members - 1) {
      __hip_atomic_store(gctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned groups = (n + kClipGroup - 1) / kClipGroup;
      l = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == groups - 1;
    }
    last = l;
  }
  __syncthreads();
  if (!last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // compiler order only: the loads below are sc1
  double a = 0.0;
  constexpr int kBatch = 8;  // loads in flight per thread; the adds keep increasing index order
  for (unsigned r0 = threadIdx.x; r0 < gridDim.x; r0 += 256 * kBatch) {
    double t[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const unsigned r = r0 + 256 * j;
      t[j] = r < gridDim.x ? __hip_atomic_load(partial + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) a += t[j];  // + 0.0 past the end is exact: a partial is >= +0 or NaN
  }
  const double S = clip_block_sum(a, red);  // red: every thread passed the barrier above after reading it
  if (threadIdx.x == 0) {
    const float norm = (float)(sqrt(S) / (double)div);
    const float q = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));
    const float coef = (q < 1.0f || q != q) ? q : 1.0f;
    clip->norm = norm;
    clip->coef = coef;
    clip->steps += 1u;
    if (coef != 1.0f) clip->clipped += 1u;
    __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(256) void grad_scale_kernel(const SegEntry* __restrict__ ents,
                                                         const int64_t* __restrict__ prefix, int n_ent,
                                                         const ClipBlock* __restrict__ clip) {
  const float coef = clip->coef;  // uniform address: one scalar load
  if (coef == 1.0f) return;
  const int64_t blk = blockIdx.x;
  const int lo = clip_find_entry(prefix, n_ent, blk);
  const SegEntry E = ents[lo];
  const float NDP_SEG_GLOBAL* const src = (const float NDP_SEG_GLOBAL*)E.src;
  float NDP_SEG_GLOBAL* const dst = (float NDP_SEG_GLOBAL*)E.dst;
  const int64_t base = (blk - prefix[lo]) * kSegBlockElems;
  if (E.vec) {
    constexpr int QN = kSegBlockElems / 1024;
#pragma unroll
    for (int q = 0; q < QN; ++q) {
      const int64_t k = base + (int64_t)(q * 256 + threadIdx.x) * 4;
      if (k + 3 < E.numel) {
        seg_f32x4 v = seg_ld4(src + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = __fmul_rn(v[j], coef);
        seg_st4(dst + k, v);
      } else {
        for (int j = 0; j < 4 && k + j < E.numel; ++j) dst[k + j] = __fmul_rn(src[k + j], coef);
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < kSegBlockElems / 256; ++q) {
      const int64_t k = base + q * 256 + threadIdx.x;
      if (k < E.numel) dst[k] = __fmul_rn(src[k], coef);
    }
  }
}

void launch_grad_sqnorm(const SegEntry* entries, const int64_t* block_prefix, int n_entries, int64_t n_blocks,
                        double* partial, unsigned* ctr, ClipBlock* clip, float max_norm, float div, hipStream_t s) {
  if (n_entries <= 0 || n_blocks <= 0) return;
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, entries, block_prefix,
                     n_entries, partial, ctr, clip, max_norm, div);
}

void launch_grad_scale(const SegEntry* entries, const int64_t* block_prefix, int n_entries, int64_t n_blocks,
                       const ClipBlock* clip, hipStream_t s) {
  if (n_entries <= 0 || n_blocks <= 0) return;
  hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, entries, block_prefix,
                     n_entries, clip);
}

}  // namespace ndp
