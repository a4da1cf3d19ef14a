// Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, error_if_nonfinite=False) over a
// SegEntry table of fp32 gradients, in two launches of one workgroup per table block (the table
// walk of seg_block.h):
//
//   grad_sqnorm: S = sum v^2 with every square formed and accumulated in fp64 by an explicit
//        fma((double)v, (double)v, acc) (no fp32 overflow: 1e25 has a finite norm; independent of
//        -ffp-contract).  The block partial goes out as an sc1 (write-through) store, the
//        workgroup drains it and draws its two-level arrival ticket (arrival.h); the LAST arriver
//        sums the partials and writes the ClipBlock
//            norm = (float)(sqrt(S) / (double)div)
//            q    = max_norm / (norm + 1e-6f)           (fp32, IEEE division)
//            coef = (q < 1 || q != q) ? q : 1           (a NaN norm gives a NaN coefficient)
//            steps += 1;  clipped += coef != 1
//        and re-arms the ticket (hipGraph-replay safe).  max_norm / div go by value: a captured
//        graph freezes them.
//   grad_scale:  one scalar load of coef per workgroup; coef == 1: return at once, nothing is
//        written (the gradients stay bitwise as they were, -0 and NaN payloads included);
//        otherwise v = v * coef, one fp32 multiply per element.
//
// Two launches because the scale needs the global norm: one launch would need a grid-wide wait.
//
// Summation order (fixed: bitwise reproducible from run to run and under graph replay).
//   thread:    its kSegElems = 8 elements in the order of seg_block.h (a vector entry: the float4
//              q = 0, 1, components 0..3; a scalar entry: q = 0..7); an element past the entry's
//              end counts as 0.
//   wave:      xor butterfly, offsets 32, 16, 8, 4, 2, 1.
//   workgroup: ((w0 + w1) + w2) + w3.
//   grid:      thread t of the last workgroup adds partial[t], partial[t + 256], ... in
//              increasing order; then the wave and workgroup steps above.
// The gradients are read with plain (cached) loads: the P pass or the SGD launch reads them next.
#include <hip/hip_runtime.h>
#include <math.h>

#include "arrival.h"
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

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const SegEntry* __restrict__ ents,
                                                          const int64_t* __restrict__ prefix, int n_ent,
                                                          double* __restrict__ partial, unsigned* __restrict__ ctr,
                                                          ClipBlock* __restrict__ clip, float max_norm, float div) {
  const SegPos p = seg_find(ents, prefix, n_ent, blockIdx.x);
  const SegEntry& E = p.E;
  const float NDP_SEG_GLOBAL* const src = seg_global(E.src);
  float v[kSegElems] = {};  // every load in flight before the first fma
  seg_walk(
      E, p.base,
      [&](int q, int64_t k) __attribute__((always_inline)) {
        const seg_f32x4 t = seg_ld4(src + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * q + j] = t[j];
      },
      [&](int i, int64_t k, bool) __attribute__((always_inline)) { v[i] = src[k]; });
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < kSegElems; ++i) acc = fma((double)v[i], (double)v[i], acc);
  __shared__ double red[4];
  __shared__ int last;
  const double bsum = clip_block_sum(acc, red);
  if (threadIdx.x == 0) {
    // sc1 (write-through) store, drained before the ticket: read back by the last workgroup
    __hip_atomic_store(partial + blockIdx.x, bsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = arrive_last_grouped(ctr);
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
    arrive_rearm(ctr);
  }
}

__global__ __launch_bounds__(256) void grad_scale_kernel(const SegEntry* __restrict__ ents,
                                                         const int64_t* __restrict__ prefix, int n_ent,
                                                         const ClipBlock* __restrict__ clip) {
  const float coef = clip->coef;  // uniform address: one scalar load
  if (coef == 1.0f) return;
  const SegPos p = seg_find(ents, prefix, n_ent, blockIdx.x);
  const SegEntry& E = p.E;
  const float NDP_SEG_GLOBAL* const src = seg_global(E.src);
  float NDP_SEG_GLOBAL* const dst = seg_global(E.dst);
  seg_walk(
      E, p.base,
      [&](int, int64_t k) __attribute__((always_inline)) {
        seg_f32x4 v = seg_ld4(src + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = __fmul_rn(v[j], coef);
        seg_st4(dst + k, v);
      },
      [&](int, int64_t k, bool) __attribute__((always_inline)) { dst[k] = __fmul_rn(src[k], coef); });
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
