// Exponential moving average of the weights (torch.optim.swa_utils.AveragedModel with
// get_ema_multi_avg_fn, timm's ModelEmaV2) over a SegEntry table with src = live tensor x_i and
// dst = shadow s_i, one workgroup per table block (kSegBlockElems = 2048 elements, the
// block -> entry search of seg_block.h), in ONE launch whose step-dependent decay lives on the
// device, so one captured graph serves every step.
//
//   ema_update: n = block.updates (runs before this one);
//                 d = warmup ? min(decay, (n + 1) / (n + 10)) : decay     (fp32, IEEE division,
//                                                                          (float)n to nearest)
//                 w = 1 - d
//               every element:  t = x - s;  u = w * t;  s' = s + u       -- three single,
//               correctly rounded fp32 operations.  The build uses -ffp-contract=fast: u passes
//               an empty asm (the image_mix_batch_kernel idiom), so it is never contracted into
//               fma(w, t, s), which is a different rule.  Consequences: x == s keeps s; a
//               shared -0 becomes +0; x = s = inf gives NaN.
//               Exactly once per run the block gets decay = d, weight = w, updates = n + 1.
//
//   Who writes the block.  n is read with one scalar load per workgroup, by thread 0, and handed
//   to the other waves through LDS behind the one barrier (the element loads are issued ahead of
//   it), BEFORE thread 0 draws the workgroup's arrival ticket: every wave needs n for its own
//   stores, and none reads the block itself, so the workgroup has n before it draws.  The block
//   is written by the last arriver only, through the two-level ticket of
//   grad_sqnorm_kernel (kClipGroup workgroups share a first-level counter kClipCtrStride words
//   apart, the last of a group draws the top-level one; both re-armed, so hipGraph-replay safe),
//   and the last arriver writes only after every ticket is drawn.  So no workgroup can see
//   n + 1, no workgroup waits for another, and there is no floating-point atomic.  The ticket
//   lines are a copy of gradclip.hip's (no partial to drain here), so that file's code is
//   untouched.
//
//   Loads and stores.  x is read with plain (cached) loads: the next forward reads it.  s is
//   touched once per step: non-temporal loads and stores, as the momentum in psgd_update /
//   sgd_momentum_vec_kernel.  A vector entry (src and dst both 16-byte aligned) moves float4;
//   a float4 that crosses the entry's end handles its in-range components only; every other
//   entry takes the scalar path.  The kernel writes the shadow, the block and the tickets,
//   nothing else.
//
//   ema_swap: same table, x_i <-> s_i element by element as 32-bit words (NaN payloads and -0
//               survive; twice is the identity).  Evaluation runs on the averaged weights
//               without a second copy of the model.
#include <hip/hip_runtime.h>

#include "ndp_kernels.h"
#include "seg_block.h"

namespace ndp {

typedef unsigned ema_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int ema_find_entry(const int64_t* __restrict__ prefix, int n_ent, int64_t blk) {
  int lo = 0, hi = n_ent - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// s + w * (x - s) in three rounded operations; the empty asm keeps u out of an fma
__device__ __forceinline__ float ema_elem(float x, float s, float w) {
  const float t = __fsub_rn(x, s);
  float u = __fmul_rn(w, t);
  asm volatile("" : "+v"(u));
  return __fadd_rn(s, u);
}

// barrier (the element loads are already in flight), n from LDS, then the schedule
__device__ __forceinline__ float ema_weight(const unsigned* n_sh, float decay, int warmup, unsigned* n_out,
                                            float* d_out) {
  __syncthreads();
  const unsigned n = *n_sh;
  float d = decay;
  if (warmup) {
    const float fn = (float)n;
    d = fminf(decay, __fdiv_rn(__fadd_rn(fn, 1.0f), __fadd_rn(fn, 10.0f)));
  }
  *n_out = n;
  *d_out = d;
  return __fsub_rn(1.0f, d);
}

__global__ __launch_bounds__(256) void ema_update_kernel(const SegEntry* __restrict__ ents,
                                                         const int64_t* __restrict__ prefix, int n_ent,
                                                         unsigned* __restrict__ ctr, EmaBlock* __restrict__ block,
                                                         float decay, int warmup) {
  // one scalar load per workgroup, by the wave that later draws the ticket; the other waves get n
  // through LDS, so no wave of this workgroup reads the block after the draw
  __shared__ unsigned n_sh;
  if (threadIdx.x == 0) n_sh = block->updates;
  const int64_t blk = blockIdx.x;
  const int lo = ema_find_entry(prefix, n_ent, blk);
  const SegEntry E = ents[lo];
  const float NDP_SEG_GLOBAL* const src = (const float NDP_SEG_GLOBAL*)E.src;
  float NDP_SEG_GLOBAL* const dst = (float NDP_SEG_GLOBAL*)E.dst;
  const int64_t base = (blk - prefix[lo]) * kSegBlockElems;
  unsigned n;
  float d;
  if (E.vec) {
    constexpr int QN = kSegBlockElems / 1024;
    seg_f32x4 xv[QN], sv[QN];
    int64_t kq[QN];
#pragma unroll
    for (int q = 0; q < QN; ++q) {  // every full load in flight before the first store
      kq[q] = base + (int64_t)(q * 256 + threadIdx.x) * 4;
      if (kq[q] + 3 < E.numel) {
        xv[q] = seg_ld4(src + kq[q]);
        sv[q] = __builtin_nontemporal_load(reinterpret_cast<const seg_f32x4 NDP_SEG_GLOBAL*>(dst + kq[q]));
      }
    }
    const float w = ema_weight(&n_sh, decay, warmup, &n, &d);
#pragma unroll
    for (int q = 0; q < QN; ++q) {
      const int64_t k = kq[q];
      if (k + 3 < E.numel) {
        seg_f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = ema_elem(xv[q][j], sv[q][j], w);
        __builtin_nontemporal_store(r, reinterpret_cast<seg_f32x4 NDP_SEG_GLOBAL*>(dst + k));
      } else {
        for (int j = 0; j < 4 && k + j < E.numel; ++j) {
          const float s = __builtin_nontemporal_load(dst + k + j);
          __builtin_nontemporal_store(ema_elem(src[k + j], s, w), dst + k + j);
        }
      }
    }
  } else {
    constexpr int QS = kSegBlockElems / 256;
    float xs[QS], ss[QS];
#pragma unroll
    for (int q = 0; q < QS; ++q) {
      const int64_t k = base + q * 256 + threadIdx.x;
      if (k < E.numel) {
        xs[q] = src[k];
        ss[q] = __builtin_nontemporal_load(dst + k);
      }
    }
    const float w = ema_weight(&n_sh, decay, warmup, &n, &d);
#pragma unroll
    for (int q = 0; q < QS; ++q) {
      const int64_t k = base + q * 256 + threadIdx.x;
      if (k < E.numel) __builtin_nontemporal_store(ema_elem(xs[q], ss[q], w), dst + k);
    }
  }
  if (threadIdx.x != 0) return;
  // the two-level arrival ticket of grad_sqnorm_kernel (gradclip.hip): nothing of this
  // workgroup's stores is read by another, so no drain; n was read above, before the draw
  const unsigned nb = gridDim.x, g = blockIdx.x / kClipGroup;
  const unsigned members = min((unsigned)kClipGroup, nb - g * kClipGroup);
  unsigned* const gctr = ctr + (size_t)(1 + g) * kClipCtrStride;
  if (__hip_atomic_fetch_add(gctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != members - 1) return;
  __hip_atomic_store(gctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned groups = (nb + kClipGroup - 1) / kClipGroup;
  if (__hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != groups - 1) return;
  // last arriver: every workgroup has drawn its ticket, hence read n
  block->decay = d;
  block->weight = __fsub_rn(1.0f, d);
  block->updates = n + 1u;
  __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void ema_swap_kernel(const SegEntry* __restrict__ ents,
                                                       const int64_t* __restrict__ prefix, int n_ent) {
  const int64_t blk = blockIdx.x;
  const int lo = ema_find_entry(prefix, n_ent, blk);
  const SegEntry E = ents[lo];
  // both sides are read and written: the table's src is written here, as 32-bit words
  unsigned NDP_SEG_GLOBAL* const a = (unsigned NDP_SEG_GLOBAL*)E.src;
  unsigned NDP_SEG_GLOBAL* const b = (unsigned NDP_SEG_GLOBAL*)E.dst;
  const int64_t base = (blk - prefix[lo]) * kSegBlockElems;
  if (E.vec) {
#pragma unroll
    for (int q = 0; q < kSegBlockElems / 1024; ++q) {
      const int64_t k = base + (int64_t)(q * 256 + threadIdx.x) * 4;
      if (k + 3 < E.numel) {
        const ema_u32x4 va = *reinterpret_cast<const ema_u32x4 NDP_SEG_GLOBAL*>(a + k);
        const ema_u32x4 vb = *reinterpret_cast<const ema_u32x4 NDP_SEG_GLOBAL*>(b + k);
        *reinterpret_cast<ema_u32x4 NDP_SEG_GLOBAL*>(a + k) = vb;
        *reinterpret_cast<ema_u32x4 NDP_SEG_GLOBAL*>(b + k) = va;
      } else {
        for (int j = 0; j < 4 && k + j < E.numel; ++j) {
          const unsigned va = a[k + j], vb = b[k + j];
          a[k + j] = vb;
          b[k + j] = va;
        }
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < kSegBlockElems / 256; ++q) {
      const int64_t k = base + q * 256 + threadIdx.x;
      if (k < E.numel) {
        const unsigned va = a[k], vb = b[k];
        a[k] = vb;
        b[k] = va;
      }
    }
  }
}

void launch_ema_update(const SegEntry* entries, const int64_t* block_prefix, int n_entries, int64_t n_blocks,
                       unsigned* ctr, EmaBlock* block, float decay, int warmup, hipStream_t s) {
  if (n_entries <= 0 || n_blocks <= 0) return;
  hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, entries, block_prefix,
                     n_entries, ctr, block, decay, warmup);
}

void launch_ema_swap(const SegEntry* entries, const int64_t* block_prefix, int n_entries, int64_t n_blocks,
                     hipStream_t s) {
  if (n_entries <= 0 || n_blocks <= 0) return;
  hipLaunchKernelGGL(ema_swap_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, entries, block_prefix, n_entries);
}

}  // namespace ndp
