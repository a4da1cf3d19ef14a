// The walk of a SegEntry table, one workgroup (256 threads) per block of kSegBlockElems elements:
// which entry a block belongs to (seg_find), which elements each thread of it owns (seg_walk), and
// the segmented reduce-copy over them (seg_reduce_block: multitensor.hip's seg_reduce_kernel and
// the extra blocks of the PowerSGD P pass, powersgd.hip, which pack the rank-1 group into the comm
// buffer in the same launch).  gradclip.hip and ema.hip say what happens to an element; the
// addressing is here only.
//
// A thread's elements, in the order every kernel keeps (it fixes the summation order of
// grad_sqnorm), with base = (blk - first block of the entry) * kSegBlockElems:
//   vector entry (E.vec: 16-byte aligned): for q = 0, 1 the float4 at element
//                 base + (q*256 + tid)*4, components 0..3 in order; of a float4 that crosses the
//                 entry's end, its in-range components, in order, one by one;
//   scalar entry: for q = 0..7 the element base + q*256 + tid.
#pragma once
#include <hip/hip_runtime.h>
#include "ndp_kernels.h"

namespace ndp {

constexpr int kSegQuads = kSegBlockElems / 1024;  // float4 slots of a thread (vector entry)
constexpr int kSegElems = kSegBlockElems / 256;   // elements of a thread (either kind of entry)

typedef float seg_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned seg_u32x4 __attribute__((ext_vector_type(4)));
// the entry table's pointers, re-typed as global (address space 1): read through the table they
// would compile to FLAT accesses, which also wait on the scalar-cache counter
#define NDP_SEG_GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ T NDP_SEG_GLOBAL* seg_global(T* p) {
  return (T NDP_SEG_GLOBAL*)p;
}
__device__ __forceinline__ seg_f32x4 seg_ld4(const float NDP_SEG_GLOBAL* p) {
  return *reinterpret_cast<const seg_f32x4 NDP_SEG_GLOBAL*>(p);
}
__device__ __forceinline__ void seg_st4(float NDP_SEG_GLOBAL* p, seg_f32x4 v) {
  *reinterpret_cast<seg_f32x4 NDP_SEG_GLOBAL*>(p) = v;
}

// block `blk` of the table: its entry (index and copy) and its first element within that entry.
// The entry is fetched here, ahead of the first use of prefix[ent]: in this order the two scalar
// loads share one round trip (base first costs every workgroup a second one: measured, +0.25 us on
// grad_sqnorm over ResNet-18's 5708 blocks).
struct SegPos {
  int ent;
  int64_t base;
  SegEntry E;
};
__device__ __forceinline__ SegPos seg_find(const SegEntry* __restrict__ ents, const int64_t* __restrict__ prefix,
                                           int n_ent, int64_t blk) {
  int lo = 0, hi = n_ent - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= blk) lo = mid; else hi = mid - 1;
  }
  const SegEntry E = ents[lo];
  return {lo, (blk - prefix[lo]) * kSegBlockElems, E};
}

// first element of float4 slot q / element of scalar slot q of this thread
__device__ __forceinline__ int64_t seg_quad_at(int64_t base, int q) {
  return base + (int64_t)(q * 256 + threadIdx.x) * 4;
}
__device__ __forceinline__ int64_t seg_elem_at(int64_t base, int q) { return base + q * 256 + threadIdx.x; }

// This thread's elements of the block at `base`, in the order above:
//   quad(q, k)        float4 slot q, wholly inside the entry, at element k;
//   elem(i, k, tail)  the single element k, the i-th of the thread's kSegElems: a component of a
//                     float4 that crosses the entry's end (tail: i = 4*q + component) or slot
//                     i = q of a scalar entry (!tail).  `tail` is a constant after inlining.
// Everything is unrolled, so a kernel can keep per-slot values in register arrays indexed by q / i
// between two walks of the same block.
template <class Quad, class Elem>
__device__ __forceinline__ void seg_walk(const SegEntry& E, int64_t base, Quad&& quad, Elem&& elem) {
  if (E.vec) {
#pragma unroll
    for (int q = 0; q < kSegQuads; ++q) {
      const int64_t k = seg_quad_at(base, q);
      if (k + 3 < E.numel) {
        quad(q, k);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k + j < E.numel) elem(4 * q + j, k + j, true);
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < kSegElems; ++q) {
      const int64_t k = seg_elem_at(base, q);
      if (k < E.numel) elem(q, k, false);
    }
  }
}

// dst[k] = (sum_c src[c*stride + k]) / div over block `blk`, the adds in chunk order
__device__ __forceinline__ void seg_reduce_block(const SegEntry* __restrict__ ents,
                                                 const int64_t* __restrict__ prefix, int n_ent, int64_t blk) {
  const SegPos p = seg_find(ents, prefix, n_ent, blk);
  const SegEntry& E = p.E;
  const float NDP_SEG_GLOBAL* const src = seg_global(E.src);
  float NDP_SEG_GLOBAL* const dst = seg_global(E.dst);
  const bool scale = E.div != 1.0f;
  // an element on its own: a scalar entry's, or of the float4 that crosses a vector entry's end
  auto one = [&](int64_t k) __attribute__((always_inline)) {
    float t = src[k];
    for (int c = 1; c < E.chunks; ++c) t += src[(int64_t)c * E.stride + k];
    if (scale) t = t / E.div;
    dst[k] = t;
  };
  if (E.vec) {
    // Split-K P / Q slabs (up to ~20 chunks): the chunk loads are issued kSegBatch at a time
    // for both float4 of the thread before any add, so a block costs ~chunks / 8 memory
    // round trips instead of one per chunk (the adds keep chunk order: bitwise unchanged).
    constexpr int kSegBatch = 8;
    const seg_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    int64_t kq[kSegQuads];
    bool full[kSegQuads];
    seg_f32x4 acc[kSegQuads];
#pragma unroll
    for (int q = 0; q < kSegQuads; ++q) {
      kq[q] = seg_quad_at(p.base, q);
      full[q] = kq[q] + 3 < E.numel;
      acc[q] = full[q] ? seg_ld4(src + kq[q]) : zero;
    }
    int c = 1;
    for (; c + kSegBatch <= E.chunks; c += kSegBatch) {
      seg_f32x4 t[kSegQuads][kSegBatch];
#pragma unroll
      for (int j = 0; j < kSegBatch; ++j)
#pragma unroll
        for (int q = 0; q < kSegQuads; ++q)
          t[q][j] = full[q] ? seg_ld4(src + (int64_t)(c + j) * E.stride + kq[q]) : zero;
#pragma unroll
      for (int q = 0; q < kSegQuads; ++q)
#pragma unroll
        for (int j = 0; j < kSegBatch; ++j) acc[q] += t[q][j];
    }
    for (; c < E.chunks; ++c)
#pragma unroll
      for (int q = 0; q < kSegQuads; ++q)
        if (full[q]) acc[q] += seg_ld4(src + (int64_t)c * E.stride + kq[q]);
#pragma unroll
    for (int q = 0; q < kSegQuads; ++q) {
      if (full[q]) {
        if (scale) acc[q] = acc[q] / E.div;
        seg_st4(dst + kq[q], acc[q]);
      } else {
        for (int j = 0; j < 4 && kq[q] + j < E.numel; ++j) one(kq[q] + j);
      }
    }
  } else {
    for (int q = 0; q < kSegElems; ++q) {
      const int64_t k = seg_elem_at(p.base, q);
      if (k >= E.numel) break;
      one(k);
    }
  }
}

}  // namespace ndp
