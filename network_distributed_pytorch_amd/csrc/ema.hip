// Exponential moving average of the weights (torch.optim.swa_utils.AveragedModel with
// get_ema_multi_avg_fn, timm's ModelEmaV2) over a SegEntry table with src = live tensor x_i and
// dst = shadow s_i, one workgroup per table block (the table walk of seg_block.h), in ONE launch
// whose step-dependent decay lives on the device, so one captured graph serves every step.
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
//   it), BEFORE thread 0 draws the workgroup's two-level arrival ticket (arrival.h): every wave
//   needs n for its own stores, and none reads the block itself, so the workgroup has n before it
//   draws.  The block is written by the last arriver only, after every ticket is drawn.  So no
//   workgroup can see n + 1.  Nothing of a workgroup's stores is read by another: no drain.
//
//   Loads and stores.  x is read with plain (cached) loads: the next forward reads it.  s is
//   touched once per step: non-temporal loads and stores, as the momentum in psgd_update /
//   sgd_momentum_vec_kernel.  The kernel writes the shadow, the block and the tickets, nothing
//   else.
//
//   ema_swap: same table, x_i <-> s_i element by element as 32-bit words (NaN payloads and -0
//               survive; twice is the identity).  Evaluation runs on the averaged weights
//               without a second copy of the model.
#include <hip/hip_runtime.h>

#include "arrival.h"
#include "ndp_kernels.h"
#include "seg_block.h"

namespace ndp {

// s + w * (x - s) in three rounded operations; the empty asm keeps u out of an fma
__device__ __forceinline__ float ema_elem(float x, float s, float w) {
  const float t = __fsub_rn(x, s);
  float u = __fmul_rn(w, t);
  asm volatile("" : "+v"(u));
  return __fadd_rn(s, u);
}

__global__ __launch_bounds__(256) void ema_update_kernel(const SegEntry* __restrict__ ents,
                                                         const int64_t* __restrict__ prefix, int n_ent,
                                                         unsigned* __restrict__ ctr, EmaBlock* __restrict__ block,
                                                         float decay, int warmup) {
  // one scalar load per workgroup, by the wave that later draws the ticket; the other waves get n
  // through LDS, so no wave of this workgroup reads the block after the draw
  __shared__ unsigned n_sh;
  if (threadIdx.x == 0) n_sh = block->updates;
  const SegPos p = seg_find(ents, prefix, n_ent, blockIdx.x);
  const SegEntry& E = p.E;
  const float NDP_SEG_GLOBAL* const src = seg_global(E.src);
  float NDP_SEG_GLOBAL* const dst = seg_global(E.dst);
  // every full float4 and every scalar slot in flight before the barrier; the components of a
  // float4 that crosses the entry's end are loaded in the store phase
  float xs[kSegElems], ss[kSegElems];  // by position in the thread's order: float4 q is [4q, 4q + 4)
  seg_walk(
      E, p.base,
      [&](int q, int64_t k) __attribute__((always_inline)) {
        const seg_f32x4 xv = seg_ld4(src + k);
        const seg_f32x4 sv = __builtin_nontemporal_load(reinterpret_cast<const seg_f32x4 NDP_SEG_GLOBAL*>(dst + k));
#pragma unroll
        for (int j = 0; j < 4; ++j) xs[4 * q + j] = xv[j], ss[4 * q + j] = sv[j];
      },
      [&](int i, int64_t k, bool tail) __attribute__((always_inline)) {
        if (tail) return;
        xs[i] = src[k];
        ss[i] = __builtin_nontemporal_load(dst + k);
      });
  __syncthreads();
  const unsigned n = n_sh;
  float d = decay;
  if (warmup) {
    const float fn = (float)n;
    d = fminf(decay, __fdiv_rn(__fadd_rn(fn, 1.0f), __fadd_rn(fn, 10.0f)));
  }
  const float w = __fsub_rn(1.0f, d);
  seg_walk(
      E, p.base,
      [&](int q, int64_t k) __attribute__((always_inline)) {
        seg_f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = ema_elem(xs[4 * q + j], ss[4 * q + j], w);
        __builtin_nontemporal_store(r, reinterpret_cast<seg_f32x4 NDP_SEG_GLOBAL*>(dst + k));
      },
      [&](int i, int64_t k, bool tail) __attribute__((always_inline)) {
        const float x = tail ? src[k] : xs[i];
        const float s = tail ? __builtin_nontemporal_load(dst + k) : ss[i];
        __builtin_nontemporal_store(ema_elem(x, s, w), dst + k);
      });
  if (threadIdx.x != 0 || !arrive_last_grouped(ctr)) return;
  // last arriver: every workgroup has drawn its ticket, hence read n
  block->decay = d;
  block->weight = w;
  block->updates = n + 1u;
  arrive_rearm(ctr);
}

__global__ __launch_bounds__(256) void ema_swap_kernel(const SegEntry* __restrict__ ents,
                                                       const int64_t* __restrict__ prefix, int n_ent) {
  const SegPos p = seg_find(ents, prefix, n_ent, blockIdx.x);
  const SegEntry& E = p.E;
  // both sides are read and written: the table's src is written here, as 32-bit words
  unsigned NDP_SEG_GLOBAL* const a = seg_global((unsigned*)E.src);
  unsigned NDP_SEG_GLOBAL* const b = seg_global((unsigned*)E.dst);
  seg_walk(
      E, p.base,
      [&](int, int64_t k) __attribute__((always_inline)) {
        const seg_u32x4 va = *reinterpret_cast<const seg_u32x4 NDP_SEG_GLOBAL*>(a + k);
        const seg_u32x4 vb = *reinterpret_cast<const seg_u32x4 NDP_SEG_GLOBAL*>(b + k);
        *reinterpret_cast<seg_u32x4 NDP_SEG_GLOBAL*>(a + k) = vb;
        *reinterpret_cast<seg_u32x4 NDP_SEG_GLOBAL*>(b + k) = va;
      },
      [&](int, int64_t k, bool) __attribute__((always_inline)) {
        const unsigned va = a[k], vb = b[k];
        a[k] = vb;
        b[k] = va;
      });
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
