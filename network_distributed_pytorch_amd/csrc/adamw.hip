// AdamW (torch.optim.AdamW: Adam with decoupled weight decay, bias-corrected) over a SegEntry table
// with src = gradient g_i and dst = parameter x_i, one workgroup per table block (the table walk of
// seg_block.h), in ONE launch whose step-dependent bias corrections live on the device, so one
// captured graph serves every step.
//
//   The rule.  fp32 contiguous x_i, g_i, moments m_i, v_i (zero at start); by value beta1, beta2,
//   eps > 0, div >= 1 (frozen into a captured graph); lr, wd from the hyper block [lr, wd, 0, 0]
//   (hyper.h); the 16-byte AdamBlock {b1pow, b2pow, steps, pad} starts as {1, 1, 0, 0}.  Every line
//   is ONE correctly rounded fp32 operation; there is no fused multiply-add anywhere.
//     per launch, from the block as it was before the launch, the same in every workgroup:
//       p1 = b1pow * beta1        p2 = b2pow * beta2      (running products: beta^t without powf,
//       bc1 = 1 - p1              bc2 = 1 - p2             and t never visits the host)
//       ss = lr / bc1             sb = sqrt(bc2)
//       om1 = 1 - beta1           om2 = 1 - beta2
//       c = 1 - lr * wd
//     per element:
//       gg = (div != 1) ? g / div : g
//       x1 = (wd != 0 && the entry decays) ? x * c : x      (decoupled decay; the wd != 0 test is
//                                                            part of the rule, as in hyper.h)
//       m' = (beta1 * m) + (om1 * gg)
//       v' = (beta2 * v) + (om2 * (gg * gg))
//       den = (sqrt(v') / sb) + eps
//       x' = x1 - ss * (m' / den)
//     exactly once per launch the block becomes {p1, p2, steps + 1, 0}.
//   Consequences: g = m = v = 0 leaves x1 as it is (the dense arena's zero padding stays zero, and
//   with wd == 0 a -0 in x survives); NaN and inf propagate as in the torch twin (ops/adamw.py).
//
//   The per-element lines are adamw_elem (adamw_elem.h), which the PowerSGD update kernels that
//   step with AdamW (powersgd.hip) share.
//   Contraction and rounding.  The build uses -ffp-contract=fast: every product that feeds an add
//   or a subtract passes an empty asm (the ema.hip / image_batch.hip idiom) and is never contracted.
//   The divisions are __fdiv_rn, IEEE under hipcc's default correctly rounded divide / sqrt.  The
//   roots are __builtin_sqrtf, which that default also expands to the correctly rounded sequence;
//   __fsqrt_rn is NOT used: in this toolchain's headers it is the native (1 ulp) v_sqrt_f32 unless
//   OCML_BASIC_ROUNDED_OPERATIONS is defined.  fp32 denormals are kept (hipcc's default).
//
//   Addressing.  The table comes from build_adamw_table (plan.cpp), not make_seg_table: `stride`
//   is the entry's element offset into the two moment arenas (base pointers m, v: kernel
//   arguments), bit 0 of `pad` says "no decay", `vec` needs all FOUR streams 16-byte aligned.
//   chunks = 1 and div = 1 always (the by-value div scales the gradient).
//
//   Who writes the block.  Thread 0 reads b1pow / b2pow / steps with scalar loads and hands the
//   two products' inputs to the other waves through LDS behind the workgroup's one barrier (the
//   element loads are issued ahead of it), BEFORE it draws the two-level arrival ticket
//   (arrival.h).  No wave reads the block after the draw, the block is written by the last arriver
//   only, after every ticket is drawn: no workgroup can see steps + 1, none waits for another,
//   there is no floating-point atomic, and the last arriver re-arms the ticket: replay-safe.
//   Nothing of a workgroup's stores is read by another: no drain.
//
//   Loads and stores.  g, m and v are touched once per step: non-temporal loads and stores, as the
//   momentum in sgd_momentum_vec_kernel and the shadow in ema.hip.  x gets plain loads and stores:
//   the next forward reads it.  The kernel writes x, m, v, the block and the tickets; never g.
//
//   Resources (hipcc --offload-arch=gfx950 -O3 -ffp-contract=fast, -Rpass-analysis=kernel-resource-usage,
//   adamw_step_kernel): 68 VGPRs, 0 AGPRs, 44 SGPRs, no scratch (0 bytes/lane, no spills), 8 B of
//   LDS, occupancy 7 waves/SIMD.  The 32 values a thread keeps in flight across the barrier (8
//   elements of g, x, m, v) are half of the VGPRs.
#include <hip/hip_runtime.h>

#include "adamw_elem.h"
#include "arrival.h"
#include "ndp_kernels.h"
#include "seg_block.h"

namespace ndp {

__global__ __launch_bounds__(256) void adamw_step_kernel(const SegEntry* __restrict__ ents,
                                                         const int64_t* __restrict__ prefix, int n_ent,
                                                         unsigned* __restrict__ ctr, AdamBlock* __restrict__ block,
                                                         const float* __restrict__ hyper, float* __restrict__ m_base,
                                                         float* __restrict__ v_base, float beta1, float beta2,
                                                         float eps, float div) {
  // one set of scalar loads per workgroup, by the wave that later draws the ticket; the other
  // waves get the running products through LDS, so no wave reads the block after the draw
  __shared__ float pow_sh[2];
  unsigned steps = 0;
  if (threadIdx.x == 0) {
    pow_sh[0] = block->b1pow;
    pow_sh[1] = block->b2pow;
    steps = block->steps;
  }
  const SegPos p = seg_find(ents, prefix, n_ent, blockIdx.x);
  const SegEntry& E = p.E;
  const float NDP_SEG_GLOBAL* const g = seg_global(E.src);
  float NDP_SEG_GLOBAL* const x = seg_global(E.dst);
  float NDP_SEG_GLOBAL* const m = seg_global(m_base) + E.stride;
  float NDP_SEG_GLOBAL* const v = seg_global(v_base) + E.stride;
  // every full float4 and every scalar slot in flight before the barrier; the components of a
  // float4 that crosses the entry's end are loaded in the store phase
  float gs[kSegElems], xs[kSegElems], ms[kSegElems], vs[kSegElems];
  seg_walk(
      E, p.base,
      [&](int q, int64_t k) __attribute__((always_inline)) {
        const seg_f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const seg_f32x4 NDP_SEG_GLOBAL*>(g + k));
        const seg_f32x4 xv = seg_ld4(x + k);
        const seg_f32x4 mv = __builtin_nontemporal_load(reinterpret_cast<const seg_f32x4 NDP_SEG_GLOBAL*>(m + k));
        const seg_f32x4 vv = __builtin_nontemporal_load(reinterpret_cast<const seg_f32x4 NDP_SEG_GLOBAL*>(v + k));
#pragma unroll
        for (int j = 0; j < 4; ++j) gs[4 * q + j] = gv[j], xs[4 * q + j] = xv[j], ms[4 * q + j] = mv[j], vs[4 * q + j] = vv[j];
      },
      [&](int i, int64_t k, bool tail) __attribute__((always_inline)) {
        if (tail) return;
        gs[i] = __builtin_nontemporal_load(g + k);
        xs[i] = x[k];
        ms[i] = __builtin_nontemporal_load(m + k);
        vs[i] = __builtin_nontemporal_load(v + k);
      });
  const float lr = hyper[0], wd = hyper[1];
  __syncthreads();
  const float b1pow = pow_sh[0], b2pow = pow_sh[1];
  const float p1 = __fmul_rn(b1pow, beta1);
  const float p2 = __fmul_rn(b2pow, beta2);
  float lw = __fmul_rn(lr, wd);
  asm volatile("" : "+v"(lw));
  AdamScalars S;
  S.beta1 = beta1;
  S.beta2 = beta2;
  S.om1 = __fsub_rn(1.0f, beta1);
  S.om2 = __fsub_rn(1.0f, beta2);
  S.ss = __fdiv_rn(lr, __fsub_rn(1.0f, p1));
  S.sb = __builtin_sqrtf(__fsub_rn(1.0f, p2));
  S.eps = eps;
  S.c = __fsub_rn(1.0f, lw);
  S.div = div;
  S.scale = div != 1.0f;
  S.decay = wd != 0.f && !(E.pad & 1);
  seg_walk(
      E, p.base,
      [&](int q, int64_t k) __attribute__((always_inline)) {
        seg_f32x4 xv, mv, vv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          adamw_elem(xs[4 * q + j], gs[4 * q + j], ms[4 * q + j], vs[4 * q + j], S);
          xv[j] = xs[4 * q + j], mv[j] = ms[4 * q + j], vv[j] = vs[4 * q + j];
        }
        seg_st4(x + k, xv);
        __builtin_nontemporal_store(mv, reinterpret_cast<seg_f32x4 NDP_SEG_GLOBAL*>(m + k));
        __builtin_nontemporal_store(vv, reinterpret_cast<seg_f32x4 NDP_SEG_GLOBAL*>(v + k));
      },
      [&](int i, int64_t k, bool tail) __attribute__((always_inline)) {
        const float gk = tail ? __builtin_nontemporal_load(g + k) : gs[i];
        float xk = tail ? x[k] : xs[i];
        float mk = tail ? __builtin_nontemporal_load(m + k) : ms[i];
        float vk = tail ? __builtin_nontemporal_load(v + k) : vs[i];
        adamw_elem(xk, gk, mk, vk, S);
        x[k] = xk;
        __builtin_nontemporal_store(mk, m + k);
        __builtin_nontemporal_store(vk, v + k);
      });
  if (threadIdx.x != 0 || !arrive_last_grouped(ctr)) return;
  // last arriver: every workgroup has drawn its ticket, hence read the block
  block->b1pow = p1;
  block->b2pow = p2;
  block->steps = steps + 1u;
  block->pad = 0u;
  arrive_rearm(ctr);
}

void launch_adamw_step(const SegEntry* entries, const int64_t* block_prefix, int n_entries, int64_t n_blocks,
                       unsigned* ctr, AdamBlock* block, const float* hyper, float* m, float* v, float beta1,
                       float beta2, float eps, float div, hipStream_t s) {
  if (n_entries <= 0 || n_blocks <= 0) return;
  hipLaunchKernelGGL(adamw_step_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, entries, block_prefix, n_entries,
                     ctr, block, hyper, m, v, beta1, beta2, eps, div);
}

}  // namespace ndp
