// LAMB (You et al. 2020, with bias correction) and LARS (You et al. 2017, the scaled-gradient form
// of LARC / lightning-bolts): the layer-wise trust-ratio optimisers, over a SegEntry table with ONE
// entry per parameter tensor (src = gradient g, dst = parameter x; build_adamw_table: `stride` is the
// tensor's offset into the moment arenas, pad bit 0 says "exempt"), one workgroup per table block of
// 2048 elements (the walk of seg_block.h; a block never spans tensors), in TWO launches per step:
//
//   lw_norm   reads the step's inputs, forms two fp64 sums of squares per tensor and from them
//             trust[t] (fp32, one per table entry); LAMB also writes the new moments and advances
//             the AdamBlock.
//   lw_apply  one scalar load of trust[t] per workgroup, then the element update.
// Two launches because an element's update needs its whole tensor's norms: one launch would need a
// grid-wide wait.  No workgroup waits for another; there is no floating-point atomic.
//
//   The rules.  fp32 unless marked; every line is ONE correctly rounded operation, and a product
//   that feeds an add or a subtract passes an empty asm (the adamw_elem.h idiom) unless the line
//   is written as an fma.  adapts_t = !(pad & 1): an exempt tensor neither decays nor adapts
//   (trust 1).  div >= 1, beta1, beta2, eps, mu, eta = lars_coef, eps_l = lars_eps go by value;
//   lr, wd come from the hyper block [lr, wd, 0, 0] (hyper.h).  gg = (div != 1) ? g / div : g.
//
//   LAMB, from the AdamBlock {b1pow, b2pow, steps} as it was before lw_norm:
//       p1 = b1pow * beta1     p2 = b2pow * beta2     bc1 = 1 - p1     sb = sqrt(1 - p2)
//       om1 = 1 - beta1        om2 = 1 - beta2
//     per element (lw_norm; m', v' are bitwise the AdamW rule's):
//       m' = (beta1 m) + (om1 gg)           v' = (beta2 v) + (om2 (gg gg))
//       den = (sqrt(v') / sb) + eps         q = m' / den          r = q / bc1
//       u = (wd != 0 && adapts_t) ? r + (wd x) : r                            (lamb_u, both kernels)
//     per tensor:  W = sqrt(sum x^2), U = sqrt(sum u^2) in fp64;
//       trust_t = (adapts_t && W > 0 && U > 0) ? (float)(W / U) : 1      (a NaN fails the tests and
//                                                                          then propagates through u)
//     per element (lw_apply):  a = lr * trust_t      x' = x - (a u)
//     once per step, by lw_norm's last arriver, the block becomes {p1, p2, steps + 1, 0}.  lw_apply
//     reads bc1 = 1 - b1pow and sb = sqrt(1 - b2pow) from the ADVANCED block: b1pow is then exactly
//     p1, so they are lw_norm's values bit for bit, and u is re-formed from the stored m', v' and the
//     x that nothing touched in between.
//
//   LARS, momentum buffer b:
//     per tensor:  W = sqrt(sum x^2), G = sqrt(sum gg^2) in fp64;
//       lam_t = (adapts_t && W > 0 && G > 0) ? (float)((eta W) / ((G + (wd W)) + eps_l)) : 1
//       (fp64 on the fp32 values of eta, wd, eps_l; no contraction; rounded to fp32 once)
//     per element (lw_apply):
//       d = (wd != 0 && adapts_t) ? fma(wd, x, gg) : gg        (the dense arm's decay rule, hyper.h)
//       s = lam_t * d           b' = fma(b, mu, s)           x' = fma(-lr, b', x)
//     The two fmas are what sgd_momentum_vec_kernel executes (its mu * b + g contracts under
//     -ffp-contract=fast; here they are written out, so they do not depend on the flag): where
//     lam_t == 1 the element rule is bitwise that kernel's.
//
//   Norm sums (fixed order: bitwise reproducible from run to run and under graph replay, never
//   dependent on which workgroup arrived when).  acc = fma((double)v, (double)v, acc):
//     thread:    its 8 elements in the order of seg_block.h; an absent element adds nothing (+0.0).
//     wave:      xor butterfly, offsets 32, 16, 8, 4, 2, 1.
//     workgroup: ((w0 + w1) + w2) + w3.  Thread 0 stores the pair {sum_a, sum_b} at
//                partial[2 * blk] as sc1 (write-through) stores, drains them and draws the
//                two-level ticket (arrival.h), as grad_sqnorm_kernel does.
//     tensor:    by the LAST arriver, all 256 threads of it.  A tensor of more than kLwWaveBlocks
//                blocks is summed by the whole workgroup: thread t adds the tensor's block partials
//                t, t + 256, ... in increasing order, then the wave and workgroup steps above.  A
//                tensor of at most kLwWaveBlocks = 64 blocks (131 072 elements) is summed by ONE wave
//                (wave w takes the tensors w, w + 4, ... of the table and skips the large ones): lane
//                l holds partial l, then the butterfly.  Which of the two applies depends on the
//                tensor's block count only.  (DistilBERT: the word embedding is 11 446 blocks: one
//                thread never walks them; ResNet-18: 14 of 62 tensors are large, the other 48 go four
//                at a time.)
//   The last arriver then advances the block (LAMB) and re-arms the ticket: replay-safe.
//
//   Loads, stores, cache policy.  Every full float4 and scalar slot of every stream is in flight
//   before lw_norm's one barrier (LAMB: 32 values per thread, as adamw_step_kernel).  lw_norm writes
//   m', v' with PLAIN stores and reads x, and LARS's g, with plain loads: lw_apply reads them again
//   within the same step, and what of them still sits in L2 / MALL (the MI355X has 256 MB of it:
//   ResNet-18's 2 x 45 MB of moments fit, DistilBERT's 2 x 265 MB do not) is served from there; a
//   non-temporal store would send the lines to HBM for certain.  lw_apply takes g, m', v', b with
//   non-temporal loads and writes b' non-temporally: their last touch of the step.  x is always
//   plain: the next forward reads it.  Neither kernel writes g.
//   Bytes per element over the two launches: LAMB 16 + 8 (norm) + 12 + 4 (apply) = 40 (AdamW: 28),
//   LARS 8 + 12 + 8 = 28 (SGD: 20).
//
//   Resources (hipcc --offload-arch=gfx950 -O3 -ffp-contract=fast, -Rpass-analysis=kernel-resource-usage):
//   no kernel uses AGPRs or scratch (0 bytes/lane, no spills).
//     lw_norm_kernel<LAMB>   64 VGPRs, 61 SGPRs, 80 B of LDS, occupancy 8 waves/SIMD
//     lw_norm_kernel<LARS>   61 VGPRs, 59 SGPRs, 72 B of LDS, occupancy 8 waves/SIMD
//     lw_apply_kernel<LAMB>  26 VGPRs, 36 SGPRs, no LDS,     occupancy 8 waves/SIMD
//     lw_apply_kernel<LARS>  38 VGPRs, 36 SGPRs, no LDS,     occupancy 8 waves/SIMD
#include <hip/hip_runtime.h>
#include <math.h>

#include "arrival.h"
#include "ndp_kernels.h"
#include "seg_block.h"

namespace ndp {

constexpr int kLwWaveBlocks = 64;  // a tensor of at most this many blocks is summed by one wave (one per lane)

// the LAMB launch scalars, wave-uniform
struct LambScalars {
  float beta1, beta2, om1, om2, sb, bc1, eps, wd, div;
  bool scale, decay;
};

// m', v' of one element: the AdamW rule's lines (adamw_elem.h), bitwise
__device__ __forceinline__ void lamb_moments(float g, float& m, float& v, const LambScalars& S) {
  const float gg = S.scale ? __fdiv_rn(g, S.div) : g;
  float a = __fmul_rn(S.beta1, m);
  float b = __fmul_rn(S.om1, gg);
  asm volatile("" : "+v"(a));
  asm volatile("" : "+v"(b));
  m = __fadd_rn(a, b);
  float g2 = __fmul_rn(gg, gg);
  asm volatile("" : "+v"(g2));
  float d = __fmul_rn(S.beta2, v);
  float e = __fmul_rn(S.om2, g2);
  asm volatile("" : "+v"(d));
  asm volatile("" : "+v"(e));
  v = __fadd_rn(d, e);
}

// u of one element from the NEW moments: lw_norm squares it, lw_apply steps with it
__device__ __forceinline__ float lamb_u(float x, float m, float v, const LambScalars& S) {
  const float den = __fadd_rn(__fdiv_rn(__builtin_sqrtf(v), S.sb), S.eps);
  const float r = __fdiv_rn(__fdiv_rn(m, den), S.bc1);
  if (!S.decay) return r;
  float wx = __fmul_rn(S.wd, x);
  asm volatile("" : "+v"(wx));
  return __fadd_rn(r, wx);
}

__device__ __forceinline__ double lw_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// trust_t / lam_t from the tensor's two sums
template <bool LAMB>
__device__ __forceinline__ float lw_trust(double sa, double sb, bool adapts, float wd, float eta, float eps_l) {
  const double W = sqrt(sa), B = sqrt(sb);
  if (!(adapts && W > 0.0 && B > 0.0)) return 1.0f;
  if (LAMB) return (float)(W / B);
  double num = (double)eta * W, dw = (double)wd * W;
  asm volatile("" : "+v"(num));
  asm volatile("" : "+v"(dw));
  return (float)(num / ((B + dw) + (double)eps_l));
}

template <bool LAMB>
__global__ __launch_bounds__(256) void lw_norm_kernel(const SegEntry* __restrict__ ents,
                                                      const int64_t* __restrict__ prefix, int n_ent,
                                                      double* __restrict__ partial, unsigned* __restrict__ ctr,
                                                      float* __restrict__ trust, LwArgs a) {
  __shared__ float pow_sh[2];
  __shared__ double red[4][2];
  __shared__ int last;
  unsigned steps = 0;
  if (LAMB && threadIdx.x == 0) {  // the wave that later draws the ticket; nobody reads the block after the draw
    pow_sh[0] = a.block->b1pow;
    pow_sh[1] = a.block->b2pow;
    steps = a.block->steps;
  }
  const SegPos p = seg_find(ents, prefix, n_ent, blockIdx.x);
  const SegEntry& E = p.E;
  const float NDP_SEG_GLOBAL* const g = seg_global(E.src);
  const float NDP_SEG_GLOBAL* const x = seg_global(E.dst);
  float NDP_SEG_GLOBAL* const m = seg_global(a.m) + E.stride;
  float NDP_SEG_GLOBAL* const v = seg_global(a.v) + E.stride;
  float gs[kSegElems], xs[kSegElems], ms[kSegElems], vs[kSegElems];  // ms / vs: LAMB only
  seg_walk(
      E, p.base,
      [&](int q, int64_t k) __attribute__((always_inline)) {
        const seg_f32x4 gv = seg_ld4(g + k), xv = seg_ld4(x + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) gs[4 * q + j] = gv[j], xs[4 * q + j] = xv[j];
        if (LAMB) {
          const seg_f32x4 mv = seg_ld4(m + k), vv = seg_ld4(v + k);
#pragma unroll
          for (int j = 0; j < 4; ++j) ms[4 * q + j] = mv[j], vs[4 * q + j] = vv[j];
        }
      },
      [&](int i, int64_t k, bool tail) __attribute__((always_inline)) {
        if (tail) return;
        gs[i] = g[k];
        xs[i] = x[k];
        if (LAMB) ms[i] = m[k], vs[i] = v[k];
      });
  const float wd = a.hyper[1];
  float p1 = 0.f, p2 = 0.f;
  LambScalars S;
  S.div = a.div;
  S.scale = a.div != 1.0f;
  S.decay = wd != 0.f && !(E.pad & kAdamNoDecay);
  S.wd = wd;
  if (LAMB) {
    __syncthreads();
    p1 = __fmul_rn(pow_sh[0], a.beta1);
    p2 = __fmul_rn(pow_sh[1], a.beta2);
    asm volatile("" : "+v"(p1));  // 1 - p is a subtraction of a ROUNDED product
    asm volatile("" : "+v"(p2));
    S.beta1 = a.beta1;
    S.beta2 = a.beta2;
    S.om1 = __fsub_rn(1.0f, a.beta1);
    S.om2 = __fsub_rn(1.0f, a.beta2);
    S.bc1 = __fsub_rn(1.0f, p1);
    S.sb = __builtin_sqrtf(__fsub_rn(1.0f, p2));
    S.eps = a.eps;
  }
  double acc_a = 0.0, acc_b = 0.0;  // x^2 ; u^2 (LAMB) or gg^2 (LARS)
  // one present element: its two squares, and for LAMB the new moments into mk / vk
  auto one = [&](float gk, float xk, float& mk, float& vk) __attribute__((always_inline)) {
    float t;
    if (LAMB) {
      lamb_moments(gk, mk, vk, S);
      t = lamb_u(xk, mk, vk, S);
    } else {
      t = S.scale ? __fdiv_rn(gk, S.div) : gk;
    }
    acc_a = fma((double)xk, (double)xk, acc_a);
    acc_b = fma((double)t, (double)t, acc_b);
  };
  seg_walk(
      E, p.base,
      [&](int q, int64_t k) __attribute__((always_inline)) {
        seg_f32x4 mv, vv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float mk = LAMB ? ms[4 * q + j] : 0.f, vk = LAMB ? vs[4 * q + j] : 0.f;
          one(gs[4 * q + j], xs[4 * q + j], mk, vk);
          mv[j] = mk, vv[j] = vk;
        }
        if (LAMB) {
          seg_st4(m + k, mv);
          seg_st4(v + k, vv);
        }
      },
      [&](int i, int64_t k, bool tail) __attribute__((always_inline)) {
        const float gk = tail ? g[k] : gs[i];
        const float xk = tail ? x[k] : xs[i];
        float mk = 0.f, vk = 0.f;
        if (LAMB) mk = tail ? m[k] : ms[i], vk = tail ? v[k] : vs[i];
        one(gk, xk, mk, vk);
        if (LAMB) m[k] = mk, v[k] = vk;
      });
  // workgroup: butterfly, then ((w0 + w1) + w2) + w3 on thread 0
  acc_a = lw_wave_sum(acc_a);
  acc_b = lw_wave_sum(acc_b);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = acc_a, red[threadIdx.x >> 6][1] = acc_b;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sa = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    const double sb = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    // sc1 (write-through) stores, drained before the ticket: read back by the last workgroup
    __hip_atomic_store(partial + 2 * (size_t)blockIdx.x, sa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(partial + 2 * (size_t)blockIdx.x + 1, sb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = arrive_last_grouped(ctr);
  }
  __syncthreads();
  if (!last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // compiler order only: the loads below are sc1

  // ---- the last arriver: every tensor's sums in a fixed order, trust[t] -------------------------
  const float eta = a.coef, eps_l = a.eps_l;
  auto ld = [&](int64_t b) __attribute__((always_inline)) {
    return __hip_atomic_load(partial + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  auto blocks_of = [&](int t, int64_t& b0) __attribute__((always_inline)) {
    b0 = prefix[t];
    return (t + 1 < n_ent ? prefix[t + 1] : (int64_t)gridDim.x) - b0;
  };
  constexpr int kBatch = 8;  // block partials in flight per thread; the adds keep increasing index order
  // tensors of more than kLwWaveBlocks blocks: the whole workgroup (the loop and its barriers are uniform)
  for (int t = 0; t < n_ent; ++t) {
    int64_t b0;
    const int64_t nb = blocks_of(t, b0);
    if (nb <= kLwWaveBlocks) continue;
    double sa = 0.0, sb = 0.0;
    for (int64_t r0 = threadIdx.x; r0 < nb; r0 += 256 * kBatch) {
      double ta[kBatch], tb[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const int64_t r = r0 + 256 * j;
        ta[j] = r < nb ? ld(2 * (b0 + r)) : 0.0;
        tb[j] = r < nb ? ld(2 * (b0 + r) + 1) : 0.0;
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) sa += ta[j], sb += tb[j];  // + 0.0 past the end is exact: a partial is >= +0 or NaN
    }
    sa = lw_wave_sum(sa);
    sb = lw_wave_sum(sb);
    __syncthreads();  // red: thread 0 has read the previous sums
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = sa, red[threadIdx.x >> 6][1] = sb;
    __syncthreads();
    if (threadIdx.x == 0) {
      sa = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
      sb = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
      trust[t] = lw_trust<LAMB>(sa, sb, !(ents[t].pad & kAdamNoDecay), wd, eta, eps_l);
    }
  }
  // the others: one wave each, four at a time
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  for (int t = wave; t < n_ent; t += 4) {
    int64_t b0;
    const int64_t nb = blocks_of(t, b0);
    if (nb > kLwWaveBlocks) continue;
    static_assert(kLwWaveBlocks == 64, "one block partial per lane");
    const double sa = lw_wave_sum(lane < nb ? ld(2 * (b0 + lane)) : 0.0);  // + 0.0 past the end is exact
    const double sb = lw_wave_sum(lane < nb ? ld(2 * (b0 + lane) + 1) : 0.0);
    if (lane == 0) trust[t] = lw_trust<LAMB>(sa, sb, !(ents[t].pad & kAdamNoDecay), wd, eta, eps_l);
  }
  if (threadIdx.x == 0) {
    if (LAMB) {  // every workgroup has drawn its ticket, hence read the block
      a.block->b1pow = p1;
      a.block->b2pow = p2;
      a.block->steps = steps + 1u;
      a.block->pad = 0u;
    }
    arrive_rearm(ctr);
  }
}

template <bool LAMB>
__global__ __launch_bounds__(256) void lw_apply_kernel(const SegEntry* __restrict__ ents,
                                                       const int64_t* __restrict__ prefix, int n_ent,
                                                       const float* __restrict__ trust, LwArgs a) {
  const SegPos p = seg_find(ents, prefix, n_ent, blockIdx.x);
  const SegEntry& E = p.E;
  const float tr = trust[p.ent];  // uniform address: one scalar load
  const float lr = a.hyper[0], wd = a.hyper[1];
  const bool decay = wd != 0.f && !(E.pad & kAdamNoDecay);
  float NDP_SEG_GLOBAL* const x = seg_global(E.dst);
  typedef const seg_f32x4 NDP_SEG_GLOBAL* V4;
  if (LAMB) {
    const float NDP_SEG_GLOBAL* const m = seg_global(a.m) + E.stride;
    const float NDP_SEG_GLOBAL* const v = seg_global(a.v) + E.stride;
    LambScalars S;
    S.bc1 = __fsub_rn(1.0f, a.block->b1pow);  // the advanced block: lw_norm's 1 - p1, bit for bit
    S.sb = __builtin_sqrtf(__fsub_rn(1.0f, a.block->b2pow));
    S.eps = a.eps;
    S.wd = wd;
    S.decay = decay;
    const float al = __fmul_rn(lr, tr);
    auto one = [&](float xk, float mk, float vk) __attribute__((always_inline)) {
      float au = __fmul_rn(al, lamb_u(xk, mk, vk, S));
      asm volatile("" : "+v"(au));
      return __fsub_rn(xk, au);
    };
    seg_walk(
        E, p.base,
        [&](int, int64_t k) __attribute__((always_inline)) {
          seg_f32x4 xv = seg_ld4(x + k);
          const seg_f32x4 mv = __builtin_nontemporal_load(reinterpret_cast<V4>(m + k));
          const seg_f32x4 vv = __builtin_nontemporal_load(reinterpret_cast<V4>(v + k));
#pragma unroll
          for (int j = 0; j < 4; ++j) xv[j] = one(xv[j], mv[j], vv[j]);
          seg_st4(x + k, xv);
        },
        [&](int, int64_t k, bool) __attribute__((always_inline)) {
          x[k] = one(x[k], __builtin_nontemporal_load(m + k), __builtin_nontemporal_load(v + k));
        });
  } else {
    const float NDP_SEG_GLOBAL* const g = seg_global(E.src);
    float NDP_SEG_GLOBAL* const b = seg_global(a.m) + E.stride;
    const float mu = a.mu, div = a.div;
    const bool scale = div != 1.0f;
    auto one = [&](float gk, float& xk, float& bk) __attribute__((always_inline)) {
      const float gg = scale ? __fdiv_rn(gk, div) : gk;
      const float d = decay ? fmaf(wd, xk, gg) : gg;
      float s = __fmul_rn(tr, d);
      asm volatile("" : "+v"(s));
      bk = fmaf(bk, mu, s);
      xk = fmaf(-lr, bk, xk);
    };
    seg_walk(
        E, p.base,
        [&](int, int64_t k) __attribute__((always_inline)) {
          const seg_f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<V4>(g + k));
          seg_f32x4 bv = __builtin_nontemporal_load(reinterpret_cast<V4>(b + k));
          seg_f32x4 xv = seg_ld4(x + k);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float xk = xv[j], bk = bv[j];
            one(gv[j], xk, bk);
            xv[j] = xk, bv[j] = bk;
          }
          __builtin_nontemporal_store(bv, reinterpret_cast<seg_f32x4 NDP_SEG_GLOBAL*>(b + k));
          seg_st4(x + k, xv);
        },
        [&](int, int64_t k, bool) __attribute__((always_inline)) {
          float xk = x[k], bk = __builtin_nontemporal_load(b + k);
          one(__builtin_nontemporal_load(g + k), xk, bk);
          __builtin_nontemporal_store(bk, b + k);
          x[k] = xk;
        });
  }
}

void launch_lw_norm(bool lamb, const SegEntry* entries, const int64_t* block_prefix, int n_entries, int64_t n_blocks,
                    double* partial, unsigned* ctr, float* trust, const LwArgs& a, hipStream_t s) {
  if (n_entries <= 0 || n_blocks <= 0) return;
  if (lamb)
    hipLaunchKernelGGL(lw_norm_kernel<true>, dim3((unsigned)n_blocks), dim3(256), 0, s, entries, block_prefix,
                       n_entries, partial, ctr, trust, a);
  else
    hipLaunchKernelGGL(lw_norm_kernel<false>, dim3((unsigned)n_blocks), dim3(256), 0, s, entries, block_prefix,
                       n_entries, partial, ctr, trust, a);
}

void launch_lw_apply(bool lamb, const SegEntry* entries, const int64_t* block_prefix, int n_entries, int64_t n_blocks,
                     const float* trust, const LwArgs& a, hipStream_t s) {
  if (n_entries <= 0 || n_blocks <= 0) return;
  if (lamb)
    hipLaunchKernelGGL(lw_apply_kernel<true>, dim3((unsigned)n_blocks), dim3(256), 0, s, entries, block_prefix,
                       n_entries, trust, a);
  else
    hipLaunchKernelGGL(lw_apply_kernel<false>, dim3((unsigned)n_blocks), dim3(256), 0, s, entries, block_prefix,
                       n_entries, trust, a);
}

}  // namespace ndp
