// What the per-block error-feedback compressors (signsgd.hip, quant.hip) share: one workgroup of 256
// threads per block of 2048 elements, thread tid owning the in-block elements
//     t = 1024 h + 4 tid + c,   h = 0, 1 (round),  c = 0 .. 3 (float4 component),
// the float4-or-scalars quad access of a ragged block, the rule's single-instruction add / subtract,
// and the element rule behind the decompressed average.
#pragma once
#include <hip/hip_runtime.h>

#include "adam_block.h"
#include "hyper.h"

namespace ndp {

// the compiler forms no packed fp32 instruction in these kernels (neighbouring components of the
// update's last fma would pair otherwise).  A function without the attribute is not inlined into one
// with it unless it is always_inline, so cross-lane operations are the builtins, not the HIP wrappers.
#define NDP_NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))

typedef float sign_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned sign_u32x4 __attribute__((ext_vector_type(4)));

struct Quad {
  float v[4];
  int nv;  // leading valid elements (the rest lie past the block's length)
};

// the 4 elements at i (a multiple of 4; src is 16-byte aligned): one float4, or scalars across n
__device__ __forceinline__ Quad load_quad(const float* __restrict__ src, int i, int n) {
  Quad q = {{0.f, 0.f, 0.f, 0.f}, 0};
  if (i + 4 <= n) {
    const sign_f32x4 t = *reinterpret_cast<const sign_f32x4*>(src + i);
    q.v[0] = t[0]; q.v[1] = t[1]; q.v[2] = t[2]; q.v[3] = t[3];
    q.nv = 4;
  } else if (i < n) {
    q.nv = n - i;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (j < q.nv) q.v[j] = src[i + j];
  }
  return q;
}

__device__ __forceinline__ void store_quad(float* __restrict__ dst, int i, const Quad& q) {
  if (q.nv == 4) {
    sign_f32x4 t;
    t[0] = q.v[0]; t[1] = q.v[1]; t[2] = q.v[2]; t[3] = q.v[3];
    *reinterpret_cast<sign_f32x4*>(dst + i) = t;
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (j < q.nv) dst[i + j] = q.v[j];
  }
}

// fadd / fsub as one scalar instruction each: never fused, never paired into a packed fp32 op
__device__ __forceinline__ float fadd_scalar(float a, float b) {
  float r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float fsub_scalar(float a, float b) {
  float r;
  asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

__device__ __forceinline__ unsigned bits_of(float v) { return __builtin_bit_cast(unsigned, v); }

// __syncthreads()
__device__ __forceinline__ void block_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the element rule behind the rank-ordered sum a of N decompressed contributions
__device__ __forceinline__ float sign_step(float a, float x, float& b, int N, float fN, float lr, float wd, float lam) {
  const float o = N != 1 ? __fdiv_rn(a, fN) : a;
  const float d = decayed(o, x, wd);
  float bl = __fmul_rn(b, lam);
  asm volatile("" : "+v"(bl));  // the build's -ffp-contract=fast would fuse the product into the add
  b = fadd_scalar(bl, d);
  return __fmaf_rn(-lr, fadd_scalar(d, b), x);
}

// ---- AdamW behind the rank-ordered sum (sign_update_adam_kernel, quant_update_adam_kernel) --------
// The SGD update kernels' thread map and decode with the element rule of adamw_elem.h in the place of
// sign_step: g := o, div = 1, decay per block.  The arena b holds the first moment m, a third arena
// of the same layout the second moment v; both are touched once per step, so their quads go through
// non-temporal loads and stores (x keeps plain ones: the next forward reads it).  The step-dependent
// scalars come from the AdamBlock by the protocol of adam_block.h: one barrier and 8 bytes of LDS are
// all these kernels have over the SGD ones.
constexpr int kEfThreads = 256, kEfRounds = 2;

__device__ __forceinline__ Quad load_quad_nt(const float* __restrict__ src, int i, int n) {
  Quad q = {{0.f, 0.f, 0.f, 0.f}, 0};
  if (i + 4 <= n) {
    const sign_f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const sign_f32x4*>(src + i));
    q.v[0] = t[0]; q.v[1] = t[1]; q.v[2] = t[2]; q.v[3] = t[3];
    q.nv = 4;
  } else if (i < n) {
    q.nv = n - i;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (j < q.nv) q.v[j] = __builtin_nontemporal_load(src + i + j);
  }
  return q;
}

__device__ __forceinline__ void store_quad_nt(float* __restrict__ dst, int i, const Quad& q) {
  if (q.nv == 4) {
    sign_f32x4 t;
    t[0] = q.v[0]; t[1] = q.v[1]; t[2] = q.v[2]; t[3] = q.v[3];
    __builtin_nontemporal_store(t, reinterpret_cast<sign_f32x4*>(dst + i));
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (j < q.nv) __builtin_nontemporal_store(q.v[j], dst + i + j);
  }
}

// a thread's two quads of x, m and v of its block
struct EfAdamRegs {
  Quad x[kEfRounds], m[kEfRounds], v[kEfRounds];
};

// xb / mb / vb: the block's first element in the three arenas.  Six loads in flight on return.
__device__ __forceinline__ EfAdamRegs ef_adam_load(const float* __restrict__ xb, const float* __restrict__ mb,
                                                   const float* __restrict__ vb, int tid, int len) {
  EfAdamRegs R;
#pragma unroll
  for (int h = 0; h < kEfRounds; ++h) {
    R.x[h] = load_quad(xb, h * 4 * kEfThreads + 4 * tid, len);
    R.m[h] = load_quad_nt(mb, h * 4 * kEfThreads + 4 * tid, len);
    R.v[h] = load_quad_nt(vb, h * 4 * kEfThreads + 4 * tid, len);
  }
  return R;
}

// Behind the decode: the workgroup's one barrier, the launch's scalars from what adam_block_read left
// in pow_sh, o = acc / N, the element rule, the stores, and the block's ticket.  steps: thread 0's.
__device__ __forceinline__ void ef_adam_tail(float* __restrict__ xb, float* __restrict__ mb, float* __restrict__ vb,
                                             int tid, EfAdamRegs& R, const float (&acc)[kEfRounds][4], int N, Hyper hy,
                                             bool decays, const float* pow_sh, float beta1, float beta2, float eps,
                                             unsigned* ctr, AdamBlock* block, unsigned steps) {
  block_barrier();
  float p1, p2;
  AdamScalars S = adam_launch_scalars(pow_sh[0], pow_sh[1], hy.lr, hy.wd, beta1, beta2, eps, p1, p2);
  S.decay = hy.wd != 0.f && decays;
  const float fN = (float)N;
#pragma unroll
  for (int h = 0; h < kEfRounds; ++h) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float o = N != 1 ? __fdiv_rn(acc[h][c], fN) : acc[h][c];
      adamw_elem(R.x[h].v[c], o, R.m[h].v[c], R.v[h].v[c], S);
    }
    store_quad(xb, h * 4 * kEfThreads + 4 * tid, R.x[h]);
    store_quad_nt(mb, h * 4 * kEfThreads + 4 * tid, R.m[h]);
    store_quad_nt(vb, h * 4 * kEfThreads + 4 * tid, R.v[h]);
  }
  adam_block_advance(ctr, block, p1, p2, steps);
}

}  // namespace ndp
