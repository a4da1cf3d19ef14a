// What the per-block error-feedback compressors (signsgd.hip, quant.hip) share: one workgroup of 256
// threads per block of 2048 elements, thread tid owning the in-block elements
//     t = 1024 h + 4 tid + c,   h = 0, 1 (round),  c = 0 .. 3 (float4 component),
// the float4-or-scalars quad access of a ragged block, the rule's single-instruction add / subtract,
// and the element rule behind the decompressed average.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace ndp
