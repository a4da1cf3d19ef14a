// The optimisers' device-resident hyper-parameter block, read by every update kernel
// (powersgd.hip: psgd_update_kernel, psgd_update_wide_kernel, rank1_step_kernel;
// multitensor.hip: sgd_momentum_vec_kernel, sgd_momentum_kernel).
//
//   hyper = [lr, weight_decay, 0, 0]   (fp32, 16 B, allocated before any graph capture)
//
// A captured step freezes its by-value kernel arguments into the hipGraph, so a learning-rate
// schedule cannot reach a replay through them.  The block can: the host overwrites it between
// replays (one 16-B async copy, only when a value changed) and the kernels read it at run time.
// The pointer is a kernel argument, so the two loads are scalar loads: once per workgroup,
// wave-uniform, no VGPR.  hyper == nullptr keeps the by-value lr and weight_decay = 0.
#pragma once
#include <hip/hip_runtime.h>

namespace ndp {

struct Hyper {
  float lr, wd;
};

__device__ __forceinline__ Hyper load_hyper(const float* __restrict__ hyper, float lr_arg) {
  if (hyper == nullptr) return Hyper{lr_arg, 0.f};
  return Hyper{hyper[0], hyper[1]};
}

// d = o + wd x (L2 weight decay joins the decompressed / averaged gradient o).  The wd != 0 test
// is part of the rule: fmaf(0, x, o) turns o = -0 into +0 and spreads an infinite x, and with
// weight_decay = 0 every step has to stay bitwise what it was without the block.
__device__ __forceinline__ float decayed(float o, float x, float wd) { return wd != 0.f ? fmaf(wd, x, o) : o; }

typedef float hyper_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ hyper_f32x4 decayed(hyper_f32x4 o, hyper_f32x4 x, float wd) {
  if (wd != 0.f) {  // wave-uniform
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = fmaf(wd, x[j], o[j]);
  }
  return o;
}

}  // namespace ndp
