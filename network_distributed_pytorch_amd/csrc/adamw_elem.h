// The AdamW element rule of adamw.hip's header comment, shared by adamw_step_kernel (adamw.hip)
// and the PowerSGD update kernels that step with it (powersgd.hip: psgd_update_adam_wide_kernel,
// rank1_adam_step_kernel).  Every line is ONE correctly rounded fp32 operation: every product that
// feeds an add or a subtract passes an empty asm, so -ffp-contract=fast never fuses it.
#pragma once
#include <hip/hip_runtime.h>

namespace ndp {

// the launch's scalars, wave-uniform
struct AdamScalars {
  float beta1, beta2, om1, om2, ss, sb, eps, c, div;
  bool scale, decay;
};

// one element of the rule; every product that feeds an add or a subtract passes an empty asm
__device__ __forceinline__ void adamw_elem(float& x, float g, float& m, float& v, const AdamScalars& S) {
  const float gg = S.scale ? __fdiv_rn(g, S.div) : g;
  float x1 = x;
  if (S.decay) x1 = __fmul_rn(x, S.c);
  asm volatile("" : "+v"(x1));
  float a = __fmul_rn(S.beta1, m);
  float b = __fmul_rn(S.om1, gg);
  asm volatile("" : "+v"(a));
  asm volatile("" : "+v"(b));
  const float mn = __fadd_rn(a, b);
  float g2 = __fmul_rn(gg, gg);
  asm volatile("" : "+v"(g2));
  float d = __fmul_rn(S.beta2, v);
  float e = __fmul_rn(S.om2, g2);
  asm volatile("" : "+v"(d));
  asm volatile("" : "+v"(e));
  const float vn = __fadd_rn(d, e);
  const float den = __fadd_rn(__fdiv_rn(__builtin_sqrtf(vn), S.sb), S.eps);
  float u = __fmul_rn(S.ss, __fdiv_rn(mn, den));
  asm volatile("" : "+v"(u));
  x = __fsub_rn(x1, u);
  m = mn;
  v = vn;
}

// The per-launch scalars from the block as it was before the step (ops/adamw.py adamw_scalars is
// the twin); p1 / p2 are the running products the block's last writer stores.  div = 1, no decay:
// the caller sets S.div / S.scale / S.decay for its stream.
__device__ __forceinline__ AdamScalars adam_launch_scalars(float b1pow, float b2pow, float lr, float wd, float beta1,
                                                           float beta2, float eps, float& p1, float& p2) {
  p1 = __fmul_rn(b1pow, beta1);
  p2 = __fmul_rn(b2pow, beta2);
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
  S.div = 1.0f;
  S.scale = false;
  S.decay = false;
  return S;
}

}  // namespace ndp
