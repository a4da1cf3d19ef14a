// Fused softmax cross-entropy (torch.nn.CrossEntropyLoss, mean over non-ignored rows).
//
// PyTorch-ROCm runs the training loss as log_softmax + nll_loss forward and, in backward, a
// zero fill + nll_loss_backward + log_softmax_backward: five launches per step, and its
// nll_loss_forward reduction alone takes ~15 µs at ResNet's 512 x 1000 logits (profiles/r2/).
// Here:
//   fwd: one wave per row (4 rows per 256-thread workgroup): row max, sum of exp(x - max),
//        lse = max + log(sum) (fp32, butterfly order: the same value on every lane),
//        loss_b = lse - x[t], and the row of the saved gradient dl[b, k] = softmax_k - [k == t]
//        (unscaled).  Rows whose target is ignore_index contribute nothing (0 loss, 0 grad).
//        Row losses go to rowloss[b] as sc1 stores; the LAST workgroup to finish (the one-level
//        arrival ticket of arrival.h) adds them in row order and writes loss = sum / n_valid and
//        inv = 1 / n_valid, then re-arms the counter (hipGraph-replay safe).
//   bwd: dx = dl * (dloss * inv) — one float4 launch.
//   ce_soft_fwd_kernel: the forward with label smoothing and a second, weighted target per row
//        (mixup / CutMix); ce_fwd_kernel is the default path and is left as it is.
// Fixed summation order everywhere: bitwise reproducible.
#include <hip/hip_runtime.h>
#include <math.h>

#include "arrival.h"
#include "ndp_kernels.h"

namespace ndp {

typedef float f4ce __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

constexpr int kCeRowsPerWg = 4;
constexpr int kCeRegs = 16;  // row length held in registers: K <= 1024

__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt,
                                                     int B, int K, int64_t ignore, float* __restrict__ dl,
                                                     float* __restrict__ rowloss, float* __restrict__ loss,
                                                     float* __restrict__ inv, unsigned* __restrict__ ctr,
                                                     float* __restrict__ acc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kCeRowsPerWg + wave;
  if (b < B) {
    const float* xr = x + (int64_t)b * K;
    float* dr = dl + (int64_t)b * K;
    const int64_t t = tgt[b];
    const bool valid = t != ignore;
    const bool in_range = t >= 0 && t < K;
    float m = -INFINITY, s = 0.f, lse;
    if (K <= 64 * kCeRegs) {  // the row in registers: one load pass (ResNet's 1000 classes)
      float v[kCeRegs];
#pragma unroll
      for (int i = 0; i < kCeRegs; ++i) {
        const int k = lane + 64 * i;
        v[i] = k < K ? xr[k] : -INFINITY;
        m = fmaxf(m, v[i]);
      }
      m = wave_max_f(m);
#pragma unroll
      for (int i = 0; i < kCeRegs; ++i) s += lane + 64 * i < K ? expf(v[i] - m) : 0.f;
      s = wave_sum_f(s);
      lse = m + logf(s);
#pragma unroll
      for (int i = 0; i < kCeRegs; ++i) {
        const int k = lane + 64 * i;
        if (k < K) dr[k] = valid ? expf(v[i] - lse) - (k == t ? 1.f : 0.f) : 0.f;
      }
    } else {
      for (int k = lane; k < K; k += 64) m = fmaxf(m, xr[k]);
      m = wave_max_f(m);
      for (int k = lane; k < K; k += 64) s += expf(xr[k] - m);
      s = wave_sum_f(s);
      lse = m + logf(s);
      for (int k = lane; k < K; k += 64)
        dr[k] = valid ? expf(xr[k] - lse) - (k == t ? 1.f : 0.f) : 0.f;
    }
    if (lane == 0)  // sc1 (write-through) store: read back by the last workgroup below
      __hip_atomic_store(rowloss + b, !valid ? 0.f : (in_range ? lse - xr[t] : __builtin_nanf("")), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
  // last-arriving workgroup: fixed-order mean over the rows, which cross workgroups through sc1
  // stores (drained by the ticket) and agent-scope loads
  if (!arrive_last(ctr, gridDim.x)) return;
  __shared__ float red[2][4];
  float a = 0.f, n = 0.f;
  for (int r = threadIdx.x; r < B; r += 256) {
    a += __hip_atomic_load(rowloss + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    n += tgt[r] != ignore ? 1.f : 0.f;
  }
  a = wave_sum_f(a);
  n = wave_sum_f(n);
  if (lane == 0) {
    red[0][wave] = a;
    red[1][wave] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float tot = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    const float cnt = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    loss[0] = tot / cnt;  // 0 / 0 = NaN when every row is ignored, like PyTorch
    if (acc != nullptr) acc[0] += tot / cnt;  // running loss sum (logging): no separate add launch
    inv[0] = 1.f / cnt;
    arrive_rearm(ctr);
  }
}

// ---- label smoothing and two targets per row (mixup / CutMix) --------------------------------
// torch.nn.CrossEntropyLoss(label_smoothing=eps) on a row whose target is `ta` with weight lam
// and `tb` with weight 1 - lam (tgt_b == nullptr: lam = 1, one target):
//   la = lse - x[ta], lb = lse - x[tb], hard = lam * la + (1 - lam) * lb   (hard = la with one target)
//   rowloss = (1 - eps) * hard + eps * (lse - sx / K),  sx = sum_k x[k]  (lane order, then the
//             wave butterfly: a fixed order)
//   dl[k]   = softmax_k - (1 - eps) * (lam * [k == ta] + (1 - lam) * [k == tb]) - eps / K
//             (ta == tb: both weights land on k)
// A row is valid iff ta != ignore; ignored rows give 0 loss and a 0 dl row; a valid row with ta
// or tb outside [0, K) gets a NaN loss.  The shape, the sc1 row-loss stores, the ticket, the
// fixed-order mean, inv, acc and the re-arm are ce_fwd_kernel's, and so is the scratch layout:
// ce_bwd_kernel serves both.  eps arrives by value: a captured graph freezes it.
__global__ __launch_bounds__(256) void ce_soft_fwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt,
                                                          const int64_t* __restrict__ tgt_b,
                                                          const float* __restrict__ lam, float eps, int B, int K,
                                                          int64_t ignore, float* __restrict__ dl,
                                                          float* __restrict__ rowloss, float* __restrict__ loss,
                                                          float* __restrict__ inv, unsigned* __restrict__ ctr,
                                                          float* __restrict__ acc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kCeRowsPerWg + wave;
  if (b < B) {
    const float* xr = x + (int64_t)b * K;
    float* dr = dl + (int64_t)b * K;
    const int64_t ta = tgt[b];
    const int64_t tb = tgt_b != nullptr ? tgt_b[b] : ta;
    const float l = tgt_b != nullptr ? lam[b] : 1.f;
    const bool valid = ta != ignore;
    const bool in_range = ta >= 0 && ta < K && tb >= 0 && tb < K;
    const float wa = (1.f - eps) * l, wb = (1.f - eps) * (1.f - l);  // wb = 0 with one target
    const float uni = eps / (float)K;
    float m = -INFINITY, s = 0.f, sx = 0.f, lse;
    if (K <= 64 * kCeRegs) {  // the row in registers: one load pass
      float v[kCeRegs];
#pragma unroll
      for (int i = 0; i < kCeRegs; ++i) {
        const int k = lane + 64 * i;
        v[i] = k < K ? xr[k] : -INFINITY;
        m = fmaxf(m, v[i]);
        sx += k < K ? v[i] : 0.f;
      }
      m = wave_max_f(m);
#pragma unroll
      for (int i = 0; i < kCeRegs; ++i) s += lane + 64 * i < K ? expf(v[i] - m) : 0.f;
      s = wave_sum_f(s);
      lse = m + logf(s);
#pragma unroll
      for (int i = 0; i < kCeRegs; ++i) {
        const int k = lane + 64 * i;
        if (k < K) {
          const float hard = (k == ta ? wa : 0.f) + (k == tb ? wb : 0.f);
          dr[k] = valid ? (expf(v[i] - lse) - hard) - uni : 0.f;
        }
      }
    } else {
      for (int k = lane; k < K; k += 64) {
        const float xv = xr[k];
        m = fmaxf(m, xv);
        sx += xv;
      }
      m = wave_max_f(m);
      for (int k = lane; k < K; k += 64) s += expf(xr[k] - m);
      s = wave_sum_f(s);
      lse = m + logf(s);
      for (int k = lane; k < K; k += 64) {
        const float hard = (k == ta ? wa : 0.f) + (k == tb ? wb : 0.f);
        dr[k] = valid ? (expf(xr[k] - lse) - hard) - uni : 0.f;
      }
    }
    sx = wave_sum_f(sx);
    if (lane == 0) {  // sc1 (write-through) store: read back by the last workgroup below
      float rl = 0.f;
      if (valid) {
        rl = __builtin_nanf("");
        if (in_range) {
          const float la = lse - xr[ta];
          const float hard = tgt_b != nullptr ? l * la + (1.f - l) * (lse - xr[tb]) : la;
          rl = (1.f - eps) * hard + eps * (lse - sx / (float)K);
        }
      }
      __hip_atomic_store(rowloss + b, rl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // last-arriving workgroup: ce_fwd_kernel's ticket and fixed-order mean
  if (!arrive_last(ctr, gridDim.x)) return;
  __shared__ float red[2][4];
  float a = 0.f, n = 0.f;
  for (int r = threadIdx.x; r < B; r += 256) {
    a += __hip_atomic_load(rowloss + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    n += tgt[r] != ignore ? 1.f : 0.f;
  }
  a = wave_sum_f(a);
  n = wave_sum_f(n);
  if (lane == 0) {
    red[0][wave] = a;
    red[1][wave] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float tot = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    const float cnt = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    loss[0] = tot / cnt;  // 0 / 0 = NaN when every row is ignored, like PyTorch
    if (acc != nullptr) acc[0] += tot / cnt;
    inv[0] = 1.f / cnt;
    arrive_rearm(ctr);
  }
}

__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ dl, const float* __restrict__ g,
                                                     const float* __restrict__ inv, float* __restrict__ dx,
                                                     int64_t n) {
  const float sc = g[0] * inv[0];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (4 * i + 3 < n) {
    const f4ce v = reinterpret_cast<const f4ce*>(dl)[i];
    reinterpret_cast<f4ce*>(dx)[i] = v * sc;
  } else {
    for (int64_t j = 4 * i; j < n; ++j) dx[j] = dl[j] * sc;
  }
}

// ---- fused evaluation metrics: loss sum, valid rows, top-1 / top-k correct -----------------
// ATen spends about eight launches and a host sync per batch on cross_entropy + topk + eq + sum
// + .item().  One launch of the ce_fwd shape (one wave per row, 4 rows per workgroup) instead:
//   lse as in ce_fwd, row loss = lse - x[t] (fp32), and the target's rank
//     rank = #{j : x[j] > x[t]} + #{j < t : x[j] == x[t]}
//   (top-1 correct iff rank == 0, which is "first maximum == t", top-k correct iff rank < k: ties
//   resolve towards the lower index, deterministically).  A row that holds a NaN or whose target
//   is outside [0, K) is incorrect at every k (rank = K) and its loss is NaN.  pred[b] (optional)
//   is the index of the first maximum (a NaN counts as the maximum, like torch.argmax);
//   rows whose target is ignore_index get pred = ignore_index and contribute nothing.
//   (loss, rank) per row cross workgroups through sc1 stores; the last-arriving workgroup (the
//   ce_fwd ticket, re-armed) adds them in a fixed order, the loss in fp64, and does
//   state += [loss_sum, n_valid, correct1, correctk]: a whole validation pass accumulates on
//   the device with no host sync, bitwise reproducible and hipGraph-replay safe.
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// argmax key: larger value first (NaN above everything, -0 == +0), then the lower index
__device__ __forceinline__ unsigned long long argmax_key(float v, int k) {
  unsigned u;
  if (v != v) {
    u = 0xffffffffu;
  } else {
    const unsigned bits = __float_as_uint(v + 0.f);
    u = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  }
  return ((unsigned long long)u << 32) | (unsigned)(0x7fffffff - k);
}

__global__ __launch_bounds__(256) void cls_metrics_kernel(const float* __restrict__ x,
                                                          const int64_t* __restrict__ tgt, int B, int K,
                                                          int64_t ignore, int topk, double* __restrict__ state,
                                                          float* __restrict__ rowbuf, unsigned* __restrict__ ctr,
                                                          int64_t* __restrict__ pred) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kCeRowsPerWg + wave;
  int* rowrank = reinterpret_cast<int*>(rowbuf + B);
  if (b < B) {
    const float* xr = x + (int64_t)b * K;
    const int64_t t = tgt[b];
    const bool valid = t != ignore;
    const bool in_range = t >= 0 && t < K;
    float rl = 0.f;
    int rank = -1;  // ignored row
    if (valid) {    // wave-uniform
      const float xt = in_range ? xr[t] : __builtin_nanf("");
      float m = -INFINITY, s = 0.f, lse;
      int cnt = 0, bad = 0;
      unsigned long long best = 0ull;
      if (K <= 64 * kCeRegs) {  // the row in registers: one load pass
        float v[kCeRegs];
#pragma unroll
        for (int i = 0; i < kCeRegs; ++i) {
          const int k = lane + 64 * i;
          v[i] = k < K ? xr[k] : -INFINITY;
          m = fmaxf(m, v[i]);
          if (k < K) {
            const unsigned long long key = argmax_key(v[i], k);
            best = key > best ? key : best;
            bad |= v[i] != v[i];
            cnt += (v[i] > xt || (v[i] == xt && k < t)) ? 1 : 0;
          }
        }
        m = wave_max_f(m);
#pragma unroll
        for (int i = 0; i < kCeRegs; ++i) s += lane + 64 * i < K ? expf(v[i] - m) : 0.f;
      } else {
        for (int k = lane; k < K; k += 64) {
          const float xv = xr[k];
          m = fmaxf(m, xv);
          const unsigned long long key = argmax_key(xv, k);
          best = key > best ? key : best;
          bad |= xv != xv;
          cnt += (xv > xt || (xv == xt && k < t)) ? 1 : 0;
        }
        m = wave_max_f(m);
        for (int k = lane; k < K; k += 64) s += expf(xr[k] - m);
      }
      s = wave_sum_f(s);
      lse = m + logf(s);
      cnt = wave_sum_i(cnt);
      bad = wave_sum_i(bad);
      best = wave_max_u64(best);
      const bool ok = in_range && bad == 0;
      rl = ok ? lse - xt : __builtin_nanf("");
      rank = ok ? cnt : K;
      if (pred != nullptr && lane == 0) pred[b] = (int64_t)(0x7fffffff - (int)(unsigned)(best & 0xffffffffull));
    } else if (pred != nullptr && lane == 0) {
      pred[b] = ignore;
    }
    if (lane == 0) {  // sc1 (write-through) stores: read back by the last workgroup below
      __hip_atomic_store(rowbuf + b, rl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(rowrank + b, rank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // last-arriving workgroup: the ce_fwd ticket, then a fixed-order sum over the rows, the loss in fp64
  if (!arrive_last(ctr, gridDim.x)) return;
  __shared__ double redl[4];
  __shared__ int redc[3][4];
  double a = 0.0;
  int n = 0, c1 = 0, ck = 0;
  for (int r = threadIdx.x; r < B; r += 256) {
    const int rk = __hip_atomic_load(rowrank + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float l = __hip_atomic_load(rowbuf + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (rk >= 0) {
      a += (double)l;
      n += 1;
      c1 += rk == 0 ? 1 : 0;
      ck += rk < topk ? 1 : 0;
    }
  }
  a = wave_sum_d(a);
  n = wave_sum_i(n);
  c1 = wave_sum_i(c1);
  ck = wave_sum_i(ck);
  if (lane == 0) {
    redl[wave] = a;
    redc[0][wave] = n;
    redc[1][wave] = c1;
    redc[2][wave] = ck;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    state[0] += ((redl[0] + redl[1]) + redl[2]) + redl[3];
    state[1] += (double)(redc[0][0] + redc[0][1] + redc[0][2] + redc[0][3]);
    state[2] += (double)(redc[1][0] + redc[1][1] + redc[1][2] + redc[1][3]);
    state[3] += (double)(redc[2][0] + redc[2][1] + redc[2][2] + redc[2][3]);
    arrive_rearm(ctr);
  }
}

void launch_ce_fwd(const float* x, const int64_t* tgt, int B, int K, int64_t ignore, float* dl, float* rowloss,
                   float* loss, float* inv, unsigned* ctr, hipStream_t s, float* acc) {
  const unsigned wgs = (unsigned)((B + kCeRowsPerWg - 1) / kCeRowsPerWg);
  hipLaunchKernelGGL(ce_fwd_kernel, dim3(wgs), dim3(256), 0, s, x, tgt, B, K, ignore, dl, rowloss, loss, inv, ctr,
                     acc);
}

void launch_ce_soft_fwd(const float* x, const int64_t* tgt, const int64_t* tgt_b, const float* lam, float eps, int B,
                        int K, int64_t ignore, float* dl, float* rowloss, float* loss, float* inv, unsigned* ctr,
                        hipStream_t s, float* acc) {
  const unsigned wgs = (unsigned)((B + kCeRowsPerWg - 1) / kCeRowsPerWg);
  hipLaunchKernelGGL(ce_soft_fwd_kernel, dim3(wgs), dim3(256), 0, s, x, tgt, tgt_b, lam, eps, B, K, ignore, dl,
                     rowloss, loss, inv, ctr, acc);
}

void launch_ce_bwd(const float* dl, const float* g, const float* inv, float* dx, int64_t n, hipStream_t s) {
  const int64_t n4 = (n + 3) / 4;
  hipLaunchKernelGGL(ce_bwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, dl, g, inv, dx, n);
}

void launch_cls_metrics(const float* x, const int64_t* tgt, int B, int K, int64_t ignore, int k, double* state,
                        float* rowbuf, unsigned* ctr, int64_t* pred, hipStream_t s) {
  const unsigned wgs = (unsigned)((B + kCeRowsPerWg - 1) / kCeRowsPerWg);
  hipLaunchKernelGGL(cls_metrics_kernel, dim3(wgs), dim3(256), 0, s, x, tgt, B, K, ignore, k, state, rowbuf, ctr,
                     pred);
}

}  // namespace ndp
