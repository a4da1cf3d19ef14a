// Convolution kernels for ResNet on CIFAR-shape inputs (NCHW fp32, gfx950).
//
// ResNet-18 on 32x32 images runs layer3/layer4 at 4x4 -> 2x2 -> 1x1 feature maps, where a
// 3x3 convolution is really a small dense matrix product ("Toeplitz" form, see
// models/conv_gemm.py):  out.view(B, Co*OH*OW) = x.view(B, C*H*W) @ W_big with
//   W_big[(ci,ih,iw), (co,oh,ow)] = W[co, ci, ih - oh*s + p, iw - ow*s + p]   (0 outside).
// The GEMMs run on hipBLASLt; these two kernels build W_big from W and fold grad-W_big back
// into grad-W with index arithmetic (no index tensors, no torch.cat / fill / gather /
// scatter chains: profiles/ showed ~0.6 ms per ResNet-18 step in those ATen launches).
// The fold sums the <= OH*OW taps of each weight in a fixed order: deterministic.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <utility>

#include "ndp_kernels.h"
#include "ds_stream.h"
#include "wino_dpp.h"

namespace ndp {

typedef float f32x4e __attribute__((ext_vector_type(4)));

// Device orientation: Wt_big = W_big^T, [N = Co*OH*OW rows][K = C*H*W cols], so that both
// kernels walk contiguous memory on both sides (a row of Wt_big reads one filter W[co]).
// grid: (ceil(K/256), N); one thread per Wt_big element
__global__ __launch_bounds__(256) void toeplitz_expand_kernel(const float* __restrict__ w, float* __restrict__ wt,
                                                              ConvGeom g) {
  const int K = g.C * g.H * g.W;
  const int kcol = blockIdx.x * 256 + threadIdx.x;
  if (kcol >= K) return;
  const int n = blockIdx.y;
  const int OHW = g.OH * g.OW;
  const int co = n / OHW, ohw = n - co * OHW;
  const int oh = ohw / g.OW, ow = ohw - oh * g.OW;
  const int HW = g.H * g.W;
  const int ci = kcol / HW, ihw = kcol - ci * HW;
  const int ih = ihw / g.W, iw = ihw - ih * g.W;
  const int kh = ih - oh * g.stride + g.pad, kw = iw - ow * g.stride + g.pad;
  float v = 0.f;
  if (kh >= 0 && kh < g.KH && kw >= 0 && kw < g.KW) v = w[((co * g.C + ci) * g.KH + kh) * g.KW + kw];
  wt[(int64_t)n * K + kcol] = v;
}

// Every Toeplitz layer of a model in ONE launch (forward start, ToeplitzBank in
// models/conv_gemm.py).  One workgroup per W_big^T row n = (co, oh, ow) of one layer (the
// layer is found by scanning the <= kMaxExpand row prefix sums in the kernel arguments — no
// table upload); thread t owns input channels ci = t, t + 256, ... and writes their H*W
// contiguous columns (one float4 per 4 columns for the 2x2 / 4x4 maps): all index math is
// per row or per channel, none per element.
template <int H, int W>
__device__ __forceinline__ void expand_row(const float* __restrict__ w, float* __restrict__ row, const ConvGeom& g,
                                           int co, int oh, int ow) {
  const int h0 = oh * g.stride - g.pad, w0 = ow * g.stride - g.pad;
  for (int ci = threadIdx.x; ci < g.C; ci += 256) {
    const float* wc = w + ((int64_t)co * g.C + ci) * g.KH * g.KW;
    float v[H * W];
#pragma unroll
    for (int ih = 0; ih < H; ++ih)
#pragma unroll
      for (int iw = 0; iw < W; ++iw) {
        const int kh = ih - h0, kw = iw - w0;
        v[ih * W + iw] = (kh >= 0 && kh < g.KH && kw >= 0 && kw < g.KW) ? wc[kh * g.KW + kw] : 0.f;
      }
    float* d = row + (int64_t)ci * (H * W);
    if constexpr ((H * W) % 4 == 0) {
#pragma unroll
      for (int j = 0; j < H * W; j += 4)
        *reinterpret_cast<f32x4e*>(d + j) = f32x4e{v[j], v[j + 1], v[j + 2], v[j + 3]};
    } else {
#pragma unroll
      for (int j = 0; j < H * W; ++j) d[j] = v[j];
    }
  }
}

__global__ __launch_bounds__(256) void toeplitz_expand_many_kernel(ExpandBatch b) {
  const int64_t r = blockIdx.x;
  int e = 0;
  while (e + 1 < b.n && r >= b.end[e]) ++e;
  const ConvGeom& g = b.g[e];
  const int n = (int)(r - (e ? b.end[e - 1] : 0));
  const int OHW = g.OH * g.OW;
  const int co = n / OHW, ohw = n - co * OHW;
  const int oh = ohw / g.OW, ow = ohw - oh * g.OW;
  float* row = b.wt[e] + (int64_t)n * g.C * g.H * g.W;
  if (g.H == 1 && g.W == 1) expand_row<1, 1>(b.w[e], row, g, co, oh, ow);
  else if (g.H == 2 && g.W == 2) expand_row<2, 2>(b.w[e], row, g, co, oh, ow);
  else if (g.H == 4 && g.W == 4) expand_row<4, 4>(b.w[e], row, g, co, oh, ow);
  else {
    const int K = g.C * g.H * g.W, HW = g.H * g.W;
    for (int kcol = threadIdx.x; kcol < K; kcol += 256) {
      const int ci = kcol / HW, ihw = kcol - ci * HW;
      const int ih = ihw / g.W, iw = ihw - ih * g.W;
      const int kh = ih - oh * g.stride + g.pad, kw = iw - ow * g.stride + g.pad;
      float v = 0.f;
      if (kh >= 0 && kh < g.KH && kw >= 0 && kw < g.KW) v = b.w[e][((co * g.C + ci) * g.KH + kh) * g.KW + kw];
      row[kcol] = v;
    }
  }
}

// kExpandRows consecutive W_big^T rows of one layer per workgroup, the 256 threads over the
// rows' (row, ci) pairs: a one-row workgroup left half its threads idle at C = 128 and spent
// its time on the layer scan and index setup for 2-8 KB of stores (21.6 µs per ResNet-18
// forward for ~35 MB, 1.6 TB/s; profiles/r4).  Consecutive threads write consecutive H*W-float
// segments of a row: coalesced.  What remains (~19 µs at batch 64): PMC shows 42 MB READ for
// 37 MB written — layer4's 1x1-map layers use only the centre tap, but every cache line of
// their [co][ci][3][3] weights is fetched to extract it; issuing 2-4 pairs' loads per thread
// before their stores changed nothing (measured).
constexpr int kExpandRows = 8;
template <int H, int W>
__device__ __forceinline__ void expand_rows(const float* __restrict__ w, float* __restrict__ wt, const ConvGeom& g,
                                            int n0) {
  const int C = g.C, OHW = g.OH * g.OW;
  const int64_t K = (int64_t)C * H * W;
  for (int idx = threadIdx.x; idx < kExpandRows * C; idx += 256) {
    const int rr = idx / C, ci = idx - rr * C;
    const int n = n0 + rr;
    const int co = n / OHW, ohw = n - co * OHW;
    const int oh = ohw / g.OW, ow = ohw - oh * g.OW;
    const int h0 = oh * g.stride - g.pad, w0 = ow * g.stride - g.pad;
    const float* wc = w + ((int64_t)co * C + ci) * g.KH * g.KW;
    float v[H * W];
#pragma unroll
    for (int ih = 0; ih < H; ++ih)
#pragma unroll
      for (int iw = 0; iw < W; ++iw) {
        const int kh = ih - h0, kw = iw - w0;
        v[ih * W + iw] = (kh >= 0 && kh < g.KH && kw >= 0 && kw < g.KW) ? wc[kh * g.KW + kw] : 0.f;
      }
    float* d = wt + (int64_t)n * K + (int64_t)ci * (H * W);
    if constexpr ((H * W) % 4 == 0) {
#pragma unroll
      for (int j = 0; j < H * W; j += 4)
        *reinterpret_cast<f32x4e*>(d + j) = f32x4e{v[j], v[j + 1], v[j + 2], v[j + 3]};
    } else {
#pragma unroll
      for (int j = 0; j < H * W; ++j) d[j] = v[j];
    }
  }
}

__global__ __launch_bounds__(256) void toeplitz_expand_rows_kernel(ExpandBatch b) {
  const int64_t r0 = (int64_t)blockIdx.x * kExpandRows;
  int e = 0;
  while (e + 1 < b.n && r0 >= b.end[e]) ++e;
  const ConvGeom& g = b.g[e];
  const int n0 = (int)(r0 - (e ? b.end[e - 1] : 0));
  if (g.H == 1 && g.W == 1) expand_rows<1, 1>(b.w[e], b.wt[e], g, n0);
  else if (g.H == 2 && g.W == 2) expand_rows<2, 2>(b.w[e], b.wt[e], g, n0);
  else expand_rows<4, 4>(b.w[e], b.wt[e], g, n0);
}

void launch_toeplitz_expand_many(const ExpandBatch& b, hipStream_t s) {
  if (b.n <= 0) return;
  bool rows_ok = true;  // every layer's rows split into whole groups of the covered map sizes
  for (int e = 0; e < b.n; ++e) {
    const ConvGeom& g = b.g[e];
    const int64_t rows = b.end[e] - (e ? b.end[e - 1] : 0);
    rows_ok = rows_ok && rows % kExpandRows == 0 && g.H == g.W && (g.H == 1 || g.H == 2 || g.H == 4);
  }
  if (rows_ok)
    hipLaunchKernelGGL(toeplitz_expand_rows_kernel, dim3((unsigned)(b.end[b.n - 1] / kExpandRows)), dim3(256), 0, s,
                       b);
  else
    hipLaunchKernelGGL(toeplitz_expand_many_kernel, dim3((unsigned)b.end[b.n - 1]), dim3(256), 0, s, b);
}

// One thread per (co, ci) weight PAIR: it reads, for every output position (oh, ow), the
// H*W contiguous dWt_big columns of input channel ci (row n = (co, oh, ow)) — lanes with
// consecutive ci read consecutive segments, fully coalesced — and accumulates them into
// its KH*KW taps in registers (the same (oh, ow)-ascending order per tap as the one-thread-
// per-weight fold, so results are bitwise identical); then writes its KH*KW contiguous
// weights.  Toeplitz layers have KH, KW <= 3 and H*W <= 16.
constexpr int kFoldMaxTaps = 9;
__device__ __forceinline__ void fold_pair(const float* __restrict__ dwt, const ConvGeom& g, int pair,
                                          float (&acc)[kFoldMaxTaps]) {
  const int co = pair / g.C, ci = pair - co * g.C;
  const int K = g.C * g.H * g.W, HW = g.H * g.W;
#pragma unroll
  for (int t = 0; t < kFoldMaxTaps; ++t) acc[t] = 0.f;
  for (int oh = 0; oh < g.OH; ++oh)
    for (int ow = 0; ow < g.OW; ++ow) {
      const float* row = dwt + (int64_t)((co * g.OH + oh) * g.OW + ow) * K + ci * HW;
      for (int ih = 0; ih < g.H; ++ih) {
        const int kh = ih - oh * g.stride + g.pad;
        if (kh < 0 || kh >= g.KH) continue;
        for (int iw = 0; iw < g.W; ++iw) {
          const int kw = iw - ow * g.stride + g.pad;
          if (kw < 0 || kw >= g.KW) continue;
          const float v = row[ih * g.W + iw];
#pragma unroll
          for (int t = 0; t < kFoldMaxTaps; ++t)
            if (t == kh * g.KW + kw) acc[t] += v;
        }
      }
    }
}

// The same fold with the geometry at compile time (ResNet-18/34 layer3 / layer4 Toeplitz
// shapes): every tap test resolves statically and the <= OH*OW*H*W loads of a pair issue
// together instead of behind a runtime-bounded loop (the generic fold ran at 1.4 TB/s).
// Same (oh, ow, ih, iw) accumulation order per tap: bitwise equal to fold_pair.
template <int H, int W, int OH, int OW, int ST, int PD, int KH, int KW>
__device__ __forceinline__ void fold_pair_t(const float* __restrict__ dwt, int C, int pair,
                                            float (&acc)[kFoldMaxTaps]) {
  const int co = pair / C, ci = pair - co * C;
  const int64_t K = (int64_t)C * H * W;
#pragma unroll
  for (int t = 0; t < kFoldMaxTaps; ++t) acc[t] = 0.f;
  float v[OH * OW][H * W];
#pragma unroll
  for (int oh = 0; oh < OH; ++oh)
#pragma unroll
    for (int ow = 0; ow < OW; ++ow) {
      const float* row = dwt + (int64_t)((co * OH + oh) * OW + ow) * K + (int64_t)ci * (H * W);
#pragma unroll
      for (int ih = 0; ih < H; ++ih)
#pragma unroll
        for (int iw = 0; iw < W; ++iw) {
          const int kh = ih - oh * ST + PD, kw = iw - ow * ST + PD;
          v[oh * OW + ow][ih * W + iw] = (kh >= 0 && kh < KH && kw >= 0 && kw < KW) ? row[ih * W + iw] : 0.f;
        }
    }
#pragma unroll
  for (int oh = 0; oh < OH; ++oh)
#pragma unroll
    for (int ow = 0; ow < OW; ++ow)
#pragma unroll
      for (int ih = 0; ih < H; ++ih)
#pragma unroll
        for (int iw = 0; iw < W; ++iw) {
          const int kh = ih - oh * ST + PD, kw = iw - ow * ST + PD;
          if (kh >= 0 && kh < KH && kw >= 0 && kw < KW) acc[kh * KW + kw] += v[oh * OW + ow][ih * W + iw];
        }
}

__device__ __forceinline__ void fold_any(const float* __restrict__ dwt, const ConvGeom& g, int pair,
                                         float (&acc)[kFoldMaxTaps]) {
  const bool k3 = g.KH == 3 && g.KW == 3 && g.pad == 1, k1 = g.KH == 1 && g.KW == 1 && g.pad == 0;
  if (k3 && g.H == 2 && g.W == 2 && g.stride == 1) fold_pair_t<2, 2, 2, 2, 1, 1, 3, 3>(dwt, g.C, pair, acc);
  else if (k3 && g.H == 4 && g.W == 4 && g.stride == 2) fold_pair_t<4, 4, 2, 2, 2, 1, 3, 3>(dwt, g.C, pair, acc);
  else if (k1 && g.H == 4 && g.W == 4 && g.stride == 2) fold_pair_t<4, 4, 2, 2, 2, 0, 1, 1>(dwt, g.C, pair, acc);
  else if (k3 && g.H == 2 && g.W == 2 && g.stride == 2) fold_pair_t<2, 2, 1, 1, 2, 1, 3, 3>(dwt, g.C, pair, acc);
  else if (k1 && g.H == 2 && g.W == 2 && g.stride == 2) fold_pair_t<2, 2, 1, 1, 2, 0, 1, 1>(dwt, g.C, pair, acc);
  else if (k3 && g.H == 1 && g.W == 1 && g.stride == 1) fold_pair_t<1, 1, 1, 1, 1, 1, 3, 3>(dwt, g.C, pair, acc);
  else fold_pair(dwt, g, pair, acc);
}

// Every deferred grad-W fold of a backward pass in ONE launch (ops/gradfinish.py): flat
// grid over all layers' (co, ci) pairs, the layer found from the <= kMaxExpand prefix sums
// in the kernel arguments.  A workgroup's 256 pairs own one contiguous run of 256 * KH*KW
// weights, so the taps go through LDS and leave as coalesced float stores (a lane writing
// its own 9 weights would stride the wave's stores by 36 B).
__device__ __forceinline__ void fold_many_block(const FoldBatch& b, int64_t blk, float* __restrict__ stage) {
  const int64_t base = blk * 256;
  const int64_t i = base + threadIdx.x;
  const int64_t total = b.end[b.n - 1];
  int e = 0;
  while (e + 1 < b.n && base >= b.end[e]) ++e;  // the workgroup's first entry
  const int64_t e_lo = e ? b.end[e - 1] : 0;
  const bool one_entry = base + 256 <= b.end[e];  // whole workgroup inside entry e
  if (one_entry) {
    const ConvGeom& g = b.g[e];
    const int T = g.KH * g.KW;
    float acc[kFoldMaxTaps];
    fold_any(b.dwt[e], g, (int)(i - e_lo), acc);
#pragma unroll
    for (int t = 0; t < kFoldMaxTaps; ++t)
      if (t < T) stage[threadIdx.x * T + t] = acc[t];
    __syncthreads();
    float* out = b.dw[e] + (base - e_lo) * T;
    for (int k = threadIdx.x; k < 256 * T; k += 256) out[k] = stage[k];
    return;
  }
  if (i >= total) return;  // straddling workgroup: direct per-lane writes
  while (e + 1 < b.n && i >= b.end[e]) ++e;
  const ConvGeom& g = b.g[e];
  const int T = g.KH * g.KW;
  const int pair = (int)(i - (e ? b.end[e - 1] : 0));
  float acc[kFoldMaxTaps];
  fold_any(b.dwt[e], g, pair, acc);
  float* out = b.dw[e] + (int64_t)pair * T;
#pragma unroll
  for (int t = 0; t < kFoldMaxTaps; ++t)
    if (t < T) out[t] = acc[t];
}

__global__ __launch_bounds__(256) void toeplitz_fold_many_kernel(FoldBatch b) {
  __shared__ float stage[256 * kFoldMaxTaps];
  fold_many_block(b, blockIdx.x, stage);
}

void launch_toeplitz_fold_many(const FoldBatch& b, hipStream_t s) {
  if (b.n <= 0) return;
  const int64_t total = b.end[b.n - 1];  // (co, ci) pairs
  hipLaunchKernelGGL(toeplitz_fold_many_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, b);
}

void launch_toeplitz_expand(const float* w, float* wb, const ConvGeom& g, hipStream_t s) {
  const int N = g.Co * g.OH * g.OW, K = g.C * g.H * g.W;
  hipLaunchKernelGGL(toeplitz_expand_kernel, dim3((K + 255) / 256, N), dim3(256), 0, s, w, wb, g);
}

void launch_toeplitz_fold(const float* dwb, float* dw, const ConvGeom& g, hipStream_t s) {
  FoldBatch b{};
  b.dwt[0] = dwb;
  b.dw[0] = dw;
  b.g[0] = g;
  b.end[0] = (int64_t)g.Co * g.C;
  b.n = 1;
  launch_toeplitz_fold_many(b, s);
}

// =====================================================================================
// Direct (implicit-GEMM) convolutions on v_mfma_f32_32x32x2_f32 — exact f32, NCHW.
//
// ResNet-18 on 32x32 images runs its stem at 16x16 and layer1/layer2 at 8x8 / 4x4 maps
// with 64-128 channels.  MIOpen's fp32 paths for these shapes are Winograd (fwd / grad-x)
// and NHWC implicit-GEMM (grad-W) kernels that need NCHW<->NHWC transposes and zero-fill
// passes around every call (profiles/: ~1.1 ms of a 2.7 ms step).  Here each direction is
// one launch on the matrix cores, reading and writing NCHW directly:
//
// forward  Y[k, (b,p,q)] = sum_{c,r,s} W[k,c,r,s] * Xpad[b, c, p*st + r, q*st + s]
//   GEMM  M = out channels (tile BM), N = output pixels of IMGS whole images, K = C*R*S
//   chunked by CK input channels.  Per chunk the workgroup stages
//     A: W[m0:m0+BM, c0:c0+CK, :, :] transposed to [kk][m] (row stride BM+1: conflict-free
//        transposing writes and conflict-free MFMA reads),
//     B: the raw input planes x[b, c0:c0+CK] into a zero-bordered [img][c][Hp][Wp] image,
//        so the im2col operand is ONE ds_read_b32 at (per-lane pixel base + compile-time
//        tap offset): no bounds checks, no im2col buffer.
//   The two k-values of each MFMA (lane halves) are channels c and c + CK/2 at the same
//   tap, so both halves' addresses differ by a constant and every tap offset is an
//   immediate.  Global loads of chunk i+1 are issued before the MFMAs of chunk i and
//   written to the other LDS buffer after them (one barrier per chunk).
// grad-x (stride 1) is the same kernel on dY with the weight transposed and flipped
//   (TRANSW):  dX[c, (b,h,w)] = sum_{k,r,s} W[k, c, R-1-r, S-1-s] * dYpad[b, k, h + r, w + s]
//   with pad' = R-1-pad.
// grad-W   dW[k, (c,r,s)] = sum_{b,p,q} dY[b,k,p,q] * Xpad[b, c, p*st + r, q*st + s]
//   M = out channels (BM), N = (c,r,s) flattened (CB channels x R*S taps, 32-wide blocks;
//   each lane carries its (c,r,s) as an LDS base offset), K = pixels, two pixels per MFMA:
//   rows p and p + P/2.  The batch is split into slices; every slice writes its partial
//   dW tile to a slab and conv_slab_sum adds the slabs in slice order (deterministic).
// =====================================================================================

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4c __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  // D(32x32) += A(32x2) * B(2x32); lane l supplies A[l&31][l>>5] and B[l>>5][l&31];
  // D: col = l&31, row = (reg&3) + 8*(reg>>2) + 4*(l>>5)
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// PSPLIT (one image per tile only): the tile covers P / PSPLIT output rows of its image
// (blockIdx.x = image * PSPLIT + row block); the whole image is still staged in LDS.  The stem at
// small per-GPU batches: one 16x16-output image per workgroup left 3/4 of the CUs idle at batch 64.
// One forward / grad-x kernel configuration as a type: the parameters of conv_fwd_body (described below) and
// the LDS geometry they imply.  The shape classes (further down) name each one once; all else reads it here.
template <int R_, int S_, int ST_, int PD_, int H_, int W_, int CK_, int BM_, int IMGS_, int WM_, int NBUF_, int KB_,
          bool TRANSW_, bool VEC_, int UPS_ = 1, int SCH_ = 0, int IUPS_ = 1, int PSPLIT_ = 1>
struct FwdTile {
  static constexpr int R = R_, S = S_, ST = ST_, PD = PD_, H = H_, W = W_, CK = CK_, BM = BM_, IMGS = IMGS_, WM = WM_,
                       NBUF = NBUF_, KB = KB_, UPS = UPS_, SCH = SCH_, IUPS = IUPS_, PSPLIT = PSPLIT_;
  static constexpr bool TRANSW = TRANSW_, VEC = VEC_;
  // the same tile on the transposed, flipped weights (grad-x of a stride-1 conv), on a zero-inserted
  // half-size input (IUPS), in row blocks of one image (PSPLIT)
  using transposed = FwdTile<R, S, ST, PD, H, W, CK, BM, IMGS, WM, NBUF, KB, !TRANSW, VEC, UPS, SCH, IUPS, PSPLIT>;
  template <int N>
  using iups = FwdTile<R, S, ST, PD, H, W, CK, BM, IMGS, WM, NBUF, KB, TRANSW, VEC, UPS, SCH, N, PSPLIT>;
  template <int N>
  using psplit = FwdTile<R, S, ST, PD, H, W, CK, BM, IMGS, WM, NBUF, KB, TRANSW, VEC, UPS, SCH, IUPS, N>;
  static constexpr int P = (H + 2 * PD - R) / ST + 1, Q = (W + 2 * PD - S) / ST + 1, PQ = P * Q;
  static_assert(PSPLIT == 1 || (IMGS == 1 && P % PSPLIT == 0), "row blocks of one image");
  // Bank-conflict-free LDS image (ds_read_b32: bank = dword % 32, one 32-lane half-wave per
  // LDS cycle; the B read of a half-wave is 32 output pixels at pixel_base + tap):
  //  * 8x8 stride 1, one image per tile: lanes cover 8 rows x 4 columns (MAP 1) of a
  //    12-wide row stride -> row offsets 12p mod 32 = {0,12,24,4,16,28,8,20}: 32 banks;
  //  * 4x4 stride 1, 2 images per half-wave: row stride 8 (4 rows x 4 columns = banks
  //    {0-3, 8-11, 16-19, 24-27}) and an image stride = 4 (mod 32) for the second image;
  //  * 8x8 stride 2, 2 images per half-wave: row stride 12 (rows 24p = {0,24,16,8} mod 32,
  //    even columns -> the 16 even banks) and an image stride = 1 (mod 32): odd banks.
  // (Measured before: 34-54 % of LDS cycles were conflict cycles, profiles/r2/pmc_counters.md.)
  //  * 32x32 stride 2 (the 7x7 stem): the even and odd columns of each padded row are stored
  //    apart (DEINT: position (col & 1) * HALF + col / 2, row stride 2 * HALF = 40), so the 16
  //    lanes of an output row read 16 CONSECUTIVE words instead of every other one, and the
  //    next output row (2 input rows = 80 words = 16 mod 32) lands on the other 16 banks
  //    (interleaved: 2-way on every B read, 47 % of LDS cycles in conflict, PMC round 4).
  static constexpr int LAYOUT = (ST == 1 && H == 8 && W == 8 && PD == 1 && IMGS == 1) ? 1
                                : (ST == 1 && H == 4 && W == 4 && IMGS % 2 == 0)      ? 2
                                : (ST == 2 && H == 8 && W == 8 && IMGS % 2 == 0)      ? 3
                                : (ST == 2 && H == 32 && W == 32 && R == 7 && IMGS == 1) ? 4
                                                                                       : 0;
  static constexpr bool DEINT = LAYOUT == 4;
  static constexpr int HALF = (W + 2 * PD + 2) / 2;  // >= every padded column's half position
  static constexpr int Hp = H + 2 * PD;
  static constexpr int Wp = LAYOUT == 1 ? 12 : LAYOUT == 2 ? 8 : LAYOUT == 3 ? 12 : DEINT ? 2 * HALF : W + 2 * PD;
  // LDS column of padded input column `col` within a row
  __device__ static __forceinline__ constexpr int cpos(int col) {
    return DEINT ? (col & 1) * HALF + (col >> 1) : col;
  }
  // channel stride odd: the B staging stores (float4 per lane -> 4 scalar ds_write_b32, a
  // 32-lane group spanning 2-8 channels) land on disjoint bank sets per channel (<= 2-way,
  // which a b32 store absorbs); the reads of a half-wave stay inside one channel
  static constexpr int HWp = (Hp * Wp) | 1, HW = H * W;
  static constexpr int IPAD0 = LAYOUT == 2 ? 4 : LAYOUT == 3 ? 1 : 0;  // target image stride mod 32
  static constexpr int IMGSTR = LAYOUT >= 2 ? (CK * HWp + 31) / 32 * 32 + IPAD0 : CK * HWp;
  static_assert(Wp >= W + 2 * PD && (!DEINT || (ST == 2 && HALF * 2 == Wp && (ST * Wp) % 32 == 16)),
                "row stride holds the zero border");
  // output pixel n of the tile -> (image, row, column)
  __device__ static __forceinline__ void pix(int n, int& img, int& p, int& q) {
    if constexpr (LAYOUT == 1) {
      img = 0;
      p = (n & 31) >> 2;
      q = (n & 3) + 4 * (n >> 5);
    } else {
      img = n / PQ;
      const int pq = n - img * PQ;
      p = pq / Q;
      q = pq - p * Q;
    }
  }
  static constexpr int RS = R * S, KK = CK * RS;
  // PAIRK (the 3-channel 7x7 stem): the two k values of an MFMA step (lane halves h = 0 / 1)
  // were channels c and c + 2 of CK = 4 (98 steps, a quarter of them on the zero 4th channel).
  // Now: steps 0-48 pair channel 0 with channel 1 at the same tap (B offset + 1 plane), steps
  // 49-55 channel 2's kernel row 3 with the zero plane (+ 1 plane), steps 56-76 channel 2's rows
  // 0-2 with its rows 4-6 (+ 4 rows): 77 steps, each half's B offset still a compile-time
  // immediate on one of two per-lane bases.  The A image is staged in the same step order.
  static constexpr bool PAIRK = DEINT && R == 7 && S == 7;
  static constexpr int NSTEP = PAIRK ? 77 : (CK / 2) * RS, NBLK = NSTEP / KB;
  static_assert(!PAIRK || (CK == 4 && 2 * NSTEP <= KK), "stem k pairing");
  // PAIRK: the (c, r, s) tap of lane half 0 at step t
  __device__ static __forceinline__ constexpr int pk_c(int t) { return t < 49 ? 0 : 2; }
  __device__ static __forceinline__ constexpr int pk_r(int t) { return t < 49 ? t / 7 : t < 56 ? 3 : (t - 56) / 7; }
  __device__ static __forceinline__ constexpr int pk_s(int t) { return t < 49 ? t % 7 : t < 56 ? t - 49 : (t - 56) % 7; }
  // PAIRK: A-image row (h * NSTEP + t) of flattened weight index kk = c * 49 + r * 7 + s, or -1
  // (kk < 147: the three real channels; branch-free, every weight of the tile is staged through it)
  __device__ static __forceinline__ int pk_row(int kk) {
    const int c = kk / 49, rem = kk - 49 * c, r = rem / 7, sc = rem - 7 * r;
    const int v2 = r == 3 ? 49 + sc : (r < 3 ? 56 + rem : NSTEP + 28 + rem);
    return c == 0 ? rem : (c == 1 ? NSTEP + rem : v2);
  }
  static constexpr int BN = IMGS * PQ / PSPLIT;
  static constexpr int WN = 4 / WM;
  static constexpr int TM = BM / 32 / WM, TN = BN / 32 / WN;
  // [kk][m] A image.  Reads (32 consecutive m) are conflict-free for any stride; the stride is
  // picked for the transposing scalar stores: forward (m fastest over 4 lanes, then kk in
  // float4 steps) LDA = 1 mod 32 -> <= 2-way; grad-x (TRANSW: 4 consecutive (m, tap) of a
  // weight row per lane) LDA = 2 mod 32 -> <= 2-way (1 mod 32 was 5-way; PMC round 3)
  static constexpr int LDA = TRANSW ? BM + 2 : BM + 1;
  // AV: [m][kk] A image instead (kk contiguous, row stride LDAM with LDAM / 4 odd: the 16 rows
  // of a ds_read_b128 phase start in disjoint 4-bank groups).  Lane half h consumes kk =
  // h * NSTEP + t at MFMA step t, so KB consecutive steps are KB / 4 ds_read_b128 per tile
  // instead of KB ds_read_b32 (each of which the MFMA chain waited on), and the forward's
  // float4 weight loads land as one ds_write_b128.  Needs KB % 4 == 0 and NSTEP % 4 == 0
  // (every 8x8 / 4x4 layer config; the 7x7 stem keeps [kk][m]).
  static constexpr bool AV = KB % 4 == 0 && ((CK / 2) * RS) % 4 == 0;
  static constexpr int LDAM = KK + (((KK / 4) % 2 == 0) ? 4 : 8);
  static constexpr int A_SZ = AV ? BM * LDAM : KK * LDA;
  static constexpr int B_SZ = IMGS * IMGSTR;
  // A staging: float4 rows when every chunk is whole channels and rows are 16-B aligned
  static constexpr int B4 = IMGS * CK * HW / 4, B_PER_T = (B4 + 255) / 256;
  static constexpr size_t LDS_BYTES = (size_t)NBUF * (A_SZ + B_SZ) * sizeof(float);
  static_assert(CK % 2 == 0 && BM % (32 * WM) == 0 && BN % (32 * WN) == 0 && TM >= 1 && TN >= 1, "tile");
  static_assert(NSTEP % KB == 0, "operand prefetch blocks");
  static_assert((W % 4 == 0 || (PD == 0 && H * W == 4)) && BM % 4 == 0, "float4 staging");
  // BatchNorm statistics epilogue (conv_fwd_kernel `stats`): the [BM][BN + 4] output tile
  // fits in the LDS the main loop used, 256 / BM threads per channel, float4 reads
  static constexpr int STATS_LDO = BN + 4, STATS_TPC = 256 / BM;
  static constexpr bool STATS_OK = 256 % BM == 0 && BN % (4 * STATS_TPC) == 0 &&
                                   (size_t)BM * STATS_LDO <= (size_t)NBUF * (A_SZ + B_SZ);
  // backward mode keeps two such tiles (dz and dz * xhat)
  static constexpr bool STATS2_OK = STATS_OK && (size_t)2 * BM * STATS_LDO <= (size_t)NBUF * (A_SZ + B_SZ);
};

// A (weights) is read straight from W: forward rows W[m][c0:c0+CK][:] (CK*RS contiguous
// floats), grad-x rows W[c][m0:m0+BM][:] (BM*RS contiguous) with the taps flipped; both are
// written transposed into the [kk][m] LDS image.  VEC=1 needs Cin % CK == 0 (float4 over
// whole channels); the stem (Cin = 3 < CK) stages scalars.
// SCH (instruction scheduling of the MFMA block, benchmarking variants): 0 = compiler default,
// 1 = __builtin_amdgcn_iglp_opt(0), 2 = pinned interleave of one MFMA and one LDS read (the
// default schedule waits on each operand read right before its MFMA: exposed LDS latency
// at 1-2 waves per SIMD)
// IUPS = 2 (grad-x of the 3x3 stride-2 conv): the input is a (H/2) x (W/2) map staged onto
// the even pixels of the H x W LDS image (the odd ones keep the zero fill), i.e. the stride-1
// correlation of the zero-inserted dY with the flipped weights:
//   dX[c, h, w] = sum_{k,r,s} W[k, c, 2-r, 2-s] * Z[k, h-1+r, w-1+s],  Z[k, 2p, 2q] = dY[k, p, q]

// (a device function of the workgroup's grid coordinates: the downsample-conv backward pairs run it
// on one part of a combined grid, launch_conv_dgrad)
template <typename G>  // G: a FwdTile
__device__ __forceinline__ void conv_fwd_body(const float* __restrict__ x, const float* __restrict__ w,
                                              float* __restrict__ y, float* __restrict__ part, int Cin, int Kout,
                                              int cps, int64_t slab, const float* __restrict__ addend,
                                              const ConvBnStats& st, const uint3 bid, const uint3 gdim,
                                              float* __restrict__ smem) {
  constexpr int S = G::S, ST = G::ST, PD = G::PD, H = G::H, W = G::W, CK = G::CK, BM = G::BM, IMGS = G::IMGS,
                WM = G::WM, NBUF = G::NBUF, KB = G::KB, UPS = G::UPS, SCH = G::SCH, IUPS = G::IUPS, PSPLIT = G::PSPLIT;
  constexpr bool TRANSW = G::TRANSW, VEC = G::VEC;
  constexpr int AE = (BM * G::KK + 3) / 4;  // float4 slots (scalar path: 4 scalars per slot)
  constexpr int A_PER_T = (AE + 255) / 256;
  float* As = smem;
  float* Bs = smem + NBUF * G::A_SZ;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int h = lane >> 5, l32 = lane & 31;
  const int m0 = bid.y * BM;
  const int b0 = (PSPLIT == 1 ? bid.x : bid.x / PSPLIT) * IMGS;
  const int prow0 = PSPLIT == 1 ? 0 : (bid.x % PSPLIT) * (G::P / PSPLIT);  // first output row
  // split-K: workgroup z reduces channel chunks [ch0, ch0 + nchunks) into output slab z
  const int ch0 = bid.z * cps;
  const int nchunks = min((Cin + CK - 1) / CK - ch0, cps);

  for (int i = tid; i < NBUF * G::B_SZ; i += 256) Bs[i] = 0.f;  // zero borders (never rewritten)

  int a_base[G::TM], b_base[G::TN], b_base2[G::PAIRK ? G::TN : 1];
#pragma unroll
  for (int tm = 0; tm < G::TM; ++tm)
    a_base[tm] = G::AV ? ((wm * G::TM + tm) * 32 + l32) * G::LDAM + h * G::NSTEP
                       : h * G::NSTEP * G::LDA + (wm * G::TM + tm) * 32 + l32;
#pragma unroll
  for (int tn = 0; tn < G::TN; ++tn) {
    const int n = (wn * G::TN + tn) * 32 + l32;
    int img, p, q;
    G::pix(n, img, p, q);
    p += prow0;
    b_base[tn] = img * G::IMGSTR + (G::PAIRK ? h : h * (CK / 2)) * G::HWp + p * ST * G::Wp + (G::DEINT ? q : q * ST);
    if constexpr (G::PAIRK) b_base2[tn] = b_base[tn] - h * G::HWp + h * 4 * G::Wp;
  }

  // B staging: float4 of the (possibly half-size, IUPS) input planes
  constexpr int IW = W / IUPS, IHW = (H / IUPS) * IW;
  constexpr int B4I = IMGS * CK * IHW / 4, BPT = (B4I + 255) / 256;
  // a 2x2 unpadded plane is one float4 stored whole (row stride Wp = W = 2)
  static_assert((IW % 4 == 0 || (PD == 0 && IUPS == 1 && IHW == 4)) && (IUPS == 1 || (ST == 1 && UPS == 1)),
                "input staging");
  // PAIRK stem: the BM x 147 weights of the tile are one contiguous run (Cin = 3): float4 loads
  // of the flat run, scattered to the paired-step rows at the LDS store (the generic scalar path
  // computed and held a 64-bit address and a branch per weight: 400+ registers, 1 wave / SIMD)
  constexpr int PKE = G::PAIRK ? BM * 3 * G::RS / 4 : 1, PK_PER_T = (PKE + 255) / 256;
  static_assert(!G::PAIRK || (BM * 3 * G::RS) % 4 == 0, "stem weight run in float4");
  f32x4c ra[A_PER_T > PK_PER_T ? A_PER_T : PK_PER_T];
  f32x4c rb[BPT];
  auto load = [&](int ch) {
    const int c0 = (ch0 + ch) * CK;
    if constexpr (G::PAIRK) {
      // (staged straight from global in store(): no register copy of the weights)
    } else
#pragma unroll
    for (int i = 0; i < A_PER_T; ++i) {
      const int e = tid + 256 * i;
      f32x4c v = {0.f, 0.f, 0.f, 0.f};
      if (e < AE) {
        if (VEC) {
          if (!TRANSW) {  // lanes: 4 rows (m) fastest, then float4 k4 along the row
            const int r = e >> 2, k4 = r % (G::KK / 4), m = 4 * (r / (G::KK / 4)) + (e & 3);
            v = *reinterpret_cast<const f32x4c*>(w + ((int64_t)(m0 + m) * Cin + c0) * G::RS + 4 * k4);
          } else {
            const int c = e / (BM * G::RS / 4), r4 = e - c * (BM * G::RS / 4);
            v = *reinterpret_cast<const f32x4c*>(w + ((int64_t)(c0 + c) * Kout + m0) * G::RS + 4 * r4);
          }
        } else {  // forward only (stem): 4 scalars, zero past Cin
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int f = 4 * e + j, m = f / G::KK, kk = f - m * G::KK;
            if (f < BM * G::KK && c0 + kk / G::RS < Cin) v[j] = w[((int64_t)(m0 + m) * Cin + c0) * G::RS + kk];
          }
        }
      }
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
      const int e = tid + 256 * i;  // float4 index within the IMGS x CK x (input plane) block
      f32x4c v = {0.f, 0.f, 0.f, 0.f};
      if (e < B4I) {
        const int img = e / (CK * IHW / 4), rem4 = e - img * (CK * IHW / 4);
        const int c = (4 * rem4) / IHW;
        if (c0 + c < Cin)
          v = *reinterpret_cast<const f32x4c*>(x + ((int64_t)(b0 + img) * Cin + c0) * IHW + 4 * rem4);
      }
      rb[i] = v;
    }
  };
  auto store = [&](int buf) {
    float* A = As + buf * G::A_SZ;
    float* B = Bs + buf * G::B_SZ;
    if constexpr (G::PAIRK) {
      const f32x4c* w4 = reinterpret_cast<const f32x4c*>(w + (int64_t)m0 * 3 * G::RS);
      for (int e = tid; e < PKE; e += 256) {
        const f32x4c v = w4[e];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int f = 4 * e + j, m = f / (3 * G::RS), kk = f - m * (3 * G::RS);
          A[G::pk_row(kk) * G::LDA + m] = v[j];
        }
      }
      for (int idx = tid; idx < 7 * BM; idx += 256)  // the zero partners of channel 2's row 3
        A[(G::NSTEP + 49 + idx / BM) * G::LDA + idx % BM] = 0.f;
    } else
#pragma unroll
    for (int i = 0; i < A_PER_T; ++i) {
      const int e = tid + 256 * i;
      if (e < AE) {
        if (VEC) {
          if (!TRANSW) {
            const int r = e >> 2, k4 = r % (G::KK / 4), m = 4 * (r / (G::KK / 4)) + (e & 3);
            if constexpr (G::AV) {
              *reinterpret_cast<f32x4c*>(A + m * G::LDAM + 4 * k4) = ra[i];
            } else {
              float* d = A + 4 * k4 * G::LDA + m;
              d[0] = ra[i].x; d[G::LDA] = ra[i].y; d[2 * G::LDA] = ra[i].z; d[3 * G::LDA] = ra[i].w;
            }
          } else {
            const int c = e / (BM * G::RS / 4), f = 4 * (e - c * (BM * G::RS / 4));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int m = (f + j) / G::RS, rs = (f + j) - m * G::RS;
              const int kk = c * G::RS + (G::RS - 1 - rs);  // flip the taps
              if constexpr (G::AV) A[m * G::LDAM + kk] = ra[i][j];
              else A[kk * G::LDA + m] = ra[i][j];
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int f = 4 * e + j, m = f / G::KK, kk = f - m * G::KK;
            if (f < BM * G::KK) {
              if constexpr (G::PAIRK) {
                const int row = G::pk_row(kk);
                if (row >= 0) A[row * G::LDA + m] = ra[i][j];
              } else if constexpr (G::AV) {
                A[m * G::LDAM + kk] = ra[i][j];
              } else {
                A[kk * G::LDA + m] = ra[i][j];
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
      const int e = tid + 256 * i;
      if (e < B4I) {
        const int img = e / (CK * IHW / 4), rem = 4 * (e - img * (CK * IHW / 4));
        const int c = rem / IHW, hw = rem - c * IHW;
        const int hh = hw / IW, ww = hw - hh * IW;
        if constexpr (G::DEINT) {
          float* d = B + img * G::IMGSTR + c * G::HWp + (hh + PD) * G::Wp;
#pragma unroll
          for (int j = 0; j < 4; ++j) d[G::cpos(ww + PD + j)] = rb[i][j];
        } else {
          float* d = B + img * G::IMGSTR + c * G::HWp + (IUPS * hh + PD) * G::Wp + IUPS * ww + PD;
          d[0] = rb[i].x; d[IUPS] = rb[i].y; d[2 * IUPS] = rb[i].z; d[3 * IUPS] = rb[i].w;
        }
      }
    }
  };

  f32x16 acc[G::TM][G::TN];
#pragma unroll
  for (int tm = 0; tm < G::TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < G::TN; ++tn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

  load(0);
  __syncthreads();  // zero fill before interior writes
  store(0);
  __syncthreads();
  for (int ch = 0; ch < nchunks; ++ch) {
    const int cur = (NBUF == 2) ? (ch & 1) : 0;
    if (NBUF == 2 && ch + 1 < nchunks) load(ch + 1);
    const float* A = As + cur * G::A_SZ;
    const float* B = Bs + cur * G::B_SZ;
    // operands of block k+1 are read from LDS while the MFMAs of block k issue
    float av[2][KB][G::TM], bv[2][KB][G::TN];
    auto fetch = [&](int blk, int slot) {
#pragma unroll
      for (int i = 0; i < KB; ++i) {
        const int t = blk * KB + i;
        int c = t / G::RS, rs = t - c * G::RS, r = rs / S, s = rs - r * S;
        if constexpr (G::PAIRK) {
          c = G::pk_c(t);
          r = G::pk_r(t);
          s = G::pk_s(t);
        }
        const int offb = c * G::HWp + r * G::Wp + (G::DEINT ? (s & 1) * G::HALF + (s >> 1) : s);
        if constexpr (!G::AV) {
#pragma unroll
          for (int tm = 0; tm < G::TM; ++tm) av[slot][i][tm] = A[a_base[tm] + t * G::LDA];
        }
#pragma unroll
        for (int tn = 0; tn < G::TN; ++tn) {
          if constexpr (G::PAIRK) bv[slot][i][tn] = B[(t < 56 ? b_base[tn] : b_base2[tn]) + offb];
          else bv[slot][i][tn] = B[b_base[tn] + offb];
        }
      }
      if constexpr (G::AV) {
#pragma unroll
        for (int tm = 0; tm < G::TM; ++tm)
#pragma unroll
          for (int q = 0; q < KB / 4; ++q) {
            const f32x4c v = *reinterpret_cast<const f32x4c*>(A + a_base[tm] + blk * KB + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) av[slot][4 * q + j][tm] = v[j];
          }
      }
    };
    if constexpr (SCH == 1) __builtin_amdgcn_iglp_opt(0);
    fetch(0, 0);
#pragma unroll
    for (int blk = 0; blk < G::NBLK; ++blk) {
      if (blk + 1 < G::NBLK) fetch(blk + 1, (blk + 1) & 1);
#pragma unroll
      for (int i = 0; i < KB; ++i)
#pragma unroll
        for (int tm = 0; tm < G::TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < G::TN; ++tn)
            acc[tm][tn] = mfma32(av[blk & 1][i][tm], bv[blk & 1][i][tn], acc[tm][tn]);
    }
    if constexpr (SCH == 2) {
#pragma unroll
      for (int i = 0; i < G::NSTEP * G::TM * G::TN; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // one LDS read
      }
    }
    if (ch + 1 < nchunks) {
      if (NBUF == 2) {
        store(cur ^ 1);
      } else {
        __syncthreads();  // everyone done reading the single buffer
        load(ch + 1);
        store(0);
      }
    }
    __syncthreads();
  }

  // split-K (gridDim.z > 1): every workgroup stores its partial tile to its slab of `part`
  // (compact [B][Kout][PQ] layout); conv_slab_sum(_ups) adds the slabs in z order
  // (deterministic).  A last-arrival fixup inside this kernel was measured 4x slower: the
  // agent-scope release fence writes the XCD's L2 back and the fixing workgroup re-reads
  // the other XCDs' slabs from HBM on a serial dependency chain.
  if (gdim.z > 1) {
    float* pz = part + (int64_t)bid.z * slab;
#pragma unroll
    for (int tm = 0; tm < G::TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < G::TN; ++tn) {
        const int n = (wn * G::TN + tn) * 32 + l32;
        int img, p, q;
        G::pix(n, img, p, q);
        p += prow0;
        float* pb = pz + (int64_t)(b0 + img) * Kout * G::PQ + p * G::Q + q;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + (wm * G::TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          pb[(int64_t)m * G::PQ] = acc[tm][tn][r];
        }
      }
    return;
  }

  // UPS = 2 (grad-x of a 1x1 stride-2 conv): the result lands on the even pixels of a
  // (2P) x (2Q) plane and the three odd neighbours of each are written as zeros
  constexpr int OPQ = G::PQ * UPS * UPS;
  // BatchNorm partial sums (st.out, see ConvBnStats): unsplit, statistics-capable tiles only.
  // The two per-element quantities go through the LDS the main loop no longer reads (its last
  // iteration ended on a barrier) as [BM][BN + 4] tiles: row writes of 32 consecutive pixels
  // per half-wave, float4 row reads in the reduction below.
  constexpr bool kStats = G::STATS_OK && UPS == 1;
  const bool stats = kStats && st.out != nullptr;
  const bool bstats = G::STATS2_OK && stats && st.bx != nullptr;
  float* L = smem;
  float* L2 = smem + BM * G::STATS_LDO;
#pragma unroll
  for (int tm = 0; tm < G::TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < G::TN; ++tn) {
      const int n = (wn * G::TN + tn) * 32 + l32;
      int img, pp, qq;
      G::pix(n, img, pp, qq);
      pp += prow0;
      const int opix = UPS == 1 ? pp * G::Q + qq : pp * UPS * (UPS * G::Q) + qq * UPS;
      const int64_t yoff = (int64_t)(b0 + img) * Kout * OPQ + opix;
      float* yb = y + yoff;
      // addend (UPS == 1 only): y += addend, e.g. the identity-branch gradient of a residual
      // block added into conv1's grad-x (no separate add launch).  All 16 addends are loaded
      // under ONE uniform branch before any store: a per-element `addend ? acc + addend[o]`
      // compiled to 16 serial load + s_waitcnt vmcnt(0) round trips.
      // UPS == 2: the three odd neighbours of each written pixel carry the addend alone
      float ad[16], ad1[UPS == 2 ? 16 : 1], ad2[UPS == 2 ? 16 : 1], ad3[UPS == 2 ? 16 : 1];
      if (addend != nullptr) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + (wm * G::TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          const float* ap = addend + yoff + (int64_t)m * OPQ;
          ad[r] = ap[0];
          if constexpr (UPS == 2) {
            ad1[r] = ap[1];
            ad2[r] = ap[2 * G::Q];
            ad3[r] = ap[2 * G::Q + 1];
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          ad[r] = 0.f;
          if constexpr (UPS == 2) ad1[r] = ad2[r] = ad3[r] = 0.f;
        }
      }
      float bxv[16], byv[16], bmu[16], bis[16];  // backward statistics operands, same rule
      if (kStats && bstats) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + (wm * G::TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          bxv[r] = st.bx[yoff + (int64_t)m * OPQ];
          byv[r] = st.by[yoff + (int64_t)m * OPQ];
          bmu[r] = st.mean[m];
          bis[r] = st.invstd[m];
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int mloc = (wm * G::TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const int m = m0 + mloc;
        float* d = yb + (int64_t)m * OPQ;
        const float v = acc[tm][tn][r] + ad[r];
        d[0] = v;
        if constexpr (UPS == 2) {
          d[1] = ad1[r];
          d[2 * G::Q] = ad2[r];
          d[2 * G::Q + 1] = ad3[r];
        }
        if constexpr (kStats) {
          if (bstats) {
            const float dz = byv[r] > 0.f ? v : 0.f;
            L[mloc * G::STATS_LDO + n] = dz;
            L2[mloc * G::STATS_LDO + n] = dz * ((bxv[r] - bmu[r]) * bis[r]);
          } else if (stats) {
            L[mloc * G::STATS_LDO + n] = v;
          }
        }
      }
    }

  // Per output channel, fp32 over 4 values then fp64, stored to st.out[(c * S + s) * 2 + {0, 1}]
  // with s = blockIdx.x of S = gridDim.x: the [c][s][2] slice-partial layout the BN kernels fold
  // in a fixed order, so the BN runs no statistics pass (one launch and one full read fewer).
  if constexpr (kStats) {
    if (stats) {
      __syncthreads();
      constexpr int TPC = G::STATS_TPC, NPT = G::BN / TPC;
      const int c = tid / TPC, j = tid - c * TPC;
      const float* src = L + c * G::STATS_LDO + j * NPT;
      const float* src2 = L2 + c * G::STATS_LDO + j * NPT;
      double sum = 0.0, sq = 0.0;
#pragma unroll 4
      for (int i = 0; i < NPT; i += 4) {
        const f32x4c v = *reinterpret_cast<const f32x4c*>(src + i);
        sum += (double)((v.x + v.y) + (v.z + v.w));
        if (bstats) {
          const f32x4c u = *reinterpret_cast<const f32x4c*>(src2 + i);
          sq += (double)((u.x + u.y) + (u.z + u.w));
        } else {
          sq += (double)((v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w));
        }
      }
#pragma unroll
      for (int o = 1; o < TPC; o <<= 1) {
        sum += __shfl_xor(sum, o, 64);
        sq += __shfl_xor(sq, o, 64);
      }
      if (j == 0) {
        double* d = st.out + ((int64_t)(m0 + c) * gdim.x + bid.x) * 2;
        d[0] = sum;
        d[1] = sq;
      }
    }
  }
}

template <int R, int S, int ST, int PD, int H, int W, int CK, int BM, int IMGS, int WM, int NBUF, int KB, bool TRANSW,
          bool VEC, int UPS = 1, int SCH = 0, int IUPS = 1, int PSPLIT = 1>
__global__ __launch_bounds__(256) void conv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       float* __restrict__ y, float* __restrict__ part, int Cin,
                                                       int Kout, int cps, int64_t slab,
                                                       const float* __restrict__ addend, ConvBnStats st) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  conv_fwd_body<FwdTile<R, S, ST, PD, H, W, CK, BM, IMGS, WM, NBUF, KB, TRANSW, VEC, UPS, SCH, IUPS, PSPLIT>>(
      x, w, y, part, Cin, Kout, cps, slab, addend, st, make_uint3(blockIdx.x, blockIdx.y, blockIdx.z),
      make_uint3(gridDim.x, gridDim.y, gridDim.z), smem);
}

// ---- grad-W -----------------------------------------------------------------------------
// One grad-W kernel configuration as a type: the parameters of conv_wgrad_body (IPS: images per stage)
template <int R_, int S_, int ST_, int PD_, int H_, int W_, int CB_, int BM_, int NW_, int NBPW_, int KB_, int IPS_ = 1>
struct WgTile {
  static constexpr int R = R_, S = S_, ST = ST_, PD = PD_, H = H_, W = W_, CB = CB_, BM = BM_, NW = NW_, NBPW = NBPW_,
                       KB = KB_, IPS = IPS_;
  template <int N>
  using staged = WgTile<R, S, ST, PD, H, W, CB, BM, NW, NBPW, KB, N>;  // N images per stage
  static constexpr int P = (H + 2 * PD - R) / ST + 1, Q = (W + 2 * PD - S) / ST + 1, PQ = P * Q;
  // odd channel stride + tap-major columns (TAPMAJ: column j = rs * CB + c, so the 32 lanes of
  // a B read are 32 channels at one tap): conflict-free B reads.  Channel-major (c * RS + rs)
  // put 3-4 channels' 3x3 windows in one half-wave: 2-3-way conflicts (PMC round 3), and the
  // even 8x8 1x1 stride was 32-way.
  static constexpr int Hp = H + 2 * PD, Wp = W + 2 * PD, HWp = (Hp * Wp) | 1, HW = H * W;
  static constexpr int RS = R * S, J = CB * RS, JB = (J + 31) / 32, MB = BM / 32;
  static constexpr bool TAPMAJ = CB % 32 == 0;
  __device__ static __forceinline__ void col(int j, int& c, int& rs) {
    if constexpr (TAPMAJ) {
      rs = j / CB;
      c = j - rs * CB;
    } else {
      c = j / RS;
      rs = j - c * RS;
    }
  }
  static constexpr int NSTEP = PQ / 2, NBLK = NSTEP / KB;
  // AVW: the dY row of a lane is read KB pixels at a time (ds_read_b128) — LDY / 4 odd, so
  // the 16 rows of a b128 phase start in disjoint 4-bank groups; else LDY odd for b32 reads
  static constexpr bool AVW = KB % 4 == 0 && (PQ / 2) % 4 == 0;
  static constexpr int LDY = AVW ? PQ + (((PQ / 4) % 2 == 0) ? 4 : 8) : PQ + 1;
  static constexpr int A_SZ = BM * LDY;  // dY tile of one image: [m][pixel]
  static constexpr int B_SZ = CB * HWp;  // zero-bordered x planes of one image
  static constexpr int NT = 64 * NW;
  static constexpr int A4 = BM * PQ / 4, B4 = CB * HW / 4;
  static constexpr int A_PER_T = (A4 + NT - 1) / NT, B_PER_T = (B4 + NT - 1) / NT;
  // TAPMAJ epilogue: the dW tile goes through LDS back to channel-major rows ([BM][J], row
  // stride LDJ, 16-B aligned) so the slab stores stay contiguous float4 (a lane-per-channel
  // store at stride RS scattered every row over RS x 128 B and doubled the write bytes)
  static constexpr int LDJ = J + 4;
  static constexpr size_t MAIN_BYTES = 2 * (size_t)(A_SZ + B_SZ) * sizeof(float);
  static constexpr size_t EPI_BYTES = TAPMAJ ? (size_t)BM * LDJ * sizeof(float) : 0;
  // IPS images per stage (conv_wgrad_body): both stage buffers hold IPS images' tiles
  static constexpr size_t LDS_BYTES = IPS * MAIN_BYTES > EPI_BYTES ? IPS * MAIN_BYTES : EPI_BYTES;
  static_assert(MB * JB == NW * NBPW, "every wave owns NBPW 32x32 blocks");
  static_assert(P % 2 == 0 && PQ % 4 == 0 && HW % 4 == 0 && NSTEP % KB == 0, "pixel pairing / float4 loads");
};

// (a device function of the workgroup's grid coordinates: the layer2 backward pairs run it on
// one part of a combined grid, launch_conv_dgrad)
// IPS = images per stage; only the layer2 3x3 class (4x4 maps) is built with IPS > 1 (wgrad_staged).
// One image of that class is only PQ / 2 = 8 k-steps: as the span between two barriers and the
// whole prefetch distance that is shorter than a trip to HBM, and the waves (one per SIMD) stood
// waiting at every image.  A stage of IPS images
// issues its IPS x (A_PER_T + B_PER_T) float4 loads, runs the MFMAs of the previous stage's images
// in image order, writes its tiles to LDS and meets ONE barrier: IPS times the work per barrier and
// per load round trip, the same MFMAs in the same order on every accumulator (bitwise the one-image
// loop's result).  The slice's image count must be a multiple of IPS: the dispatch (wgrad_staged)
// never gives a slice another IPS, there is no predicated last stage.
template <typename G>  // G: a WgTile
__device__ __forceinline__ void conv_wgrad_body(const float* __restrict__ x, const float* __restrict__ dy,
                                                float* __restrict__ part, int Cin, int Kout, int imgs_per_slice,
                                                const uint3 bid, float* __restrict__ smem) {
  constexpr int S = G::S, ST = G::ST, PD = G::PD, W = G::W, CB = G::CB, BM = G::BM, NBPW = G::NBPW, KB = G::KB,
                IPS = G::IPS;
  float* As = smem;                       // [2][IPS][A_SZ]
  float* Bs = smem + 2 * IPS * G::A_SZ;   // [2][IPS][B_SZ]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l32 = lane & 31;
  const int slice = bid.x, m0 = bid.y * BM, c0 = bid.z * CB;
  const int bb = slice * imgs_per_slice;

  for (int i = tid; i < 2 * IPS * G::B_SZ; i += G::NT) Bs[i] = 0.f;  // every buffer's zero border, once

  int a_base[NBPW], b_base[NBPW];
#pragma unroll
  for (int t = 0; t < NBPW; ++t) {
    const int blk = wave * NBPW + t;
    const int mb = blk / G::JB, jb = blk - mb * G::JB;
    const int j = jb * 32 + l32;
    a_base[t] = (mb * 32 + l32) * G::LDY + h * (G::PQ / 2);
    int c, rs;
    G::col(j, c, rs);
    const int r = rs / S, s = rs - r * S;
    b_base[t] = (j < G::J) ? c * G::HWp + r * G::Wp + s + h * (G::P / 2) * ST * G::Wp : 0;
  }

  // a stage = images [b, b + IPS) in registers, then in LDS buffer `buf` (slots [buf][0 .. IPS))
  f32x4c ra[IPS][G::A_PER_T], rb[IPS][G::B_PER_T];
  auto load = [&](int b) {
#pragma unroll
    for (int ii = 0; ii < IPS; ++ii) {
#pragma unroll
      for (int i = 0; i < G::A_PER_T; ++i) {
        const int e = tid + G::NT * i;
        f32x4c v = {0.f, 0.f, 0.f, 0.f};
        if (e < G::A4) v = *reinterpret_cast<const f32x4c*>(dy + ((int64_t)(b + ii) * Kout + m0) * G::PQ + 4 * e);
        ra[ii][i] = v;
      }
#pragma unroll
      for (int i = 0; i < G::B_PER_T; ++i) {
        const int e = tid + G::NT * i;
        f32x4c v = {0.f, 0.f, 0.f, 0.f};
        if (e < G::B4 && c0 + (4 * e) / G::HW < Cin)
          v = *reinterpret_cast<const f32x4c*>(x + ((int64_t)(b + ii) * Cin + c0) * G::HW + 4 * e);
        rb[ii][i] = v;
      }
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int ii = 0; ii < IPS; ++ii) {
      float* A = As + (buf * IPS + ii) * G::A_SZ;
      float* B = Bs + (buf * IPS + ii) * G::B_SZ;
#pragma unroll
      for (int i = 0; i < G::A_PER_T; ++i) {
        const int e = tid + G::NT * i;
        if (e < G::A4) {
          const int m = (4 * e) / G::PQ, pq = 4 * e - m * G::PQ;
          float* d = A + m * G::LDY + pq;
          if constexpr (G::AVW) {
            *reinterpret_cast<f32x4c*>(d) = ra[ii][i];
          } else {
            d[0] = ra[ii][i].x; d[1] = ra[ii][i].y; d[2] = ra[ii][i].z; d[3] = ra[ii][i].w;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < G::B_PER_T; ++i) {
        const int e = tid + G::NT * i;
        if (e < G::B4) {
          const int c = (4 * e) / G::HW, hw = 4 * e - c * G::HW;
          const int hh = hw / W, ww = hw - hh * W;
          float* d = B + c * G::HWp + (hh + PD) * G::Wp + ww + PD;
          d[0] = rb[ii][i].x; d[1] = rb[ii][i].y; d[2] = rb[ii][i].z; d[3] = rb[ii][i].w;
        }
      }
    }
  };

  f32x16 acc[NBPW];
#pragma unroll
  for (int t = 0; t < NBPW; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  load(bb);
  __syncthreads();
  store(0);
  __syncthreads();
  const int stages = imgs_per_slice / IPS;
  for (int i = 0; i < stages; ++i) {
    const int cur = i & 1;
    if (i + 1 < stages) load(bb + (i + 1) * IPS);
#pragma unroll
    for (int ii = 0; ii < IPS; ++ii) {
      const float* A = As + (cur * IPS + ii) * G::A_SZ;
      const float* B = Bs + (cur * IPS + ii) * G::B_SZ;
      float av[2][KB][NBPW], bv[2][KB][NBPW];
      auto fetch = [&](int blk, int slot) {
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          const int t = blk * KB + k;
          const int p = t / G::Q, q = t - p * G::Q;
#pragma unroll
          for (int u = 0; u < NBPW; ++u) {
            if constexpr (!G::AVW) av[slot][k][u] = A[a_base[u] + t];
            bv[slot][k][u] = B[b_base[u] + p * ST * G::Wp + q * ST];
          }
        }
        if constexpr (G::AVW) {
#pragma unroll
          for (int u = 0; u < NBPW; ++u)
#pragma unroll
            for (int q4 = 0; q4 < KB / 4; ++q4) {
              const f32x4c v = *reinterpret_cast<const f32x4c*>(A + a_base[u] + blk * KB + 4 * q4);
#pragma unroll
              for (int j = 0; j < 4; ++j) av[slot][4 * q4 + j][u] = v[j];
            }
        }
      };
      fetch(0, 0);
#pragma unroll
      for (int blk = 0; blk < G::NBLK; ++blk) {
        if (blk + 1 < G::NBLK) fetch(blk + 1, (blk + 1) & 1);
#pragma unroll
        for (int k = 0; k < KB; ++k)
#pragma unroll
          for (int u = 0; u < NBPW; ++u) acc[u] = mfma32(av[blk & 1][k][u], bv[blk & 1][k][u], acc[u]);
      }
    }
    if (i + 1 < stages) store(cur ^ 1);
    __syncthreads();
  }

  float* out = part + (int64_t)slice * Kout * Cin * G::RS;
  if constexpr (G::TAPMAJ && G::RS > 1) {
    // the loop's last barrier retired every LDS read: reuse the buffers as the staging tile
    float* st = smem;
#pragma unroll
    for (int t = 0; t < NBPW; ++t) {
      const int blk = wave * NBPW + t;
      const int mb = blk / G::JB, jb = blk - mb * G::JB;
      const int j = jb * 32 + l32;
      int c, rs;
      G::col(j, c, rs);
      if (j < G::J) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          st[(mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * G::LDJ + c * G::RS + rs] = acc[t][r];
      }
    }
    __syncthreads();
    const int lim = min(CB, Cin - c0) * G::RS;  // valid columns of a row (partial channel block)
    constexpr int J4 = G::J / 4;
    static_assert(G::J % 4 == 0, "float4 rows");
    for (int i = tid; i < BM * J4; i += G::NT) {
      const int mr = i / J4, q = 4 * (i - mr * J4);
      const f32x4c v = *reinterpret_cast<const f32x4c*>(st + mr * G::LDJ + q);
      float* o = out + ((int64_t)(m0 + mr) * Cin + c0) * G::RS + q;
      if (q + 3 < lim) {
        *reinterpret_cast<f32x4c*>(o) = v;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (q + k < lim) o[k] = v[k];
      }
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < NBPW; ++t) {
    const int blk = wave * NBPW + t;
    const int mb = blk / G::JB, jb = blk - mb * G::JB;
    const int j = jb * 32 + l32;
    int c, rs;
    G::col(j, c, rs);
    if (j < G::J && c0 + c < Cin) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        out[((int64_t)m * Cin + c0 + c) * G::RS + rs] = acc[t][r];
      }
    }
  }
}

template <int R, int S, int ST, int PD, int H, int W, int CB, int BM, int NW, int NBPW, int KB, int IPS = 1>
__global__ __launch_bounds__(64 * NW) void conv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             float* __restrict__ part, int Cin, int Kout,
                                                             int imgs_per_slice) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  conv_wgrad_body<WgTile<R, S, ST, PD, H, W, CB, BM, NW, NBPW, KB, IPS>>(
      x, dy, part, Cin, Kout, imgs_per_slice, make_uint3(blockIdx.x, blockIdx.y, blockIdx.z), smem);
}

// A layer2 backward pair in ONE launch: workgroups [0, n_dgrad) run the Winograd grad-x
// (wino_dpp.h; 4x4 maps, or the 3x3/2 conv's zero-inserted 8x8 dY), the rest the direct grad-W of
// the same conv (64 NW threads: the surplus wave leaves before any barrier, which then waits for
// the live waves only).  Both read only dY / x / the weights and write disjoint outputs.
template <int WH, int IUPS, int R, int S, int ST, int PD, int H, int W, int CB, int BM, int NW, int NBPW, int KB,
          int IPS = 1>
__global__ __launch_bounds__(256, 2) void wino_direct_pair_kernel(WinoConvArgs A, uint3 ga, const float* __restrict__ x,
                                                                  const float* __restrict__ dy, float* __restrict__ part,
                                                                  int Cin, int Kout, int imgs, uint3 gw) {
  static_assert(NW <= 4, "grad-W workgroup within the pair's 256 threads");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const unsigned na = ga.x * ga.y * ga.z;
  unsigned b = blockIdx.x;
  if (b < na) {
    wino_dpp_body<WH, IUPS>(A, make_uint3(b % ga.x, (b / ga.x) % ga.y, b / (ga.x * ga.y)), ga, smem);
  } else {
    if (threadIdx.x >= 64 * NW) return;
    b -= na;
    conv_wgrad_body<WgTile<R, S, ST, PD, H, W, CB, BM, NW, NBPW, KB, IPS>>(
        x, dy, part, Cin, Kout, imgs, make_uint3(b % gw.x, (b / gw.x) % gw.y, b / (gw.x * gw.y)), smem);
  }
}

// dw[i] = sum_{s < n_slices} part[s * n + i], n % 4 == 0.  A workgroup owns 16 float4
// columns x 16 slice groups: thread (g, col) sums slices g, g+16, ... of its column, then
// group 0 adds the 16 group sums in order — a fixed summation tree (deterministic) with
// 16x the memory-level parallelism of a one-thread-per-column sum.
__global__ __launch_bounds__(256) void conv_slab_sum_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                            int64_t n, int n_slices,
                                                            const float* __restrict__ addend = nullptr) {
  __shared__ f32x4c red[16][16];
  const int col = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int64_t i4 = ((int64_t)blockIdx.x * 16 + col) * 4;
  f32x4c acc = {0.f, 0.f, 0.f, 0.f};
  if (i4 < n) {
#pragma unroll 4
    for (int s = g; s < n_slices; s += 16) acc += *reinterpret_cast<const f32x4c*>(part + (int64_t)s * n + i4);
  }
  red[g][col] = acc;
  __syncthreads();
  if (g == 0 && i4 < n) {
    f32x4c t = red[0][col];
#pragma unroll
    for (int k = 1; k < 16; ++k) t += red[k][col];
    if (addend) t += *reinterpret_cast<const f32x4c*>(addend + i4);  // fused residual-branch gradient
    *reinterpret_cast<f32x4c*>(dw + i4) = t;
  }
}

// Every deferred grad-W slab sum of a backward pass in ONE launch (ops/gradfinish.py):
// entry e owns blocks [end[e-1], end[e]); inside an entry the same 16-group fixed-order
// tree as conv_slab_sum_kernel (bitwise identical results).
__device__ __forceinline__ void slab_sum_many_block(const SlabBatch& b, int64_t blk, f32x4c (*red)[16]) {
  int e = 0;
  while (e + 1 < b.n && blk >= b.end[e]) ++e;
  const int64_t lb = blk - (e ? b.end[e - 1] : 0);
  const float* part = b.part[e];
  const int64_t n = b.numel[e];
  const int n_slices = b.slices[e];
  const int col = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int64_t i4 = (lb * 16 + col) * 4;
  f32x4c acc = {0.f, 0.f, 0.f, 0.f};
  if (i4 < n) {
#pragma unroll 4
    for (int sl = g; sl < n_slices; sl += 16) {
      if (b.nt) acc += __builtin_nontemporal_load(reinterpret_cast<const f32x4c*>(part + (int64_t)sl * n + i4));
      else acc += *reinterpret_cast<const f32x4c*>(part + (int64_t)sl * n + i4);
    }
  }
  red[g][col] = acc;
  __syncthreads();
  if (g == 0 && i4 < n) {
    f32x4c t = red[0][col];
#pragma unroll
    for (int k = 1; k < 16; ++k) t += red[k][col];
    *reinterpret_cast<f32x4c*>(b.dw[e] + i4) = t;
  }
}

__global__ __launch_bounds__(256) void conv_slab_sum_many_kernel(SlabBatch b) {
  __shared__ f32x4c red[16][16];
  slab_sum_many_block(b, blockIdx.x, red);
}

// The end-of-backward grad-W finish in ONE launch: blocks [0, slab blocks) run the slab sums,
// the rest the Toeplitz folds (the two lists touch disjoint gradients).  Same per-block
// bodies as the two kernels above, so the results are bitwise identical to them.
__global__ __launch_bounds__(256) void gradw_finish_kernel(SlabBatch sb, FoldBatch fb) {
  constexpr int kFloats = 256 * kFoldMaxTaps > 16 * 16 * 4 ? 256 * kFoldMaxTaps : 16 * 16 * 4;
  __shared__ __attribute__((aligned(16))) float smem[kFloats];
  const int64_t n_slab = sb.n > 0 ? sb.end[sb.n - 1] : 0;
  const int64_t blk = blockIdx.x;
  if (blk < n_slab) slab_sum_many_block(sb, blk, reinterpret_cast<f32x4c (*)[16]>(smem));
  else fold_many_block(fb, blk - n_slab, smem);
}

void launch_gradw_finish(const SlabBatch& sb, const FoldBatch& fb, hipStream_t s) {
  if (sb.n <= 0) return launch_toeplitz_fold_many(fb, s);
  if (fb.n <= 0) return launch_slab_sum_many(sb, s);
  const_cast<SlabBatch&>(sb).nt = 1;
  const int64_t blocks = sb.end[sb.n - 1] + (fb.end[fb.n - 1] + 255) / 256;
  hipLaunchKernelGGL(gradw_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, s, sb, fb);
}

void launch_slab_sum_many(const SlabBatch& b, hipStream_t s) {
  const_cast<SlabBatch&>(b).nt = 1;  // slabs are read once: non-temporal loads (with the Q pass's, b64 -2.5 %)
  if (b.n <= 0) return;
  hipLaunchKernelGGL(conv_slab_sum_many_kernel, dim3((unsigned)b.end[b.n - 1]), dim3(256), 0, s, b);
}

// split-K sum for the stride-2 1x1 grad-x: dx[b, c, 2p + i, 2q + j] = (i == j == 0) ?
// sum_z part[z][b][c][p][q] : 0 (+ addend[b, c, 2p + i, 2q + j]); one thread per float4 of dx
// (a (2P) x (2Q) plane, 2Q / 4 float4 per row; compact P x Q pixels per partial plane)
template <int P, int Q>
__global__ __launch_bounds__(256) void conv_slab_sum_ups_kernel(const float* __restrict__ part, float* __restrict__ dx,
                                                                int64_t slab, int n_slices,
                                                                const float* __restrict__ addend) {
  constexpr int F4R = (2 * Q) / 4, F4P = 2 * P * F4R;
  static_assert((2 * Q) % 4 == 0, "float4 rows");
  const int64_t i4 = (int64_t)blockIdx.x * 256 + threadIdx.x;  // float4 index into dx
  if (i4 * 4 >= slab * 4) return;                              // dx has 4x the compact elements
  const int64_t plane = i4 / F4P;
  const int r4 = (int)(i4 - plane * F4P);
  const int row = r4 / F4R, half = r4 - row * F4R;
  f32x4c v = {0.f, 0.f, 0.f, 0.f};
  if (addend != nullptr) v = *reinterpret_cast<const f32x4c*>(addend + i4 * 4);
  if ((row & 1) == 0) {
    const int p = row >> 1, q0 = half * 2;                    // this float4 covers q = q0, q0 + 1
    const float* src = part + plane * (P * Q) + p * Q + q0;
    float a = 0.f, b = 0.f;
    for (int z = 0; z < n_slices; ++z) {
      a += src[z * slab];
      b += src[z * slab + 1];
    }
    v.x += a;
    v.z += b;
  }
  *reinterpret_cast<f32x4c*>(dx + i4 * 4) = v;
}

// ---- shape classes --------------------------------------------------------------------------
// Images per stage of the direct grad-W (conv_wgrad_body IPS): kWgIps for the layer2 3x3 class
// (kConv3x3Map4: 4 images = 57 KB of tiles, two workgroups per CU as before, 8 float4 of staging
// registers) when the slice holds at least two such stages, else the one-image loop — so per-GPU
// batch 64 (4-image slices) runs what it ran.  NDP_FUSION_OFF=wgrad_pipe (A/B arm) and
// conv_set_wgrad_stage(1) give the one-image loop everywhere; conv_set_wgrad_stage(0) = auto.
// Measured and not built (profiles/r7/README.md): 2 images per stage, and stages for the 3x3/2 and
// 1x1/2 classes.  conv_set_wgrad_stage accepts 0, 1 and kWgIps only (the binding rejects the rest).
constexpr int kWgIps = 4;

// Shape classes with a direct kernel (ConvClass, ndp_kernels.h, lists the shapes; everything else stays
// on MIOpen / the Toeplitz path).  Each class names its forward, grad-x and grad-W tiles once, here;
// conv_direct_class detects it, class_info reads the tiles for the host-side plan.
// MFMA-block schedule of the layer1 / layer2 fwd + grad-x kernels: SCH = 2 (pinned MFMA /
// LDS-read interleave): ResNet-18 step on 1x MI355X 2.0175 / 2.0154 -> 1.9981 / 1.9994 ms at
// batch 512, 1.0582 / 1.0627 -> 1.0546 / 1.0569 at batch 64 against the compiler's schedule
// (iglp_opt(0): 2.0043 / 1.0602; the pinned interleave on the stem / 3x3-2 / 1x1-2 forwards
// and 16-channel chunks or two-image layer1 tiles were slower — round 3 A/Bs)
using Fwd3x3Map8 = FwdTile<3, 3, 1, 1, 8, 8, 8, 64, 1, 2, 2, 4, false, true, 1, 2>;
using Dgrad3x3Map8 = Fwd3x3Map8::transposed;
using Wgrad3x3Map8 = WgTile<3, 3, 1, 1, 8, 8, 32, 32, 3, 3, 4>;
using Fwd3x3Map4 = FwdTile<3, 3, 1, 1, 4, 4, 8, 64, 4, 2, 2, 4, false, true, 1, 2>;
using Dgrad3x3Map4 = Fwd3x3Map4::transposed;
using Wgrad3x3Map4 = WgTile<3, 3, 1, 1, 4, 4, 32, 32, 3, 3, 4>;
using Wgrad3x3Map4Staged = Wgrad3x3Map4::staged<kWgIps>;
using Fwd3x3S2 = FwdTile<3, 3, 2, 1, 8, 8, 8, 64, 4, 2, 2, 4, false, true>;
using Dgrad3x3S2 = Dgrad3x3Map8::iups<2>;  // the layer1 grad-x kernel on the zero-inserted dY (staged, not stored)
using Wgrad3x3S2 = WgTile<3, 3, 2, 1, 8, 8, 32, 32, 3, 3, 4>;
using FwdStem = FwdTile<7, 7, 2, 3, 32, 32, 4, 64, 1, 2, 1, 7, false, false>;
using FwdStem2 = FwdStem::psplit<2>;
using FwdStem4 = FwdStem::psplit<4>;
struct NoTile { static constexpr int IMGS = 0, UPS = 1, IUPS = 1, PQ = 0; };  // the stem has no grad-x kernel
using WgradStem = WgTile<7, 7, 2, 3, 32, 32, 3, 32, 5, 1, 4>;
// grad-x of a 1x1 stride-2 conv: the transposed 1x1 product on the DH x DW output map, written to the
// even pixels of the (2 DH) x (2 DW) plane (UPS = 2 epilogue, odd pixels zero)
// (These six tiles describe the two 1x1 stride-2 classes to the plan — class_info reads their images per
// workgroup — and run only where the streamed bodies of ds_stream.h do not: NDP_FUSION_OFF=ds_stream and
// the 8x8 forward.)
template <int DH, int DW, int DBM, int DIMGS>
using DsDgradTile = FwdTile<1, 1, 1, 0, DH, DW, 8, DBM, DIMGS, 2, 2, 4, true, true, 2>;
using Fwd1x1S2Map8 = FwdTile<1, 1, 2, 0, 8, 8, 8, 64, 4, 2, 2, 4, false, true>;
using Dgrad1x1S2Map8 = DsDgradTile<4, 4, 64, 4>;
using Wgrad1x1S2Map8 = WgTile<1, 1, 2, 0, 8, 8, 32, 32, 1, 1, 4>;
// the kConv1x1S2Map8 scheme one map size down, 16 images per tile; the Toeplitz GEMM it replaces multiplied 15
// zero rows of W_big per useful one (profiles/r5/toeplitz_layers_b512.md: 72.8 us fwd + bwd at batch 512)
using Fwd1x1S2Map4 = FwdTile<1, 1, 2, 0, 4, 4, 8, 64, 16, 2, 2, 4, false, true>;
using Dgrad1x1S2Map4 = DsDgradTile<2, 2, 64, 16>;
using Wgrad1x1S2Map4 = WgTile<1, 1, 2, 0, 4, 4, 32, 32, 1, 1, 2>;

// A downsample conv's backward pair (the 1x1 stride-2 classes) in ONE launch: workgroups
// [0, n_dgrad) run the direct grad-x (conv_fwd_body on the transposed weights, UPS = 2 epilogue),
// the rest the direct grad-W (64 NW threads; the surplus waves leave before any barrier).
struct DirectDgradArgs {
  const float *dy, *w;
  float *dx, *part;
  int Cin, Kout, cps;
  int64_t slab;
  const float* addend;
  DsArgs ds;     // STREAM: the arguments of ds_stream_body
  DsWgArgs dsw;  //         and of ds_wgrad_body
};
// STREAM: both halves are the streamed bodies of ds_stream.h (no LDS, every wave on its own) instead of
// conv_fwd_body / conv_wgrad_body
template <bool STREAM, int DH, int DW, int DBM, int DIMGS, int R, int S, int ST, int PD, int H, int W, int CB, int BM,
          int NW, int NBPW, int KB>
__global__ __launch_bounds__(256) void direct_pair_kernel(DirectDgradArgs A, uint3 ga, const float* __restrict__ x,
                                                          const float* __restrict__ dy, float* __restrict__ part,
                                                          int Cin, int Kout, int imgs, uint3 gw) {
  static_assert(NW <= 4, "grad-W workgroup within the pair's 256 threads");
  const unsigned na = ga.x * ga.y * ga.z;
  unsigned b = blockIdx.x;
  if constexpr (STREAM) {
    if (b < na) ds_stream_body<2 * DH, true>(A.ds, make_uint3(b % ga.x, 0, b / ga.x), ga);
    else ds_wgrad_body<H>(A.dsw, make_uint3(b - na, 0, 0));
  } else {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (b < na) {
      conv_fwd_body<DsDgradTile<DH, DW, DBM, DIMGS>>(A.dy, A.w, A.dx, A.part, A.Cin, A.Kout, A.cps, A.slab, A.addend,
                                                     ConvBnStats{},
                                                     make_uint3(b % ga.x, (b / ga.x) % ga.y, b / (ga.x * ga.y)), ga, smem);
    } else {
      if (threadIdx.x >= 64 * NW) return;
      b -= na;
      conv_wgrad_body<WgTile<R, S, ST, PD, H, W, CB, BM, NW, NBPW, KB>>(
          x, dy, part, Cin, Kout, imgs, make_uint3(b % gw.x, (b / gw.x) % gw.y, b / (gw.x * gw.y)), smem);
    }
  }
}

// The streamed 1x1 stride-2 grad-W on its own
template <int MAP>
__global__ __launch_bounds__(256) void ds_wgrad_kernel(DsWgArgs A) {
  ds_wgrad_body<MAP>(A, make_uint3(blockIdx.x, 0, 0));
}

// ---- the downsample block's two forward convs in ONE launch --------------------------------
// conv1 (3x3 stride 2, kConv3x3S2) and the 1x1 stride-2 downsample (kConv1x1S2Map8) read the same
// block input; the downsample's launch is held back (launch_conv_fwd pair = true) and conv1's launch
// runs both bodies on one grid: conv1's workgroups first (its output feeds bn1 right after).
struct FwdPart {
  const float *x, *w;
  float *y, *part;
  int Cin, Kout, cps;
  int64_t slab;
};
__global__ __launch_bounds__(256) void ds_fwd_pair_kernel(FwdPart a, uint3 ga, FwdPart b, uint3 gb) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const unsigned na = ga.x * ga.y * ga.z;
  unsigned k = blockIdx.x;
  if (k < na) {
    conv_fwd_body<Fwd3x3S2>(a.x, a.w, a.y, a.part, a.Cin, a.Kout, a.cps, a.slab, nullptr, ConvBnStats{},
                                   make_uint3(k % ga.x, (k / ga.x) % ga.y, k / (ga.x * ga.y)), ga, smem);
  } else {
    k -= na;
    conv_fwd_body<Fwd1x1S2Map8>(b.x, b.w, b.y, b.part, b.Cin, b.Kout, b.cps, b.slab, nullptr, ConvBnStats{},
                                       make_uint3(k % gb.x, (k / gb.x) % gb.y, k / (gb.x * gb.y)), gb, smem);
  }
}

// The streamed 1x1 stride-2 forward (DGRAD false) / grad-x (true) on its own
template <int MAP, bool DGRAD>
__global__ __launch_bounds__(256) void ds_stream_kernel(DsArgs A) {
  ds_stream_body<MAP, DGRAD>(A, make_uint3(blockIdx.x, 0, blockIdx.z), make_uint3(gridDim.x, 1, gridDim.z));
}

// ---- launch helpers -------------------------------------------------------------------------
template <typename KernelT>
static void set_lds(KernelT k, size_t bytes) {
  // (result discarded: without the opt-in the launch that follows fails, the error every caller reads)
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

void launch_slab_sum(const float* part, float* out, int64_t n, int nslab, hipStream_t s, const float* addend) {
  hipLaunchKernelGGL(conv_slab_sum_kernel, dim3((unsigned)((n / 4 + 15) / 16)), dim3(256), 0, s, part, out, n, nslab,
                     addend);
}
// the split-K sum of a UPS = 2 grad-x tile T (slab: compact floats per partial; dx holds 4x as many)
template <typename T>
static void launch_slab_sum_ups(const float* part, float* dx, int64_t slab, int nslab, hipStream_t s,
                                const float* addend) {
  hipLaunchKernelGGL((conv_slab_sum_ups_kernel<T::P, T::Q>), dim3((unsigned)((slab + 255) / 256)), dim3(256),
                     0, s, part, dx, slab, nslab, addend);
}

// One forward / grad-x launch: y[B, Kout, ...] from x[B, Cin, ...] (grad-x: x = dY, y = dX)
struct FwdArgs {
  const float *x, *w;
  float* y;
  int B, Cin, Kout, ksplit;
  float* part;
  hipStream_t s;
  const float* addend;
  bool defer;
  ConvBnStats stats;
};
// Tile T's kernel arguments and grid for `a`; grid.z = the split-K factor as every launch normalises it (no
// split without scratch, no empty split).  ksplit > 1: the ksplit workgroups of an output tile each reduce
// 1/ksplit of the input channels (cps chunks of CK) into their own slab of `part`; conv_slab_sum(_ups) adds
// the slabs in split order (deterministic).  Used where B / IMGS * Kout / BM alone cannot fill the 256 CUs
// (small per-GPU batches: the strong-scaling shapes 512 / N).
template <typename T>
static FwdPart fwd_part(const FwdArgs& a, uint3& grid) {
  const int nchunks = (a.Cin + T::CK - 1) / T::CK;
  const int ksplit = (a.ksplit < 1 || a.part == nullptr) ? 1 : a.ksplit;
  const int cps = (nchunks + ksplit - 1) / ksplit;
  grid = make_uint3((unsigned)(a.B / T::IMGS * T::PSPLIT), (unsigned)(a.Kout / T::BM), (unsigned)((nchunks + cps - 1) / cps));
  return FwdPart{a.x, a.w, a.y, a.part, a.Cin, a.Kout, cps, (int64_t)a.B * a.Kout * T::PQ};  // compact partial tiles
}
// take a held-back launch out of its slot
template <typename P>
static P take(P& slot) { return std::exchange(slot, P{}); }

// ---- the streamed 1x1 stride-2 bodies (ds_stream.h) ----
// On unless NDP_FUSION_OFF=ds_stream (A/B arm) or conv_set_ds_stream(0): off runs conv_fwd_body on the
// Fwd1x1S2* / DsDgradTile tiles, which stay for that arm (and for the plan's ClassInfo) only.
static int g_ds_stream = -1;  // -1: by the switch
void conv_set_ds_stream(int on) { g_ds_stream = on < 0 ? -1 : (on ? 1 : 0); }
static bool ds_stream_on() {
  static const bool env_off = [] {
    const char* e = getenv("NDP_FUSION_OFF");
    const std::string s = std::string(",") + (e ? e : "") + ",";
    return s.find(",ds_stream,") != std::string::npos || s.find(",all,") != std::string::npos;
  }();
  return g_ds_stream < 0 ? !env_off : g_ds_stream == 1;
}
// FwdTile T -> the streamed body that replaces it (MAP 0: none).  Not the 8x8 forward: in the
// flagship it runs inside ds_fwd_pair_kernel, whose time is conv1's and did not move with a streamed
// 1x1 half (profiles/r11/README.md).
template <typename T>
struct DsOf {
  static constexpr bool DGRAD = T::UPS == 2;
  static constexpr int MAP = (T::R == 1 && T::S == 1 && T::PD == 0 && T::CK == 8 && (DGRAD ? T::ST == 1 : T::ST == 2) &&
                              (DGRAD || T::H == 4))
                                 ? (DGRAD ? 2 * T::H : T::H)
                                 : 0;
};
static_assert(DsOf<Fwd1x1S2Map8>::MAP == 0 && DsOf<Dgrad1x1S2Map8>::MAP == 8 && DsOf<Fwd1x1S2Map4>::MAP == 4 &&
                  DsOf<Dgrad1x1S2Map4>::MAP == 4 && DsOf<Fwd3x3S2>::MAP == 0 && DsOf<Dgrad3x3Map4>::MAP == 0,
              "the 1x1 stride-2 tiles but the 8x8 forward, and no other");
// live waves per workgroup of the streamed bodies for `tiles` independent wave tiles: as few as
// still give every CU a workgroup (a wave alone on its SIMD keeps its MFMA chain and its loads
// to itself; the pair kernels launch 256 threads, the surplus waves leave at once)
static int ds_wpw(int64_t tiles) { return tiles >= 4 * 256 ? 4 : tiles >= 2 * 256 ? 2 : 1; }
// Arguments and grid of the streamed body for launch `a`, with the split-K normalisation of fwd_part
// (the same grid z, channel ranges and slabs: the plan's ksplit decides, the consumers do not change).
// The grid's x is this launcher's: the 32-pixel x 32-channel wave tiles, ds_wpw of them per
// workgroup.  false: switched off.
template <int MAP, bool DGRAD>
static bool ds_part(const FwdArgs& a, DsArgs& d, uint3& grid) {
  using G = DsGeom<MAP>;
  if (!ds_stream_on() || a.Cin % 8 != 0 || a.Kout % 32 != 0) return false;
  const int nchunks = a.Cin / 8;
  const int ksplit = (a.ksplit < 1 || a.part == nullptr) ? 1 : a.ksplit;
  const int cps = (nchunks + ksplit - 1) / ksplit;
  if (nchunks % cps != 0) return false;
  const int gz = nchunks / cps;
  const int tiles = (int)(((int64_t)a.B * G::PQ + 31) / 32) * (a.Kout / 32);
  const int wpw = ds_wpw((int64_t)tiles * gz);
  d = DsArgs{a.x, a.w, a.y, a.part, gz > 1 ? nullptr : a.addend, a.Cin, a.Kout, a.B, cps * 8, wpw, tiles,
             (int64_t)a.B * a.Kout * G::PQ};
  grid = make_uint3((unsigned)((tiles + wpw - 1) / wpw), 1u, (unsigned)gz);
  return true;
}
// run_fwd on the streamed body: the same slab sums and return value
template <typename T>
static bool run_ds(const FwdArgs& a, int& ret) {
  constexpr int MAP = DsOf<T>::MAP;
  constexpr bool DGRAD = DsOf<T>::DGRAD;
  DsArgs d;
  uint3 grid;
  if (!ds_part<MAP, DGRAD>(a, d, grid)) return false;
  hipLaunchKernelGGL((ds_stream_kernel<MAP, DGRAD>), dim3(grid.x, 1, grid.z), dim3(256), 0, a.s, d);
  const int ksplit = (int)grid.z;
  ret = 1;
  if (ksplit > 1 && a.defer && !DGRAD) {
    ret = ksplit;
  } else if (ksplit > 1) {
    if constexpr (!DGRAD) launch_slab_sum(a.part, a.y, d.slab, ksplit, a.s, a.addend);
    else launch_slab_sum_ups<T>(a.part, a.y, d.slab, ksplit, a.s, a.addend);
  }
  return true;
}

template <typename T>
static int run_fwd(const FwdArgs& a) {
  if constexpr (DsOf<T>::MAP != 0) {
    int ret;
    if (run_ds<T>(a, ret)) return ret;
  }
  auto k = conv_fwd_kernel<T::R, T::S, T::ST, T::PD, T::H, T::W, T::CK, T::BM, T::IMGS, T::WM, T::NBUF, T::KB,
                           T::TRANSW, T::VEC, T::UPS, T::SCH, T::IUPS, T::PSPLIT>;
  static bool attr = false;  // once per instantiation (> 64 KiB of LDS needs the opt-in)
  if (!attr) { set_lds(k, T::LDS_BYTES); attr = true; }
  uint3 grid;
  const FwdPart f = fwd_part<T>(a, grid);
  const int ksplit = (int)grid.z;
  // stats: only unsplit launches of statistics-capable tiles (ConvPlan::fwd_stats_slices says which)
  ConvBnStats stats = a.stats;
  if (!(T::STATS_OK && T::UPS == 1) || ksplit > 1 || (stats.bx != nullptr && !T::STATS2_OK)) stats.out = nullptr;
  hipLaunchKernelGGL(k, dim3(grid.x, grid.y, grid.z), dim3(256), T::LDS_BYTES, a.s, f.x, f.w, f.y, f.part, f.Cin, f.Kout,
                     f.cps, f.slab, ksplit > 1 ? nullptr : a.addend, stats);
  // defer: leave the ksplit slabs for the consumer (the fused BN kernel sums them while it
  // reads its input, ops/slablink.py) — one launch fewer per conv
  // (an addend then goes to the consumer too: it adds it after the slabs, launch_bn_bwd dyadd)
  if (ksplit > 1 && a.defer && T::UPS == 1) return ksplit;
  if (ksplit > 1) {
    if constexpr (T::UPS == 1) launch_slab_sum(a.part, a.y, f.slab, ksplit, a.s, a.addend);
    else launch_slab_sum_ups<T>(a.part, a.y, f.slab, ksplit, a.s, a.addend);
  }
  return 1;
}

static int g_wgrad_stage = 0;
bool conv_set_wgrad_stage(int n) {
  if (n != 0 && n != 1 && n != kWgIps) return false;
  g_wgrad_stage = n;
  return true;
}
// pair launches made so far (a conv's grad-x and its held-back grad-W in one launch): lets a test
// tell a pair from the two launches it replaces
static int64_t g_pair_launches = 0;
int64_t conv_pair_launches() { return g_pair_launches; }
static bool wgrad_staged(int imgs) {
  const bool on = g_wgrad_stage ? g_wgrad_stage == kWgIps : !wgrad_pipe_off();
  return on && imgs % kWgIps == 0 && imgs >= 2 * kWgIps;
}

// One direct grad-W launch: slices of `imgs` images into `part`, summed into dw unless dw == nullptr
// (partials only: the caller sums the slabs, batched, ops/gradfinish.py)
struct WgArgs {
  const float *x, *dy;
  float *part, *dw;
  int B, Cin, Kout, imgs;
  hipStream_t s;
};
// its grid for tile T: (batch slices, output-channel tiles, input-channel blocks)
template <typename T>
static uint3 wgrad_grid(const WgArgs& a) {
  return make_uint3((unsigned)(a.B / a.imgs), (unsigned)(a.Kout / T::BM), (unsigned)((a.Cin + T::CB - 1) / T::CB));
}
// Arguments and grid of the streamed 1x1 stride-2 grad-W (ds_wgrad_body) for launch `a`: one wave tile per
// slice and 32 x 32 block, ds_wpw of them per workgroup; the slices and the slab layout are the plan's.
// false: switched off.
static bool ds_wg_part(const WgArgs& a, DsWgArgs& d, uint3& grid) {
  if (!ds_stream_on() || a.Cin % 32 != 0 || a.Kout % 32 != 0) return false;
  const int tiles = (a.B / a.imgs) * (a.Kout / 32) * (a.Cin / 32);
  const int wpw = ds_wpw(tiles);
  d = DsWgArgs{a.x, a.dy, a.part, a.Cin, a.Kout, a.imgs, wpw, tiles};
  grid = make_uint3((unsigned)((tiles + wpw - 1) / wpw), 1u, 1u);
  return true;
}
template <int MAP>
static bool run_ds_wgrad(const WgArgs& a) {
  DsWgArgs d;
  uint3 g;
  if (!ds_wg_part(a, d, g)) return false;
  hipLaunchKernelGGL((ds_wgrad_kernel<MAP>), dim3(g.x), dim3(256), 0, a.s, d);
  if (a.dw != nullptr) launch_slab_sum(a.part, a.dw, (int64_t)a.Kout * a.Cin, a.B / a.imgs, a.s);
  return true;
}

template <typename T>
static void run_wgrad(const WgArgs& a) {
  if constexpr (T::R == 1 && T::S == 1 && T::ST == 2 && T::PD == 0) {
    if (run_ds_wgrad<T::H>(a)) return;
  }
  auto k = conv_wgrad_kernel<T::R, T::S, T::ST, T::PD, T::H, T::W, T::CB, T::BM, T::NW, T::NBPW, T::KB, T::IPS>;
  static bool attr = false;
  if (!attr) { set_lds(k, T::LDS_BYTES); attr = true; }
  const uint3 gw = wgrad_grid<T>(a);
  hipLaunchKernelGGL(k, dim3(gw.x, gw.y, gw.z), dim3(T::NT), T::LDS_BYTES, a.s, a.x, a.dy, a.part, a.Cin, a.Kout,
                     a.imgs);
  // (Kout * Cin * RS: a multiple of 4 for every class)
  if (a.dw != nullptr) launch_slab_sum(a.part, a.dw, (int64_t)a.Kout * a.Cin * T::RS, (int)gw.x, a.s);
}
// the layer2 3x3 class: staged where the slice allows (wgrad_staged)
static void run_wgrad_c1(const WgArgs& a) {
  return wgrad_staged(a.imgs) ? run_wgrad<Wgrad3x3Map4Staged>(a) : run_wgrad<Wgrad3x3Map4>(a);
}

// ---- plan -----------------------------------------------------------------------------------
static int conv_direct_class(const ConvGeom& g) {
  const bool k3 = g.KH == 3 && g.KW == 3 && g.pad == 1, k1s2 = g.KH == 1 && g.KW == 1 && g.pad == 0 && g.stride == 2;
  const bool ch64 = g.C % 64 == 0 && g.Co % 64 == 0, map8 = g.H == 8 && g.W == 8, map4 = g.H == 4 && g.W == 4;
  if (k3 && g.stride == 1 && map8 && ch64) return kConv3x3Map8;
  if (k3 && g.stride == 1 && map4 && ch64) return kConv3x3Map4;
  if (k3 && g.stride == 2 && map8 && ch64) return kConv3x3S2;
  if (g.KH == 7 && g.KW == 7 && g.pad == 3 && g.stride == 2 && g.H == 32 && g.W == 32 && g.C == 3 && g.Co % 64 == 0)
    return kConvStem;
  if (k1s2 && map8 && ch64) return kConv1x1S2Map8;
  if (k1s2 && map4 && ch64) return kConv1x1S2Map4;
  return kConvNone;
}

// what the host-side plan reads off a class's tiles, and its default images per grad-W slice
struct ClassInfo {
  int fwd_imgs, dgrad_imgs;  // images per workgroup (dgrad_imgs 0: no grad-x kernel)
  int dgrad_pq, dgrad_ups, dgrad_iups;  // grad-x: pixels per image of a compact partial tile; UPS; IUPS
  int wg_cb, wg_bm, wg_slice;
};
template <typename F, typename D, typename Wg>
static constexpr ClassInfo info_of(int wg_slice) {
  return {F::IMGS, D::IMGS, D::PQ, D::UPS, D::IUPS, Wg::CB, Wg::BM, wg_slice};
}
static ClassInfo class_info(int cls) {
  switch (cls) {
    case kConv3x3Map8: return info_of<Fwd3x3Map8, Dgrad3x3Map8, Wgrad3x3Map8>(8);
    case kConv3x3Map4: return info_of<Fwd3x3Map4, Dgrad3x3Map4, Wgrad3x3Map4>(16);  // 32 from batch 512
    case kConv3x3S2: return info_of<Fwd3x3S2, Dgrad3x3S2, Wgrad3x3S2>(16);
    case kConvStem: return info_of<FwdStem, NoTile, WgradStem>(4);
    case kConv1x1S2Map8: return info_of<Fwd1x1S2Map8, Dgrad1x1S2Map8, Wgrad1x1S2Map8>(8);
    case kConv1x1S2Map4: return info_of<Fwd1x1S2Map4, Dgrad1x1S2Map4, Wgrad1x1S2Map4>(16);
    default: return ClassInfo{};
  }
}

static constexpr int kFillWgs = 256;  // one workgroup per CU: below this, split the reduction

// images per grad-W slice: the class default, lowered (power of two dividing B) until the
// grid has >= kFillWgs workgroups.  Workgroups per slice = (Kout / 32) * ceil(Cin / CB).
// (Larger slices = fewer slabs to sum measured slower in round 3: batch 512 x2 1.9937, x4
// 1.9969 vs 1.9904 / 1.9927 ms; batch 256 1.4473 / 1.4444 vs 1.441.)
// Round 5 (Winograd grad-W, deferred batched slab sums): doubling the layer1 (Winograd), 3x3/2 and
// stem slices halves their slabs — ResNet-18 r=4 batch 512 1.5118 / 1.5129 -> 1.4977 / 1.4957 ms;
// doubling layer2's (kConv3x3Map4) was slower, 1.5043 -> 1.5165 (profiles/r5/bench_wgrad_slices.jsonl).
// Round 7 (pipelined operand feeding: LDS prefetch in the layer1 Winograd grad-W, 4-image stages in
// layer2's): the slice sizes re-measured at batch 512 and left as they were — layer1 32-image
// 1.3774 / 1.3784 vs 1.3574 / 1.3605 ms (16), layer2 16-image 1.3745 / 1.3724 and 64-image 1.4457 /
// 1.4447 (32), 3x3/2 32-image 1.3779 / 1.3748 (16) (profiles/r7/bench_wgrad_slices.jsonl; the
// slice overrides of those arms were removed after the runs).
static int conv_wgrad_imgs(int cls, const ClassInfo& ci, const ConvGeom& g, int B) {
  // (the geometry test only, not the runtime Winograd switch: the slicing stays fixed for a shape,
  // so scratch sized from a cached plan fits whichever grad-W kernel runs)
  const bool l1 = cls == kConv3x3Map8 && g.H == 8 && g.C % 16 == 0 && g.Co % 16 == 0;
  if (l1 && B <= 128 && B % 4 == 0) {
    // Winograd grad-W with the 4-wave reduction (winograd.hip wino_wgrad_kernel RED = 4) at the
    // small per-GPU batches: a workgroup per 16 x 16 block and slice, >= one image per wave.
    // ResNet-18 r=4 batch 64 0.843 -> 0.830 ms (4x fewer slabs: grad-W 31.7 -> 29.9 µs, slab sum
    // 16.0 -> 13.3); at batch 256 / 512 the 4 waves of a workgroup reading different images lost
    // (512: grad-W + slab sum 120.9 -> 124.0 µs; 256: 1.102 -> 1.120 ms at 4 images per slice)
    const int per_slice = (g.Co / 16) * (g.C / 16);
    int d = 32;
    while (d > 4 && (B % d != 0 || (B / d) * per_slice < kFillWgs)) d /= 2;
    if (B % d == 0 && wino_wgrad_red(B, d)) return d;
  }
  if (l1 && B >= 256 && B % 16 == 0 && wino_wgrad_red(B, 16)) {
    // from batch 256: 16-image slices over the 4-wave reduction (4 images per wave) — half the
    // slabs of 8-image slices, two workgroups per CU at 512.  ResNet-18 r=4, ms/step: batch 512
    // 1.3866 / 1.3908 vs 1.4043 / 1.4021 (8-image, 2-wave), batch 256 0.9942 / 0.9993 vs 1.0035 /
    // 1.0046 (8-image, 1-wave); 32-image slices 1.4103 (profiles/r6/bench_l1_wgrad_slices.jsonl)
    // (32-image slices lose with the prefetched feeding too: the round-7 note above)
    return 16;
  }
  // layer2 (kConv3x3Map4) from batch 512: 32-image slices, half the slabs.  Its grad-W now runs in one
  // launch with its grad-x (wino_direct_pair_kernel), which fills the CUs: ResNet-18 r=4 batch 512
  // 1.3711 / 1.3692 vs 1.3775 / 1.3804 ms (16-image), and 1.3806 / 1.3819 vs 1.3877 / 1.3886 on a
  // second box; batch 256 unchanged (0.9927 vs 0.9920 / 0.9914) (profiles/r6/bench_l2_wgrad_slices.jsonl)
  int def = (cls == kConv3x3Map4 && B >= 512) ? 32 : ci.wg_slice;
  const int per_slice = (g.Co / ci.wg_bm) * ((g.C + ci.wg_cb - 1) / ci.wg_cb);
  while (def > 1 && B % def != 0) def /= 2;  // a batch that is not a multiple of the default
  while (def > 1 && (B / def) * per_slice < kFillWgs && B % (def / 2) == 0) def /= 2;
  return def;
}

// split-K cap: 4 keeps layer2's slabs summable inside the fused BN kernel (batchnorm.hip
// kMaxFusedSlabs) — ResNet-18 step on 1x MI355X, batch 128 1.216 / 1.197 -> 1.191 / 1.188 ms,
// batch 64 1.050 / 1.050 -> 1.049 / 1.046 (uncapped: 8 slabs at batch 64).  The 1x1 stride-2
// grad-x takes the same cap (a cap of 1 measured 0.960 -> 0.967 ms at batch 64).
static constexpr int kConvMaxSplit = 4;

// split-K factor of the forward (dgrad = false) / grad-x (dgrad = true) kernels: a power of
// two <= the channel chunks, so that (B / IMGS) * (outC / 64) * ksplit >= kFillWgs
static int conv_ksplit(int cls, const ClassInfo& ci, const ConvGeom& g, int B, bool dgrad) {
  if (cls == kConvStem) return 1;
  // the 1x1/2 grad-x runs in one launch with its grad-W (direct_pair_kernel), whose workgroups fill
  // the CUs: unsplit from batch 512 (no slab-sum launch; 1.4306 / 1.4308 -> 1.4192 / 1.4229 ms, at
  // 256 even: 1.0053 vs 1.0076)
  if (dgrad && ci.dgrad_ups == 2 && B >= 512) return 1;
  const int inC = dgrad ? g.Co : g.C, outC = dgrad ? g.C : g.Co;
  const int imgs = dgrad ? ci.dgrad_imgs : ci.fwd_imgs;  // (kConv3x3S2's grad-x: 8x8 tiles, 1 image)
  const int base = (B / imgs) * (outC / 64);
  const int nchunks = inC / 8;
  int ks = 1;
  while (ks * 2 <= nchunks && base * ks < kFillWgs && ks * 2 <= kConvMaxSplit) ks *= 2;
  return ks;
}

// Winograd F(2x2, 3x3) (winograd.hip) for the 3x3 classes: forward of the stride-1 classes, grad-x of
// those and of kConv3x3S2 (its zero-inserted dY is an 8x8 map), launches that tile exactly.  The
// direct kernel's split-K factor ks (small batches) is kept: the Winograd slabs then go to the same
// consumers (slab sum / the fused BN kernel)
static bool conv_wino(int cls, const ConvGeom& g, int B, bool dgrad, int ks) {
  const bool s1 = cls == kConv3x3Map8 || cls == kConv3x3Map4;
  if (dgrad) return (s1 || cls == kConv3x3S2) && wino_ok(g.Co, g.C, B, g.H, g.W, ks);
  return s1 && wino_ok(g.C, g.Co, B, g.H, g.W, ks);
}

// Output-row blocks per image of the stem forward (FwdTile PSPLIT): enough workgroups for
// the 256 CUs at the small per-GPU batches of the strong-scaling runs.  Every split re-stages
// the image and the 64 x 196 weight image, so more blocks only pay below one workgroup per CU.
// Stem forward + statistics epilogue on 1x MI355X (tools/diag/stem_psplit.py, µs, split 1/2/4;
// profiles/r5/stem_psplit*.jsonl): batch 64 20.8 / 15.9 / 12.1, 128 21.4 / 16.7 / 16.9,
// 256 22.9 / 23.5 / 30.9, 512 34.1 / 43.6 / 58.2 (paired-k stem with float4 weight staging;
// before it, 512: 51.5 / 72.3 / 110 — 1 wave per SIMD from 400+ registers of staging state).
static int g_stem_psplit = 0;  // 0 = by batch (A/B override: conv_set_stem_psplit)
void conv_set_stem_psplit(int p) { g_stem_psplit = (p == 1 || p == 2 || p == 4) ? p : 0; }
static int stem_psplit(int B) {
  if (g_stem_psplit) return g_stem_psplit;
  return B >= 256 ? 1 : B >= 128 ? 2 : 4;
}

ConvPlan conv_make_plan(const ConvGeom& g, int B) {
  ConvPlan p;
  const int cls = conv_direct_class(g);
  if (cls < 0) return p;
  const ClassInfo ci = class_info(cls);
  p.cls = cls;
  p.fwd_imgs = ci.fwd_imgs;
  p.wgrad_imgs = conv_wgrad_imgs(cls, ci, g, B);
  // Every class but the stem runs its grad-x natively.  The 3x3 stride-2 grad-x runs on the
  // zero-inserted dY (exact, 4x the MFMA work of the sub-pixel form; round 2: 2.006 / 2.005 vs MIOpen
  // 1.991 ms at batch 512): MIOpen's algorithm choice depends on its on-disk find database and,
  // captured in a hipGraph, was found non-deterministic and NaN-producing (round 3 bisection).
  p.dgrad_direct = ci.dgrad_imgs > 0;
  p.fwd_ksplit = conv_ksplit(cls, ci, g, B, false);
  p.dgrad_ksplit = conv_ksplit(cls, ci, g, B, true);
  p.fwd_wino = conv_wino(cls, g, B, false, p.fwd_ksplit);
  p.dgrad_wino = conv_wino(cls, g, B, true, p.dgrad_ksplit);
  p.fwd_psplit = cls == kConvStem ? stem_psplit(B) : 1;
  // BatchNorm statistics from the forward epilogue: the layer1 3x3 and stem 7x7 classes (their
  // BatchNorms take the two-kernel large-map path; layer2's single-launch BN computes its own), unsplit
  // launches only.  Partials = workgroups along the batch (the stem: one per image and row block).
  static_assert(Fwd3x3Map8::STATS_OK && FwdStem::STATS_OK && FwdStem2::STATS_OK && FwdStem4::STATS_OK,
                "statistics epilogue fits every layer1 / stem tile");
  if (cls == kConvStem) p.fwd_stats_slices = B * p.fwd_psplit;
  else if (cls == kConv3x3Map8 && p.fwd_ksplit == 1) p.fwd_stats_slices = B / (p.fwd_wino ? wino_imgs(g.H) : ci.fwd_imgs);
  // backward-mode BN partial sums from the grad-x epilogue: the layer1 3x3 class (its BN takes the
  // two-kernel large-map path) and kConv3x3S2, which runs the layer1 grad-x kernel (one image per
  // tile); unsplit grad-x launches only
  static_assert(Dgrad3x3Map8::STATS2_OK && Dgrad3x3S2::STATS2_OK, "backward statistics epilogue fits the layer1 grad-x tiles");
  if ((cls == kConv3x3Map8 || cls == kConv3x3S2) && p.dgrad_ksplit == 1)
    p.dgrad_stats_slices = B / (p.dgrad_wino ? wino_imgs(g.H) : ci.dgrad_imgs);
  p.dgrad_slab = (int64_t)B * g.C * ci.dgrad_pq;
  p.dgrad_defer_ok = ci.dgrad_ups == 1;  // (the UPS = 2 sum scatters: conv_slab_sum_ups_kernel)
  return p;
}

// ---- launchers ------------------------------------------------------------------------------
// split-K Winograd slabs: left to the consumer (defer: it sums them, and an addend after them) or
// summed here in slab order (+ addend), like run_fwd
static int wino_slabs(const float* part, float* out, int64_t n, int ks, bool defer, const float* addend, hipStream_t s) {
  if (!defer) launch_slab_sum(part, out, n, ks, s, addend);
  return defer ? ks : 1;
}

// the downsample conv's forward, held for its block's conv1 (kConv3x3S2); x == nullptr: none
static FwdArgs g_pending_fwd{};

void conv_flush_pending_fwd() {
  if (g_pending_fwd.x != nullptr) run_fwd<Fwd1x1S2Map8>(take(g_pending_fwd));
}

int launch_conv_fwd(const float* x, const float* w, float* y, int B, const ConvGeom& g, const ConvPlan& p, float* part,
                    hipStream_t s, bool defer, double* stats_out, float* wino_u, bool pair) {
  const ConvBnStats stats{stats_out, nullptr, nullptr, nullptr, nullptr};
  const int cls = p.cls, ks = p.fwd_ksplit;
  FwdArgs a{x, w, y, B, g.C, g.Co, ks, part, s, nullptr, defer, ConvBnStats{}};
  if (cls == kConv1x1S2Map8 && pair && stats_out == nullptr) {  // held for conv1 (ds_fwd_pair_kernel); same return as run_fwd
    conv_flush_pending_fwd();
    uint3 grid;
    fwd_part<Fwd1x1S2Map8>(a, grid);
    g_pending_fwd = a;
    return (grid.z > 1 && defer) ? (int)grid.z : 1;
  }
  if (cls == kConv3x3S2 && g_pending_fwd.x == x && g_pending_fwd.s == s && g_pending_fwd.B == B && stats_out == nullptr) {
    const FwdArgs b = take(g_pending_fwd);
    uint3 ga, gb;
    const FwdPart fa = fwd_part<Fwd3x3S2>(a, ga), fb = fwd_part<Fwd1x1S2Map8>(b, gb);
    constexpr size_t lds = std::max(Fwd3x3S2::LDS_BYTES, Fwd1x1S2Map8::LDS_BYTES);
    static bool attr = false;
    if (!attr) { set_lds(ds_fwd_pair_kernel, lds); attr = true; }
    hipLaunchKernelGGL(ds_fwd_pair_kernel, dim3(ga.x * ga.y * ga.z + gb.x * gb.y * gb.z), dim3(256), lds, s, fa, ga, fb, gb);
    if (gb.z > 1 && !b.defer) launch_slab_sum(b.part, b.y, fb.slab, (int)gb.z, s, nullptr);
    if (ga.z > 1 && defer) return (int)ga.z;
    if (ga.z > 1) launch_slab_sum(part, y, fa.slab, (int)ga.z, s, nullptr);
    return 1;
  }
  conv_flush_pending_fwd();
  if (wino_u != nullptr && p.fwd_wino) {
    launch_wino_conv(x, wino_u, y, B, g.C, g.Co, g.H, false, 1, nullptr, ks > 1 ? ConvBnStats{} : stats, ks, part, s);
    return ks > 1 ? wino_slabs(part, y, (int64_t)B * g.Co * g.H * g.W, ks, defer, nullptr, s) : 1;
  }
  if (cls == kConv3x3Map8 || cls == kConvStem) a.stats = stats;  // the classes with a statistics epilogue
  switch (cls) {
    case kConv3x3Map8: return run_fwd<Fwd3x3Map8>(a);
    case kConv3x3Map4: return run_fwd<Fwd3x3Map4>(a);
    case kConv3x3S2: return run_fwd<Fwd3x3S2>(a);
    case kConvStem:  // (never split: fwd_ksplit == 1)
      return p.fwd_psplit == 4   ? run_fwd<FwdStem4>(a)
             : p.fwd_psplit == 2 ? run_fwd<FwdStem2>(a)
                                 : run_fwd<FwdStem>(a);
    case kConv1x1S2Map8: return run_fwd<Fwd1x1S2Map8>(a);
    case kConv1x1S2Map4: return run_fwd<Fwd1x1S2Map4>(a);
    default: return 1;
  }
}

// A grad-W held back by launch_conv_wgrad(pair = true) for the grad-x of the same conv (host state
// only: set and consumed within one conv backward, capture-safe)
namespace {
struct PendingWgrad {
  WgArgs a;    // partials only (a.dw == nullptr); a.dy == nullptr: an empty slot
  int cls, H;  // the conv's class and map size
};
// two slots: a downsample block's two sibling convs (3x3/2 and 1x1/2) each hold one while the
// BranchLink defers one of their grad-x launches into the other's backward
constexpr int kPendingSlots = 2;
PendingWgrad g_pending[kPendingSlots];
unsigned g_pending_seq[kPendingSlots];
unsigned g_seq = 0;

// a held-back grad-W on its own (partials only; the classes launch_conv_wgrad holds)
void launch_pending(const PendingWgrad& p) {
  const WgArgs& a = p.a;
  switch (p.cls) {
    case kConv3x3Map8: return launch_wino_wgrad(a.x, a.dy, a.part, a.B, a.Cin, a.Kout, p.H, a.imgs, a.s);
    case kConv3x3Map4: return run_wgrad_c1(a);
    case kConv3x3S2: return run_wgrad<Wgrad3x3S2>(a);
    case kConv1x1S2Map8: return run_wgrad<Wgrad1x1S2Map8>(a);
    case kConv1x1S2Map4: return run_wgrad<Wgrad1x1S2Map4>(a);
    default: return;
  }
}
// the held-back grad-W of THIS grad-x's conv (same dY, same geometry and stream), or nullptr
PendingWgrad* find_pending(const float* dy, int cls, int B, const ConvGeom& g, hipStream_t s) {
  for (auto& p : g_pending)
    if (p.a.dy == dy && p.cls == cls && p.a.s == s && p.a.B == B && p.a.Cin == g.C && p.a.Kout == g.Co && p.H == g.H)
      return &p;
  return nullptr;
}
// launch (alone) whatever is held for this dY
void flush_pending_dy(const float* dy) {
  for (auto& p : g_pending)
    if (p.a.dy == dy) launch_pending(take(p));
}
// hold a grad-W: a free slot, else the oldest one is launched alone first
void hold_pending(const PendingWgrad& q) {
  int k = -1;
  for (int i = 0; i < kPendingSlots; ++i)
    if (g_pending[i].a.dy == nullptr) { k = i; break; }
  if (k < 0) {
    k = g_pending_seq[0] <= g_pending_seq[1] ? 0 : 1;
    launch_pending(take(g_pending[k]));
  }
  g_pending[k] = q;
  g_pending_seq[k] = ++g_seq;
}

// grad-x of a layer2 class on the Winograd kernel (its map size and zero insertion are those of the
// class's direct grad-x tile D) + the held-back direct grad-W (tile Wg), one launch
template <typename D, typename Wg>
void run_pair(const float* dy, const float* u, float* dx, int B, int inC, int outC, const float* addend,
              const ConvBnStats& st, int ks, float* part_x, const WgArgs& p, hipStream_t s) {
  constexpr int WH = D::H, IUPS = D::IUPS;
  auto k = wino_direct_pair_kernel<WH, IUPS, Wg::R, Wg::S, Wg::ST, Wg::PD, Wg::H, Wg::W, Wg::CB, Wg::BM, Wg::NW,
                                   Wg::NBPW, Wg::KB, Wg::IPS>;
  constexpr size_t lds = std::max<size_t>(kWLds, Wg::LDS_BYTES);
  static bool attr = false;
  if (!attr) { set_lds(k, lds); attr = true; }
  const WinoConvArgs a{dy, u + 16 * (int64_t)inC * outC,  // the grad-x half of the transforms
                       dx, inC, outC, ks > 1 ? nullptr : addend, ks > 1 ? ConvBnStats{} : st, (inC / kWCK) / ks,
                       part_x, (int64_t)B * outC * WH * WH};
  const uint3 ga = make_uint3((unsigned)(B / wino_imgs(WH)), (unsigned)(outC / kWBM), (unsigned)ks);
  const uint3 gw = wgrad_grid<Wg>(p);
  const unsigned n = ga.x * ga.y * ga.z + gw.x * gw.y * gw.z;
  hipLaunchKernelGGL(k, dim3(n), dim3(256), lds, s, a, ga, p.x, p.dy, p.part, p.Cin, p.Kout, p.imgs, gw);
  ++g_pair_launches;
}
// the 1x1 stride-2 grad-x (tile F: run_fwd's UPS = 2 path, incl. its split-K slab sum) + the held-back
// direct grad-W of the same conv (tile Wg), one launch
template <typename F, typename Wg>
int run_direct_pair(const FwdArgs& a, const WgArgs& p) {
  static_assert(std::is_same<F, DsDgradTile<F::H, F::W, F::BM, F::IMGS>>::value, "the tile direct_pair_kernel runs");
  uint3 ga;
  const FwdPart f = fwd_part<F>(a, ga);
  DirectDgradArgs d{f.x, f.w, f.y, f.part, f.Cin, f.Kout, f.cps, f.slab, ga.z > 1 ? nullptr : a.addend, DsArgs{}, DsWgArgs{}};
  uint3 gw = wgrad_grid<Wg>(p);
  // the streamed halves (ds_stream.h): their own grids, the same slabs; off: the old pair
  const auto launch = [&](auto k, size_t lds, const uint3& gx) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const unsigned n = gx.x * gx.y * gx.z + gw.x * gw.y * gw.z;
    hipLaunchKernelGGL(k, dim3(n), dim3(256), lds, a.s, d, gx, p.x, p.dy, p.part, p.Cin, p.Kout, p.imgs, gw);
  };
#define NDP_DIRECT_PAIR(STREAM)                                                                              \
  direct_pair_kernel<STREAM, F::H, F::W, F::BM, F::IMGS, Wg::R, Wg::S, Wg::ST, Wg::PD, Wg::H, Wg::W, Wg::CB, \
                     Wg::BM, Wg::NW, Wg::NBPW, Wg::KB>
  uint3 gs, gsw;
  if (ds_part<DsOf<F>::MAP, true>(a, d.ds, gs) && ds_wg_part(p, d.dsw, gsw)) {
    gw = gsw;
    launch(NDP_DIRECT_PAIR(true), 0, gs);
  } else {
    launch(NDP_DIRECT_PAIR(false), std::max(F::LDS_BYTES, Wg::LDS_BYTES), ga);
  }
#undef NDP_DIRECT_PAIR
  ++g_pair_launches;
  if (ga.z > 1) launch_slab_sum_ups<F>(a.part, a.y, f.slab, (int)ga.z, a.s, a.addend);
  return 1;
}
}  // namespace

// every held-back grad-W, oldest first
void conv_flush_pending() {
  while (true) {
    int k = -1;
    for (int i = 0; i < kPendingSlots; ++i)
      if (g_pending[i].a.dy != nullptr && (k < 0 || g_pending_seq[i] < g_pending_seq[k])) k = i;
    if (k < 0) return;
    launch_pending(take(g_pending[k]));
  }
}

// dx[B, C, H, W] from dy[B, Co, OH, OW]
int launch_conv_dgrad(const float* dy, const float* w, float* dx, int B, const ConvGeom& g, const ConvPlan& p,
                      float* part, hipStream_t s, const float* addend, bool defer, const ConvBnStats* bst,
                      float* wino_u) {
  const ConvBnStats stats = bst != nullptr ? *bst : ConvBnStats{nullptr, nullptr, nullptr, nullptr, nullptr};
  const int cls = p.cls, ks = p.dgrad_ksplit;
  const ClassInfo ci = class_info(cls);
  if (wino_u != nullptr && p.dgrad_wino) {
    if (PendingWgrad* pp = find_pending(dy, cls, B, g, s)) {
      // this conv's grad-W is waiting: both in one launch
      const WgArgs q = take(*pp).a;
      if (cls == kConv3x3Map8) {
        launch_wino_bwd_pair(dy, wino_u, dx, B, g.Co, g.C, addend, stats, ks, part, q.x, q.part, q.imgs, s);
        ++g_pair_launches;
      } else if (cls == kConv3x3Map4 && wgrad_staged(q.imgs))
        run_pair<Dgrad3x3Map4, Wgrad3x3Map4Staged>(dy, wino_u, dx, B, g.Co, g.C, addend, stats, ks, part, q, s);
      else if (cls == kConv3x3Map4)
        run_pair<Dgrad3x3Map4, Wgrad3x3Map4>(dy, wino_u, dx, B, g.Co, g.C, addend, stats, ks, part, q, s);
      else
        run_pair<Dgrad3x3S2, Wgrad3x3S2>(dy, wino_u, dx, B, g.Co, g.C, addend, stats, ks, part, q, s);
    } else {
      flush_pending_dy(dy);  // this conv's own grad-W, not pairable after all
      launch_wino_conv(dy, wino_u, dx, B, g.Co, g.C, g.H, true, ci.dgrad_iups, addend, ks > 1 ? ConvBnStats{} : stats, ks,
                       part, s);
    }
    return ks > 1 ? wino_slabs(part, dx, (int64_t)B * g.C * g.H * g.W, ks, defer, addend, s) : 1;
  }
  FwdArgs a{dy, w, dx, B, g.Co, g.C, ks, part, s, addend, defer, ConvBnStats{}};
  if (PendingWgrad* pp = ci.dgrad_ups == 2 ? find_pending(dy, cls, B, g, s) : nullptr) {
    // the downsample conv's grad-W is waiting: both in one launch
    const WgArgs q = take(*pp).a;
    return cls == kConv1x1S2Map8 ? run_direct_pair<Dgrad1x1S2Map8, Wgrad1x1S2Map8>(a, q)
                                 : run_direct_pair<Dgrad1x1S2Map4, Wgrad1x1S2Map4>(a, q);
  }
  flush_pending_dy(dy);
  if (cls == kConv3x3Map8 || cls == kConv3x3S2) a.stats = stats;  // the layer1 grad-x kernel's statistics epilogue
  switch (cls) {
    case kConv3x3Map8: return run_fwd<Dgrad3x3Map8>(a);
    case kConv3x3Map4: return run_fwd<Dgrad3x3Map4>(a);
    case kConv3x3S2: return run_fwd<Dgrad3x3S2>(a);
    case kConv1x1S2Map8: return run_fwd<Dgrad1x1S2Map8>(a);
    case kConv1x1S2Map4: return run_fwd<Dgrad1x1S2Map4>(a);
    default: return 1;
  }
}

// part: (B / p.wgrad_imgs) * Co * C * KH * KW floats of scratch
void launch_conv_wgrad(const float* x, const float* dy, float* part, float* dw, int B, const ConvGeom& g,
                       const ConvPlan& p, hipStream_t s, bool pair) {
  // a grad-W held back earlier stays held (its grad-x may come later, e.g. from the BranchLink
  // sibling's backward) unless this one needs its slot
  const int cls = p.cls, imgs = p.wgrad_imgs;
  const WgArgs a{x, dy, part, dw, B, g.C, g.Co, imgs, s};
  if (cls == kConv3x3Map8 && wino_wgrad_ok(g.C, g.Co, g.H)) {
    // held back for this conv's grad-x (launch_conv_dgrad).  ResNet-18 r=4, ms/step
    // (profiles/r6/bench_wino_pair.jsonl): batch 64 0.7758 / 0.7656 -> 0.7498 / 0.7517, 128
    // 0.8676 -> 0.8434, 256 (with the layer2 pairs) 1.0539 / 1.0572 -> 1.0303 / 1.0343; at 512 the
    // pair was slower with the one-wave-per-block grad-W (1.4640 -> 1.4818), faster with the
    // two-wave one (winograd.hip wgrad_red: 1.4143 / 1.4147 -> 1.3934 / 1.3966)
    if (pair && dw == nullptr) return hold_pending(PendingWgrad{a, cls, g.H});
    // Winograd-domain grad-W (winograd.hip): same slab layout and slicing as the direct kernel.
    // Layer1 only: ResNet-18 at batch 512 90.7 vs 130.2 µs per step (4 launches), batch 64 31.1 vs
    // 38.5; the 4x4 maps (one tile per lane group and image: a load per 16 MFMAs) measured slower,
    // 142.8 vs 99.0 µs at batch 512 and 64.0 vs 29.5 at batch 64 (profiles/r5)
    launch_wino_wgrad(x, dy, part, B, g.C, g.Co, g.H, imgs, s);
    if (dw != nullptr) launch_slab_sum(part, dw, (int64_t)g.Co * g.C * 9, B / imgs, s);
    return;
  }
  // the layer2 3x3 classes likewise when their grad-x takes the Winograd kernel: the 3x3 class at
  // every batch (with / without, ms/step: batch 64 0.7381 / 0.7371 vs 0.7493 / 0.7495, 256
  // 1.0539 / 1.0572 vs 1.0700 / 1.0783, 512 1.4433 / 1.4427 vs 1.4566 / 1.4542); the 3x3/2 class
  // (its grad-x comes from the downsample sibling's backward) up to 256 (128 0.8243 vs 0.8303, 256
  // 1.0196 vs 1.0339, 64 0.7295-0.7439 vs 0.7329-0.7385; 512 1.4504 / 1.4453 vs 1.4470 / 1.4431)
  // The 1x1 stride-2 downsample classes (direct grad-x + direct grad-W, direct_pair_kernel) at every
  // batch: 64 0.7218 / 0.7264 vs 0.7301 / 0.7311, 256 1.0125 vs 1.0256, 512 1.4396 / 1.4355 vs
  // 1.4469 / 1.4360.
  const bool wino_pair = (cls == kConv3x3Map4 || (cls == kConv3x3S2 && B <= 256)) && p.dgrad_wino;
  if (pair && dw == nullptr && (wino_pair || cls == kConv1x1S2Map8 || cls == kConv1x1S2Map4))
    return hold_pending(PendingWgrad{a, cls, g.H});
  switch (cls) {
    case kConv3x3Map8: return run_wgrad<Wgrad3x3Map8>(a);
    case kConv3x3Map4: return run_wgrad_c1(a);
    case kConv3x3S2: return run_wgrad<Wgrad3x3S2>(a);
    case kConvStem: return run_wgrad<WgradStem>(a);
    case kConv1x1S2Map8: return run_wgrad<Wgrad1x1S2Map8>(a);
    case kConv1x1S2Map4: return run_wgrad<Wgrad1x1S2Map4>(a);
    default: return;
  }
}

}  // namespace ndp
