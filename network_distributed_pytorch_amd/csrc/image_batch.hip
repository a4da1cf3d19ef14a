// Batch assembly from byte images on gfx950: gather by index, normalise, random crop + flip,
// ragged-tail padding and the targets, in ONE launch that writes the fp32 batch in place.
//
// The reference feeds its model through torchvision (RandomCrop/ToTensor/Normalize on the host)
// and a DataLoader (ddp_powersgd_guide_cifar10/ddp_init.py:40-58).  Here the images stay in HBM
// as bytes and each batch costs one kernel instead of index_select + copy_ per column.
//
// The rule (ops/image_batch.py holds the bitwise torch twin), per output row b:
//   i = idx[b];  h = hash4(seed, epoch, i, 0), h2 = hash4(seed, epoch, i, 1)
//   dx = (((h & 0xFFFF) * (2p+1)) >> 16) - p,  dy = (((h >> 16) * (2p+1)) >> 16) - p,
//   flip = h2 >> 31  (0 when flips are off)
//   out[b, c, y, x] = fmaf(float(src[i, c, y + dy, (flip ? 31 - x : x) + dx]), scale[c], shift[c])
//   with byte 0 for a source coordinate outside [0, 32)  (= RandomCrop(32, padding=p), then flip)
//   target[b] = labels[i]
//   rows b >= m, and rows whose index is outside [0, N): zero image, target = pad_target; the
//   latter also store 1 into *err (every writer stores the same value; the index is never used
//   as an address).
//
// Shape: one 256-lane workgroup per (b, c) plane.  idx[b], the hash and dx / dy / flip depend on
// blockIdx only, so they stay in scalar registers.  The 1 KiB source plane is staged in LDS by
// one coalesced dword load per lane; each lane then builds four consecutive output pixels from
// LDS bytes and writes them with one 16-byte store, so a workgroup writes one contiguous 4 KiB.
// Per byte read the 8 lanes of an image row touch 8 different dwords of that row (in-range
// columns only) and rows are 8 dwords apart, so a 32-lane half reads 32 different banks.
// No atomics, no cross-workgroup traffic.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "counter_hash.h"
#include "ndp_kernels.h"

namespace ndp {

__global__ __launch_bounds__(256) void image_batch_kernel(const uint8_t* __restrict__ src,
                                                          const int64_t* __restrict__ labels,
                                                          const int64_t* __restrict__ idx, float* __restrict__ out,
                                                          int64_t* __restrict__ out_target, int m, int64_t N, int C,
                                                          ImageNorm norm, int pad, int flip_on, uint32_t seed,
                                                          uint32_t epoch, int64_t pad_target, int* __restrict__ err) {
  __shared__ uint32_t plane[256];
  const int b = (int)(blockIdx.x / (unsigned)C);
  const int c = (int)(blockIdx.x % (unsigned)C);
  const int lane = threadIdx.x;
  float4* dst = reinterpret_cast<float4*>(out + ((int64_t)b * C + c) * 1024) + lane;

  const int64_t i = b < m ? idx[b] : -1;
  if (i < 0 || i >= N) {  // workgroup-uniform: tail row or bad index, nothing is read through i
    *dst = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c == 0 && lane == 0) {
      out_target[b] = pad_target;
      if (b < m) *err = 1;
    }
    return;
  }

  plane[lane] = reinterpret_cast<const uint32_t*>(src + (i * C + c) * 1024)[lane];

  float sc = 0.f, sh = 0.f;
#pragma unroll
  for (int k = 0; k < kImageMaxC; ++k)
    if (c == k) { sc = norm.scale[k]; sh = norm.shift[k]; }
  int dx = 0, dy = 0;
  if (pad > 0) {
    const uint32_t h = counter_hash4(seed, epoch, (uint32_t)i, 0u);
    const uint32_t span = 2u * (uint32_t)pad + 1u;
    dx = (int)(((h & 0xFFFFu) * span) >> 16) - pad;
    dy = (int)(((h >> 16) * span) >> 16) - pad;
  }
  const bool flip = flip_on && (counter_hash4(seed, epoch, (uint32_t)i, 1u) >> 31);
  __syncthreads();

  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(plane);
  const int y = lane >> 3, x0 = (lane & 7) * 4;
  const int sy = y + dy;
  const bool row_ok = (unsigned)sy < 32u;
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = x0 + j;
    const int sx = (flip ? 31 - x : x) + dx;
    const bool ok = row_ok && (unsigned)sx < 32u;
    const uint32_t px = ok ? bytes[sy * 32 + sx] : 0u;
    v[j] = fmaf((float)px, sc, sh);
  }
  *dst = make_float4(v[0], v[1], v[2], v[3]);
  if (c == 0 && lane == 0) out_target[b] = labels[i];
}

void launch_image_batch(const uint8_t* src, const int64_t* labels, const int64_t* idx, float* out,
                        int64_t* out_target, int m, int B, int64_t N, int C, const ImageNorm& norm, int pad,
                        int flip_on, uint32_t seed, uint32_t epoch, int64_t pad_target, int* err, hipStream_t s) {
  hipLaunchKernelGGL(image_batch_kernel, dim3((unsigned)B * (unsigned)C), dim3(256), 0, s, src, labels, idx, out,
                     out_target, m, N, C, norm, pad, flip_on, seed, epoch, pad_target, err);
}

// ---- the same batch with mixup / CutMix (ops/image_batch.py: image_mix_batch holds the twin) ----
// Row b is mixed with the row of the reversed batch, b' = m - 1 - b, j = idx[b']:
//   h3 = hash4(seed, epoch, i, 2);  mixed = (h3 >> 8) < thr && b' != b && 0 <= j < N
//   (thr = int(mix_prob * 2^24) from the host; a partner index outside [0, N) is never used as an
//   address: the row stays unmixed and *err is set)
//   kind: mode 1 mixup, 2 CutMix, 3 CutMix iff h3 & 1;  h4 = hash4(.., i, 3), h5 = hash4(.., i, 4)
//   va = image_batch's pixel for sample i with i's crop / flip draw, vb = the same for j with j's
//   mixup:  lam = float(h4 >> 8) * 2^-24;  out = fadd(fmul(lam, va), fmul(1 - lam, vb)), three fp32
//           roundings (mixup_blend keeps the products from the add's view.  HIP's __fmul_rn /
//           __fadd_rn are plain * and + and the build's -ffp-contract=fast would fuse them)
//   CutMix: side = isqrt(h4 >> 16) >> 3;  cx = ((h5 & 0xFFFF) * 32) >> 16, cy = ((h5 >> 16) * 32) >> 16
//           x0 = max(cx - side / 2, 0), x1 = min(cx - side / 2 + side, 32), y0 / y1 likewise
//           out = vb inside the box (output coordinates), va outside: a select
//           lam = float(1024 - (x1 - x0) * (y1 - y0)) / 1024
//   unmixed: out = va (bitwise image_batch_kernel's), lam = 1, target_b = target
//   target[b] = labels[i], target_b[b] = mixed ? labels[j] : labels[i], lam[b]
//   padding rows and rows with a bad own index: as above, target_b = pad_target, lam = 1.
//
// Shape: image_batch_kernel's.  One workgroup per (b, c) plane; i, j, the five hashes, both
// draws, the kind, lam and the box depend on blockIdx only and stay in scalar registers.  Both
// source planes are staged in LDS (2 KiB, one coalesced dword load per lane per plane); the
// partner's load, its pixels and the mixing are skipped when the row is unmixed, a
// workgroup-uniform branch.  The second plane sits 1 KiB = 256 dwords behind the first, a whole
// number of bank rounds, so a byte of plane B lies in the bank of the same byte of plane A and
// the header's argument holds for each plane's reads: per byte read the 8 lanes of an image row
// touch 8 different dwords of that row and rows are 8 dwords apart, so a 32-lane half reads 32
// different banks.  Each lane writes its four pixels with one 16-byte store; lane 0 of plane 0
// writes the row's targets and lam.  No atomics, no cross-workgroup traffic.
__device__ __forceinline__ void image_row_draw(uint32_t seed, uint32_t epoch, int64_t i, int pad, int flip_on, int& dx,
                                               int& dy, bool& flip) {
  dx = 0;
  dy = 0;
  if (pad > 0) {
    const uint32_t h = counter_hash4(seed, epoch, (uint32_t)i, 0u);
    const uint32_t span = 2u * (uint32_t)pad + 1u;
    dx = (int)(((h & 0xFFFFu) * span) >> 16) - pad;
    dy = (int)(((h >> 16) * span) >> 16) - pad;
  }
  flip = flip_on && (counter_hash4(seed, epoch, (uint32_t)i, 1u) >> 31);
}

// four consecutive pixels of output row y from x0 on, from a staged plane: image_batch_kernel's body
__device__ __forceinline__ void image_four_pixels(const uint8_t* bytes, int y, int x0, int dx, int dy, bool flip,
                                                  float sc, float sh, float (&v)[4]) {
  const int sy = y + dy;
  const bool row_ok = (unsigned)sy < 32u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = x0 + j;
    const int sx = (flip ? 31 - x : x) + dx;
    const bool ok = row_ok && (unsigned)sx < 32u;
    const uint32_t px = ok ? bytes[sy * 32 + sx] : 0u;
    v[j] = fmaf((float)px, sc, sh);
  }
}

// lam * a + oml * b in three fp32 roundings.  -ffp-contract=fast disregards the contraction
// pragmas, so the two products pass through an empty asm: the add then has no multiply to fuse.
__device__ __forceinline__ float mixup_blend(float lam, float oml, float a, float b) {
  float p = lam * a;
  float q = oml * b;
  asm volatile("" : "+v"(p), "+v"(q));
  return p + q;
}

__global__ __launch_bounds__(256) void image_mix_batch_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ labels, const int64_t* __restrict__ idx,
    float* __restrict__ out, int64_t* __restrict__ out_target, int64_t* __restrict__ out_target_b,
    float* __restrict__ out_lam, int m, int64_t N, int C, ImageNorm norm, int pad, int flip_on, uint32_t seed,
    uint32_t epoch, int64_t pad_target, int* __restrict__ err, int mode, uint32_t thr) {
  __shared__ uint32_t plane[512];  // [0, 256): sample i's plane, [256, 512): the partner's
  const int b = (int)(blockIdx.x / (unsigned)C);
  const int c = (int)(blockIdx.x % (unsigned)C);
  const int lane = threadIdx.x;
  float4* dst = reinterpret_cast<float4*>(out + ((int64_t)b * C + c) * 1024) + lane;

  const int64_t i = b < m ? idx[b] : -1;
  if (i < 0 || i >= N) {  // workgroup-uniform: tail row or bad index, nothing is read through i
    *dst = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c == 0 && lane == 0) {
      out_target[b] = pad_target;
      out_target_b[b] = pad_target;
      out_lam[b] = 1.f;
      if (b < m) *err = 1;
    }
    return;
  }

  // the mixing draw of the row: scalar
  const int bp = m - 1 - b;  // in [0, m) because b < m here
  const int64_t j = idx[bp];
  const uint32_t h3 = counter_hash4(seed, epoch, (uint32_t)i, 2u);
  const bool drawn = (h3 >> 8) < thr && bp != b;
  const bool partner_ok = j >= 0 && j < N;
  const bool mixed = drawn && partner_ok;  // workgroup-uniform; j is an address only below this
  const bool cut = mode == 2 || (mode == 3 && (h3 & 1u));

  plane[lane] = reinterpret_cast<const uint32_t*>(src + (i * C + c) * 1024)[lane];
  if (mixed) plane[256 + lane] = reinterpret_cast<const uint32_t*>(src + (j * C + c) * 1024)[lane];

  float sc = 0.f, sh = 0.f;
#pragma unroll
  for (int k = 0; k < kImageMaxC; ++k)
    if (c == k) { sc = norm.scale[k]; sh = norm.shift[k]; }
  int dx, dy;
  bool flip;
  image_row_draw(seed, epoch, i, pad, flip_on, dx, dy, flip);

  float lam = 1.f;
  int bx0 = 0, bx1 = 0, by0 = 0, by1 = 0;  // CutMix box, empty unless drawn
  if (mixed) {
    const uint32_t h4 = counter_hash4(seed, epoch, (uint32_t)i, 3u);
    if (cut) {
      const uint32_t h5 = counter_hash4(seed, epoch, (uint32_t)i, 4u);
      const int u = (int)(h4 >> 16);
      int r = (int)sqrtf((float)u);  // isqrt(u), u < 65536: corrected in integers whatever sqrtf rounds to
      if (r * r > u) --r;
      if ((r + 1) * (r + 1) <= u) ++r;
      const int side = r >> 3;  // [0, 31]
      const int cx = (int)(((h5 & 0xFFFFu) * 32u) >> 16), cy = (int)(((h5 >> 16) * 32u) >> 16);
      bx0 = max(cx - (side >> 1), 0);
      bx1 = min(cx - (side >> 1) + side, 32);
      by0 = max(cy - (side >> 1), 0);
      by1 = min(cy - (side >> 1) + side, 32);
      lam = (float)(1024 - (bx1 - bx0) * (by1 - by0)) * (1.f / 1024.f);
    } else {
      lam = (float)(h4 >> 8) * (1.f / 16777216.f);
    }
  }
  __syncthreads();

  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(plane);
  const int y = lane >> 3, x0 = (lane & 7) * 4;
  float v[4];
  image_four_pixels(bytes, y, x0, dx, dy, flip, sc, sh, v);
  if (mixed) {
    int dxb, dyb;
    bool flipb;
    image_row_draw(seed, epoch, j, pad, flip_on, dxb, dyb, flipb);
    float w[4];
    image_four_pixels(bytes + 1024, y, x0, dxb, dyb, flipb, sc, sh, w);
    if (cut) {
      const bool in_rows = y >= by0 && y < by1;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = (in_rows && x0 + k >= bx0 && x0 + k < bx1) ? w[k] : v[k];
    } else {
      const float oml = 1.f - lam;  // exact: lam is a multiple of 2^-24 in [0, 1)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = mixup_blend(lam, oml, v[k], w[k]);
    }
  }
  *dst = make_float4(v[0], v[1], v[2], v[3]);
  if (c == 0 && lane == 0) {
    const int64_t t = labels[i];
    out_target[b] = t;
    out_target_b[b] = mixed ? labels[j] : t;
    out_lam[b] = lam;
    if (!partner_ok) *err = 1;  // the partner's own row reports it too: every writer stores 1
  }
}

void launch_image_mix_batch(const uint8_t* src, const int64_t* labels, const int64_t* idx, float* out,
                            int64_t* out_target, int64_t* out_target_b, float* out_lam, int m, int B, int64_t N,
                            int C, const ImageNorm& norm, int pad, int flip_on, uint32_t seed, uint32_t epoch,
                            int64_t pad_target, int* err, int mode, uint32_t thr, hipStream_t s) {
  hipLaunchKernelGGL(image_mix_batch_kernel, dim3((unsigned)B * (unsigned)C), dim3(256), 0, s, src, labels, idx, out,
                     out_target, out_target_b, out_lam, m, N, C, norm, pad, flip_on, seed, epoch, pad_target, err,
                     mode, thr);
}

}  // namespace ndp
