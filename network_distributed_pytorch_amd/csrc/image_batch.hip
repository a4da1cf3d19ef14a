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

}  // namespace ndp
