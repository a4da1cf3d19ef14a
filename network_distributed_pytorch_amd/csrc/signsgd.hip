// Scaled-sign gradient compression with error feedback (EF-SignSGD, the PowerSGD paper's "Sign+Norm")
// over flat fp32 arenas, exact: one bit per coordinate of m = g + e plus one fp32 magnitude per block
// of kSignBlock = 2048 elements, and the decompress + momentum + SGD update behind the all-gather.
// Two launches, one workgroup of 256 threads per block, no workgroup ever needs another's result: no
// ticket, no atomic, every store a plain per-lane vector store.
//
// Block table: int32 [nb][2] = (off_j, len_j), off_j a multiple of 16, 1 <= len_j <= 2048 (a tensor is
// cut into blocks of 2048 and only its last block is ragged).  Arena elements outside every block are
// neither read nor written.
//
// Thread map (both launches): thread tid = 64 wave + lane owns the in-block elements
//     t = 1024 h + 4 tid + c,   h = 0, 1 (round),  c = 0 .. 3 (float4 component),
// two float4 per arena, every load in flight before the first use (a quad that crosses len_j falls back
// to scalar loads; absent elements hold m = +0 and are never stored).
//
// sign_pack:  m = fadd(g, e) stays in 8 registers per thread across the one barrier.
//   S_j, the fp64 sum of |m|, in ONE order that is part of the rule (ops/signsgd.py repeats it):
//     lane:   s = 0;  for h = 0, 1: for c = 0 .. 3:  s += (double)|m[h][c]|
//     wave:   for o = 32, 16, 8, 4, 2, 1:  s += s of lane ^ o        (a butterfly: every lane ends equal)
//     block:  S = 0;  for wave = 0 .. 3:  S += s_wave                (through 4 doubles of LDS)
//   An absent element adds +0.0, so the order does not depend on len_j.
//   s_j = (float)(S / (double)len_j)   (IEEE fp64 division, one rounding to fp32; NaN / inf pass through)
//   c   = the float with the bits (bits(s_j) & 0x7fffffff) | (bits(m) & 0x80000000);   e' = fsub(m, c)
//   Signs: one wave ballot per (h, c) gives the 64-bit mask M[h][wave][c], bit `lane` = bits(m) >> 31.
//   Wire buffer of a rank, int32 [nb * 65]: nb * 64 sign words, then nb words bits(s_j).  Block j owns
//   the sign words [64 j, 64 j + 64): mask M[h][wave][c] is the little-endian 64-bit word number
//   p = 16 h + 4 wave + c = 4 (t >> 8) + (t & 3) of them, so for the in-block element t
//       word(t) = 64 j + 8 (t >> 8) + 2 (t & 3) + ((t >> 7) & 1),     bit(t) = (t >> 2) & 31.
//   Lane 0 of a wave stores its 8 masks as four 16-byte stores; bits of absent elements are 0.
//
// sign_update:  the x / b quads are in flight first.  gathered is int32 [N][nb * 65], one wire buffer per
//   rank.  Rank after rank the wave reads its 8 masks and the block's scale with uniform (scalar) loads,
//   rank r + 1's requested before rank r's are consumed; the lane picks its bit, and
//     acc = 0;  for r = 0 .. N-1:  acc = fadd(acc, c_r)         (registers; rank order)
//     o  = (N != 1) ? acc / N : acc                             (IEEE division)
//     d  = (wd != 0) ? fmaf(wd, x, o) : o
//     b' = fadd(fmul(b, lambda), d);  up = fadd(d, b');  x' = fmaf(-lr, up, x)
//   No LDS: every rank's contribution to an element sits at the same place of its row.  lr / wd come
//   from the nullable hyper block (hyper.h).
//
// sign_update_adam:  the same loads and decode (sign_accumulate), then AdamW (adamw_elem.h) on o in the
//   place of the momentum rule; b is the first moment, a third arena the second.  It alone has a barrier,
//   8 bytes of LDS and a ticket: the AdamBlock protocol of adam_block.h (ef_block.h: ef_adam_tail).
//
// The rule's adds and subtractions are single scalar instructions (fadd_scalar / fsub_scalar): the
// build's -ffp-contract=fast has nothing to fuse them with, and the compiler cannot pair neighbouring
// components into packed fp32 instructions, which this file does without.  They, the quad access and
// the element rule (sign_step) live in ef_block.h, which quant.hip shares.
#include <hip/hip_runtime.h>

#include "ef_block.h"
#include "hyper.h"
#include "ndp_kernels.h"

namespace ndp {

namespace {

constexpr int kThreads = 256;
constexpr int kRounds = kSignBlock / (4 * kThreads);  // float4 rounds per thread and block
static_assert(kRounds == 2 && kSignWords == kSignBlock / 32 + 1, "thread map and wire layout");
static_assert(kRounds == kEfRounds && kThreads == kEfThreads, "ef_block.h's AdamW pieces use the same thread map");

__device__ __forceinline__ float with_sign(unsigned mag, unsigned sign_bit31) {
  return __builtin_bit_cast(float, mag | sign_bit31);
}

// v of lane ^ o (wave64)
__device__ __forceinline__ double lane_xor(double v, int lane, int o) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const int at = (lane ^ o) << 2;
  const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(at, (int)(unsigned)u);
  const unsigned hi = (unsigned)__builtin_amdgcn_ds_bpermute(at, (int)(unsigned)(u >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

__global__ __launch_bounds__(kThreads) NDP_NO_PACKED_F32 void sign_pack_kernel(const float* __restrict__ g,
                                                                               float* __restrict__ e,
                                                                               const int* __restrict__ table, int nb,
                                                                               int32_t* __restrict__ out) {
  __shared__ double ws[4];
  const int j = blockIdx.x;
  const int off = table[2 * j], len = table[2 * j + 1];  // uniform address: scalar loads
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float* __restrict__ gb = g + off;
  float* __restrict__ eb = e + off;
  Quad m[kRounds], gq[kRounds];
#pragma unroll
  for (int h = 0; h < kRounds; ++h) m[h] = load_quad(eb, h * 4 * kThreads + 4 * tid, len);
#pragma unroll
  for (int h = 0; h < kRounds; ++h) gq[h] = load_quad(gb, h * 4 * kThreads + 4 * tid, len);
  double s = 0.0;
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      m[h].v[c] = fadd_scalar(gq[h].v[c], m[h].v[c]);
      s += (double)__builtin_fabsf(m[h].v[c]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += lane_xor(s, lane, o);
  if (lane == 0) ws[wave] = s;
  // the ballots do not need the sum: formed before the barrier, they are 16 SGPRs across it
  uint64_t mask[kRounds][4];
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
#pragma unroll
    for (int c = 0; c < 4; ++c) mask[h][c] = __builtin_amdgcn_ballot_w64((bits_of(m[h].v[c]) >> 31) != 0u);
  }
  block_barrier();
  double S = 0.0;
#pragma unroll
  for (int w = 0; w < 4; ++w) S += ws[w];
  const float sc = (float)(S / (double)len);
  const unsigned mag = bits_of(sc) & 0x7fffffffu;
  if (lane == 0) {
#pragma unroll
    for (int h = 0; h < kRounds; ++h) {
      sign_u32x4* dst = reinterpret_cast<sign_u32x4*>(out + (size_t)j * (kSignBlock / 32) + 8 * (4 * h + wave));
#pragma unroll
      for (int c = 0; c < 4; c += 2) {
        sign_u32x4 w4;
        w4[0] = (unsigned)mask[h][c]; w4[1] = (unsigned)(mask[h][c] >> 32);
        w4[2] = (unsigned)mask[h][c + 1]; w4[3] = (unsigned)(mask[h][c + 1] >> 32);
        dst[c >> 1] = w4;
      }
    }
  }
  if (tid == 0) out[(size_t)nb * (kSignBlock / 32) + j] = (int32_t)bits_of(sc);
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float mv = m[h].v[c];
      m[h].v[c] = fsub_scalar(mv, with_sign(mag, bits_of(mv) & 0x80000000u));
    }
    store_quad(eb, h * 4 * kThreads + 4 * tid, m[h]);
  }
}

// one rank's view of a block for one wave: the masks M[h][wave][0 .. 3] as 8 words per round, and
// bits(s_j).  Word loads: a rank's row starts at a multiple of 65 words, so nothing wider is aligned.
struct RankBits {
  unsigned w[kRounds][8];
  unsigned scale;
};

__device__ __forceinline__ RankBits load_rank(const int32_t* __restrict__ row, int nb, int j, int wave) {
  RankBits r;
  const int32_t* signs = row + (size_t)j * (kSignBlock / 32);
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[h][i] = (unsigned)signs[8 * (4 * h + wave) + i];  // wave-uniform
  }
  r.scale = (unsigned)row[(size_t)nb * (kSignBlock / 32) + j];
  return r;
}

// acc = 0;  for r = 0 .. N-1:  acc = fadd(acc, c_r) for the lane's 8 elements of block j: the decode both
// update kernels share.  Rank r + 1's masks and scale are requested before rank r's are consumed.
__device__ __forceinline__ void sign_accumulate(const int32_t* __restrict__ gathered, int nb, int j, int wave,
                                                int lane, int N, float (&acc)[kRounds][4]) {
  const size_t row_words = (size_t)nb * kSignWords;
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[h][c] = 0.f;
  }
  RankBits cur = load_rank(gathered, nb, j, wave);
  for (int r = 0; r < N; ++r) {
    RankBits nxt = cur;
    if (r + 1 < N) nxt = load_rank(gathered + (size_t)(r + 1) * row_words, nb, j, wave);
    const unsigned mag = cur.scale & 0x7fffffffu;
#pragma unroll
    for (int h = 0; h < kRounds; ++h) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint64_t mk = ((uint64_t)cur.w[h][2 * c + 1] << 32) | cur.w[h][2 * c];
        const unsigned bit = (unsigned)(mk >> lane) & 1u;
        acc[h][c] = fadd_scalar(acc[h][c], with_sign(mag, bit << 31));
      }
    }
    cur = nxt;
  }
}

__global__ __launch_bounds__(kThreads) NDP_NO_PACKED_F32 void sign_update_kernel(
    float* __restrict__ x, float* __restrict__ b, const int* __restrict__ table, int nb,
    const int32_t* __restrict__ gathered, int N, float lr_arg, float lam, const float* __restrict__ hyper) {
  const Hyper hy = load_hyper(hyper, lr_arg);
  const int j = blockIdx.x;
  const int off = table[2 * j], len = table[2 * j + 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* __restrict__ xb = x + off;
  float* __restrict__ bb = b + off;
  Quad xq[kRounds], bq[kRounds];
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
    xq[h] = load_quad(xb, h * 4 * kThreads + 4 * tid, len);
    bq[h] = load_quad(bb, h * 4 * kThreads + 4 * tid, len);
  }
  float acc[kRounds][4];
  sign_accumulate(gathered, nb, j, wave, lane, N, acc);
  const float fN = (float)N;
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      xq[h].v[c] = sign_step(acc[h][c], xq[h].v[c], bq[h].v[c], N, fN, hy.lr, hy.wd, lam);
    store_quad(xb, h * 4 * kThreads + 4 * tid, xq[h]);
    store_quad(bb, h * 4 * kThreads + 4 * tid, bq[h]);
  }
}

// sign_update with AdamW behind the decompressed average (ef_block.h: ef_adam_load / ef_adam_tail).
// decays: int32 [nb], whether block j's tensor takes the weight decay.
// Resources (hipcc --offload-arch=gfx950 -O3 -ffp-contract=fast, -Rpass-analysis=kernel-resource-usage):
// 57 VGPRs, 0 AGPRs, 70 SGPRs, no scratch (0 bytes/lane, no spills), 8 B of LDS, occupancy 8 waves/SIMD
// (sign_update_kernel: 36 VGPRs, 60 SGPRs, no LDS, occupancy 8).
__global__ __launch_bounds__(kThreads) NDP_NO_PACKED_F32 void sign_update_adam_kernel(
    float* __restrict__ x, float* __restrict__ m, float* __restrict__ v, const int* __restrict__ table,
    const int* __restrict__ decays, int nb, const int32_t* __restrict__ gathered, int N, float lr_arg,
    const float* __restrict__ hyper, AdamBlock* block, unsigned* ctr, float beta1, float beta2, float eps) {
  __shared__ float pow_sh[2];
  const unsigned steps = adam_block_read(block, pow_sh);
  const Hyper hy = load_hyper(hyper, lr_arg);
  const int j = blockIdx.x;
  const int off = table[2 * j], len = table[2 * j + 1];
  const bool dec = decays[j] != 0;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  EfAdamRegs R = ef_adam_load(x + off, m + off, v + off, tid, len);
  float acc[kRounds][4];
  sign_accumulate(gathered, nb, j, wave, lane, N, acc);
  ef_adam_tail(x + off, m + off, v + off, tid, R, acc, N, hy, dec, pow_sh, beta1, beta2, eps, ctr, block, steps);
}

}  // namespace

void launch_sign_update_adam(float* x, float* m, float* v, int64_t n, const int32_t* table, const int32_t* decays,
                             int64_t nb, const int32_t* gathered, int world, float lr, const float* hyper,
                             EfAdamArgs a, hipStream_t s) {
  if (n <= 0 || n >= (1LL << 31) || nb < 1 || world < 1) return;  // the binding has refused these
  hipLaunchKernelGGL(sign_update_adam_kernel, dim3((unsigned)nb), dim3(kThreads), 0, s, x, m, v, table, decays,
                     (int)nb, gathered, world, lr, hyper, a.block, a.ctr, a.beta1, a.beta2, a.eps);
}

void launch_sign_pack(const float* g, float* e, int64_t n, const int32_t* table, int64_t nb, int32_t* out,
                      hipStream_t s) {
  if (n <= 0 || n >= (1LL << 31) || nb < 1) return;  // the binding has refused these
  hipLaunchKernelGGL(sign_pack_kernel, dim3((unsigned)nb), dim3(kThreads), 0, s, g, e, table, (int)nb, out);
}

void launch_sign_update(float* x, float* b, int64_t n, const int32_t* table, int64_t nb, const int32_t* gathered,
                        int world, float lr, float lam, const float* hyper, hipStream_t s) {
  if (n <= 0 || n >= (1LL << 31) || nb < 1 || world < 1) return;
  hipLaunchKernelGGL(sign_update_kernel, dim3((unsigned)nb), dim3(kThreads), 0, s, x, b, table, (int)nb, gathered,
                     world, lr, lam, hyper);
}

}  // namespace ndp
