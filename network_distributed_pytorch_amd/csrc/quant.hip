// Block-quantised gradient compression with error feedback (QSGD / TernGrad style, deterministic
// rounding) over flat fp32 arenas, exact: BITS = 2, 4 or 8 bits per coordinate of m = g + e plus one
// fp32 scale per block of 2048 elements, and the decompress + momentum + SGD update behind the
// all-gather.  Two launches, one workgroup of 256 threads per block of signsgd.hip's block table, no
// workgroup ever needs another's result: no ticket, no atomic, every store a per-lane vector store of
// 32 bits or wider.
//
// With L = 2^(BITS-1) - 1 (1, 7, 127) and W = 64 BITS code words per block:
//   A_j = max over the block of bits(m) & 0x7fffffff, as unsigned integers (the exact absmax, whatever
//         the order; absent elements count as 0)
//   s_j = fdiv(A_j, (float)L)
//   live block (A_j < 0x7f800000 and s_j != 0):  q = min(max(rint(fdiv(m, s_j)), -L), L) as a float
//         (rint(-0.3) = -0 stays -0),  c = fmul(q, s_j),  e' = fsub(m, c),  code u = (int)q + L
//   dead block (s_j == 0: a zero block, or A_j / L underflows):  code bits 0, scale word 0, e' = m
//   non-finite block (A_j >= 0x7f800000):  code bits 0, scale word 0x7fc00000, every e' stored as the
//         bit pattern 0x7fc00000 (a select, not an arithmetic result)
// Row of a rank, int32 [row_words]: nb * W code words, nb scale words, zero padding to a multiple of 4.
// Element t of block j is the little-endian bit field [(t BITS) & 31, +BITS) of word W j + ((t BITS) >> 5);
// bits of absent elements are 0.
//
// Thread map: the sign kernels' (ef_block.h), t = 1024 h + 4 tid + c.  It keeps every g / e / x / b
// access a fully coalesced float4 (8 consecutive elements per thread would stride them by 32 B), and
// a thread's quad of a round is the 4 BITS-bit field at bit 4 BITS (tid mod 8 / BITS) of word
// 32 BITS h + (tid BITS >> 3) of its block.  What that costs is a cross-lane merge below 8 bits, and
// it is arranged so that no lane idles at the store:
//   8 bits: the quad is a word; every lane stores both of its rounds' words.
//   4 bits: a lane pair holds two half-words per round.  One quad_perm DPP move swaps what the partner
//           needs: the even lane ends with round 0's word, the odd lane with round 1's; 256 stores.
//   2 bits: a lane quad holds four bytes per round.  Two DPP moves (lane ^ 1 on 16 bits, lane ^ 2 on
//           32) leave all 8 bytes in every lane; lane 0 of the quad stores round 0's word, lane 1
//           round 1's.
// All 256 lanes run the cross-lane moves (a ragged block masks codes, not lanes).
//
// quant_pack:  m stays in 8 registers per thread across the one barrier; both arenas' float4 loads are
//   in flight before the first use.  Absmax: 8 integer maxima per lane, in the wave two quad_perm and
//   two row-mirror DPP moves and two ds_bpermute (every lane ends with the wave's maximum), across the
//   4 waves 4 words of LDS.  Block 0 also clears the row's padding words.
//
// quant_update:  the x / b quads are in flight first.  gathered is int32 [N][row_words].  Rank after
//   rank a lane reads its own two code words with vector loads and the block's scale with a uniform
//   (scalar) load, rank r + 1's requested before rank r's are consumed; decode is shift, mask, convert:
//     acc = 0;  for r = 0 .. N-1:  acc = fadd(acc, fmul((float)(u_r - L), s_r))     (rank order)
//   then sign_step (ef_block.h): o = acc / N when N != 1, decay, momentum, SGD.  No LDS.
//
// quant_update_adam:  the same loads and decode (quant_accumulate), then AdamW (adamw_elem.h) on o in the
//   place of sign_step; b is the first moment, a third arena the second.  It alone has a barrier, 8 bytes
//   of LDS and a ticket: the AdamBlock protocol of adam_block.h (ef_block.h: ef_adam_tail).
//
// The rule's adds and subtractions are single scalar instructions and both kernels are compiled
// without packed fp32 operations, as in signsgd.hip; every product feeds such an instruction, so the
// build's -ffp-contract=fast has nothing to fuse it with.
#include <hip/hip_runtime.h>

#include "ef_block.h"
#include "hyper.h"
#include "ndp_kernels.h"

namespace ndp {

namespace {

constexpr int kThreads = 256;
constexpr int kRounds = kSignBlock / (4 * kThreads);  // float4 rounds per thread and block
static_assert(kRounds == 2, "thread map and wire layout");
static_assert(kRounds == kEfRounds && kThreads == kEfThreads, "ef_block.h's AdamW pieces use the same thread map");
constexpr unsigned kInfBits = 0x7f800000u, kNanBits = 0x7fc00000u;

// DPP controls: quad_perm [1,0,3,2] (lane ^ 1), quad_perm [2,3,0,1] (lane ^ 2), and the mirrors of
// 8 and of 16 lanes, which pair quad with quad and half-row with half-row once the quads agree
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140;

template <int CTRL>
__device__ __forceinline__ unsigned dpp(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}

__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

// the maximum over the wave, in every lane
__device__ __forceinline__ unsigned wave_umax(unsigned a, int lane) {
  a = umax(a, dpp<kDppXor1>(a));
  a = umax(a, dpp<kDppXor2>(a));
  a = umax(a, dpp<kDppHalfMirror>(a));
  a = umax(a, dpp<kDppMirror>(a));
  a = umax(a, (unsigned)__builtin_amdgcn_ds_bpermute((lane ^ 16) << 2, (int)a));
  a = umax(a, (unsigned)__builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, (int)a));
  return a;
}

template <int BITS>
__global__ __launch_bounds__(kThreads) NDP_NO_PACKED_F32 void quant_pack_kernel(const float* __restrict__ g,
                                                                                float* __restrict__ e,
                                                                                const int* __restrict__ table, int nb,
                                                                                int32_t* __restrict__ out) {
  constexpr int L = (1 << (BITS - 1)) - 1, W = 64 * BITS;
  __shared__ unsigned wa[4];
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
  unsigned a = 0u;
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      m[h].v[c] = fadd_scalar(gq[h].v[c], m[h].v[c]);
      a = umax(a, bits_of(m[h].v[c]) & 0x7fffffffu);
    }
  }
  a = wave_umax(a, lane);
  if (lane == 0) wa[wave] = a;
  block_barrier();
  const unsigned A = umax(umax(wa[0], wa[1]), umax(wa[2], wa[3]));
  const float s = __fdiv_rn(__builtin_bit_cast(float, A), (float)L);
  const bool finite = A < kInfBits, live = finite && s != 0.f;
  unsigned p[kRounds];  // a round's four codes, 4 BITS bits
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
    p[h] = 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float mv = m[h].v[c];
      float q = __builtin_rintf(__fdiv_rn(mv, s));  // v_rndne_f32: half to even
      q = __builtin_fminf(__builtin_fmaxf(q, (float)-L), (float)L);
      const float ev = fsub_scalar(mv, __fmul_rn(q, s));
      const unsigned u = (live && c < m[h].nv) ? (unsigned)((int)q + L) : 0u;
      p[h] |= u << (BITS * c);
      m[h].v[c] = live ? ev : (finite ? mv : __builtin_bit_cast(float, kNanBits));
    }
  }
  int32_t* __restrict__ codes = out + (size_t)j * W;
  if constexpr (BITS == 8) {
#pragma unroll
    for (int h = 0; h < kRounds; ++h) codes[256 * h + tid] = (int32_t)p[h];
  } else if constexpr (BITS == 4) {
    const bool odd = (tid & 1) != 0;
    const unsigned got = dpp<kDppXor1>(odd ? p[0] : p[1]);  // the partner's half of this lane's word
    codes[(odd ? 128 : 0) + (tid >> 1)] = (int32_t)(odd ? (got | (p[1] << 16)) : (p[0] | (got << 16)));
  } else {
    const unsigned mine = p[0] | (p[1] << 8);                     // [round 0, round 1] of this lane
    const unsigned got = dpp<kDppXor1>(mine);
    const unsigned pair = (tid & 1) ? (got | (mine << 16)) : (mine | (got << 16));  // even lane's, odd lane's
    const unsigned other = dpp<kDppXor2>(pair);
    // lanes 0 and 1 of the quad store: their own pair is the quad's low one
    const unsigned sh = (tid & 1) ? 8u : 0u;
    const unsigned word = ((pair >> sh) & 0xffu) | (((pair >> (16 + sh)) & 0xffu) << 8) |
                          (((other >> sh) & 0xffu) << 16) | (((other >> (16 + sh)) & 0xffu) << 24);
    if ((tid & 2) == 0) codes[((tid & 1) ? 64 : 0) + (tid >> 2)] = (int32_t)word;
  }
  const size_t tail = (size_t)nb * W;
  if (tid == 0) out[tail + j] = (int32_t)(live ? bits_of(s) : (finite ? 0u : kNanBits));
  if (j == 0 && tid < (int)(quant_row_words(nb, BITS) - (int64_t)nb * (W + 1))) out[tail + nb + tid] = 0;
#pragma unroll
  for (int h = 0; h < kRounds; ++h) store_quad(eb, h * 4 * kThreads + 4 * tid, m[h]);
}

// one rank's view of a block for one lane: the word holding its quad of each round, and bits(s_j)
struct RankCodes {
  unsigned w[kRounds];
  unsigned scale;
};

// codes: the lane's first code word of the block in rank 0's row; scales: the block's scale word there
template <int BITS>
__device__ __forceinline__ RankCodes load_rank(const int32_t* __restrict__ codes, const int32_t* __restrict__ scales,
                                               size_t row) {
  RankCodes r;
#pragma unroll
  for (int h = 0; h < kRounds; ++h) r.w[h] = (unsigned)codes[row + 32 * BITS * h];  // per lane: vector loads
  // uniform: a scalar load (the row offset is pinned to SGPRs; the compiler would otherwise fold this
  // address into the lanes' code pointer and load the scale per lane)
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)row);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(row >> 32));
  r.scale = (unsigned)scales[((size_t)hi << 32) | lo];
  return r;
}

// acc = 0;  for r = 0 .. N-1:  acc = fadd(acc, fmul((float)(u_r - L), s_r)) for the lane's 8 elements of
// block j: the decode both update kernels share.  Rank r + 1's words are requested before rank r's are
// consumed.
template <int BITS>
__device__ __forceinline__ void quant_accumulate(const int32_t* __restrict__ gathered, int nb, int j, int tid, int N,
                                                 float (&acc)[kRounds][4]) {
  constexpr int L = (1 << (BITS - 1)) - 1;
  const size_t row_words = (size_t)quant_row_words(nb, BITS);
  const unsigned shift = (unsigned)(4 * BITS * tid) & 31u;  // the quad's place in its word
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[h][c] = 0.f;
  }
  const int32_t* __restrict__ codes = gathered + (size_t)j * (64 * BITS) + ((tid * BITS) >> 3);
  const int32_t* __restrict__ scales = gathered + (size_t)nb * (64 * BITS) + j;
  RankCodes cur = load_rank<BITS>(codes, scales, 0);
  for (int r = 0; r < N; ++r) {
    RankCodes nxt = cur;
    if (r + 1 < N) nxt = load_rank<BITS>(codes, scales, (size_t)(r + 1) * row_words);
    const float sc = __builtin_bit_cast(float, cur.scale);
#pragma unroll
    for (int h = 0; h < kRounds; ++h) {
      const unsigned field = cur.w[h] >> shift;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int u = (int)((field >> (BITS * c)) & ((1u << BITS) - 1u));
        acc[h][c] = fadd_scalar(acc[h][c], __fmul_rn((float)(u - L), sc));
      }
    }
    cur = nxt;
  }
}

template <int BITS>
__global__ __launch_bounds__(kThreads) NDP_NO_PACKED_F32 void quant_update_kernel(
    float* __restrict__ x, float* __restrict__ b, const int* __restrict__ table, int nb,
    const int32_t* __restrict__ gathered, int N, float lr_arg, float lam, const float* __restrict__ hyper) {
  const Hyper hy = load_hyper(hyper, lr_arg);
  const int j = blockIdx.x;
  const int off = table[2 * j], len = table[2 * j + 1];
  const int tid = threadIdx.x;
  float* __restrict__ xb = x + off;
  float* __restrict__ bb = b + off;
  Quad xq[kRounds], bq[kRounds];
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
    xq[h] = load_quad(xb, h * 4 * kThreads + 4 * tid, len);
    bq[h] = load_quad(bb, h * 4 * kThreads + 4 * tid, len);
  }
  float acc[kRounds][4];
  quant_accumulate<BITS>(gathered, nb, j, tid, N, acc);
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

// quant_update with AdamW behind the decoded average (ef_block.h: ef_adam_load / ef_adam_tail).
// decays: int32 [nb], whether block j's tensor takes the weight decay.
// Resources (hipcc --offload-arch=gfx950 -O3 -ffp-contract=fast, -Rpass-analysis=kernel-resource-usage), the
// same at 2, 4 and 8 bits: 57 VGPRs, 0 AGPRs, 46 SGPRs, no scratch (0 bytes/lane, no spills), 8 B of LDS,
// occupancy 8 waves/SIMD (quant_update_kernel: 38-39 VGPRs, 32-34 SGPRs, no LDS, occupancy 8).
template <int BITS>
__global__ __launch_bounds__(kThreads) NDP_NO_PACKED_F32 void quant_update_adam_kernel(
    float* __restrict__ x, float* __restrict__ m, float* __restrict__ v, const int* __restrict__ table,
    const int* __restrict__ decays, int nb, const int32_t* __restrict__ gathered, int N, float lr_arg,
    const float* __restrict__ hyper, AdamBlock* block, unsigned* ctr, float beta1, float beta2, float eps) {
  __shared__ float pow_sh[2];
  const unsigned steps = adam_block_read(block, pow_sh);
  const Hyper hy = load_hyper(hyper, lr_arg);
  const int j = blockIdx.x;
  const int off = table[2 * j], len = table[2 * j + 1];
  const bool dec = decays[j] != 0;
  const int tid = threadIdx.x;
  EfAdamRegs R = ef_adam_load(x + off, m + off, v + off, tid, len);
  float acc[kRounds][4];
  quant_accumulate<BITS>(gathered, nb, j, tid, N, acc);
  ef_adam_tail(x + off, m + off, v + off, tid, R, acc, N, hy, dec, pow_sh, beta1, beta2, eps, ctr, block, steps);
}

template <int BITS>
void launch_update_adam(float* x, float* m, float* v, const int32_t* table, const int32_t* decays, int nb,
                        const int32_t* gathered, int world, float lr, const float* hyper, EfAdamArgs a, hipStream_t s) {
  hipLaunchKernelGGL(quant_update_adam_kernel<BITS>, dim3((unsigned)nb), dim3(kThreads), 0, s, x, m, v, table, decays,
                     nb, gathered, world, lr, hyper, a.block, a.ctr, a.beta1, a.beta2, a.eps);
}

}  // namespace

void launch_quant_update_adam(float* x, float* m, float* v, int64_t n, const int32_t* table, const int32_t* decays,
                              int64_t nb, int bits, const int32_t* gathered, int world, float lr, const float* hyper,
                              EfAdamArgs a, hipStream_t s) {
  if (n <= 0 || n >= (1LL << 31) || nb < 1 || world < 1) return;  // the binding has refused these
  if (bits == 2) launch_update_adam<2>(x, m, v, table, decays, (int)nb, gathered, world, lr, hyper, a, s);
  if (bits == 4) launch_update_adam<4>(x, m, v, table, decays, (int)nb, gathered, world, lr, hyper, a, s);
  if (bits == 8) launch_update_adam<8>(x, m, v, table, decays, (int)nb, gathered, world, lr, hyper, a, s);
}

void launch_quant_pack(const float* g, float* e, int64_t n, const int32_t* table, int64_t nb, int bits, int32_t* out,
                       hipStream_t s) {
  if (n <= 0 || n >= (1LL << 31) || nb < 1) return;  // the binding has refused these
  const dim3 grid((unsigned)nb), block(kThreads);
  if (bits == 2) hipLaunchKernelGGL(quant_pack_kernel<2>, grid, block, 0, s, g, e, table, (int)nb, out);
  if (bits == 4) hipLaunchKernelGGL(quant_pack_kernel<4>, grid, block, 0, s, g, e, table, (int)nb, out);
  if (bits == 8) hipLaunchKernelGGL(quant_pack_kernel<8>, grid, block, 0, s, g, e, table, (int)nb, out);
}

void launch_quant_update(float* x, float* b, int64_t n, const int32_t* table, int64_t nb, int bits,
                         const int32_t* gathered, int world, float lr, float lam, const float* hyper, hipStream_t s) {
  if (n <= 0 || n >= (1LL << 31) || nb < 1 || world < 1) return;
  const dim3 grid((unsigned)nb), block(kThreads);
  if (bits == 2)
    hipLaunchKernelGGL(quant_update_kernel<2>, grid, block, 0, s, x, b, table, (int)nb, gathered, world, lr, lam, hyper);
  if (bits == 4)
    hipLaunchKernelGGL(quant_update_kernel<4>, grid, block, 0, s, x, b, table, (int)nb, gathered, world, lr, lam, hyper);
  if (bits == 8)
    hipLaunchKernelGGL(quant_update_kernel<8>, grid, block, 0, s, x, b, table, (int)nb, gathered, world, lr, lam, hyper);
}

}  // namespace ndp
