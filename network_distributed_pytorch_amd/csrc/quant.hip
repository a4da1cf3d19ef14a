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
// Randomized Hadamard rotation (the ROT = true instances; ROT = false is the code above, unchanged).  A block
// is rotated iff len_j == 2048 (uniform per workgroup: the barrier below is taken by all 256 threads or by
// none); a ragged block follows the plain rule.  For a rotated block:
//   d_t = -1 iff bit t & 31 of counter_hash4(seed, j, t >> 5, TAG) is set, TAG = 0x48414452 ("HADR"); applying
//         d_t flips the float's sign bit.  A lane needs two hashes, one per round: word 32 h + (tid >> 3),
//         bits 4 (tid & 7) + c.
//   W:    11 butterfly stages k = 0 .. 10 in that order; in stage k every pair (t, t | 2^k) with bit k of t
//         clear becomes (fadd(a, b), fsub(a, b)), one IEEE fp32 operation each.  The natural-order Sylvester
//         Hadamard matrix H[t][u] = (-1)^popcount(t & u), unnormalised: W(W(v)) = 2048 v.
//   pack:   m = fadd(W(d o g), e): e of a rotated block lives in the rotated domain; everything behind m is
//           the plain body (an overflow in the butterflies makes the block non-finite like an inf in g).
//   update: acc as above, then a_t = d_t fmul(W(acc)_t, 2^-11) in the place of acc: one transform per block,
//           not per rank, W being linear.
// fwht2048 works on the 8 registers a thread holds, t = 1024 h + 4 tid + c = [h | wave(2) | lane(6) | c(2)]:
//   stages 0-1 (c):    in registers.
//   stages 2-7 (lane): the partner's value by quad_perm DPP (^1, ^2), ds_swizzle (^4), row_ror:8 DPP (^8) and
//                      the gfx950 v_permlane16_swap / v_permlane32_swap (^16, ^32): no LDS round trip and no
//                      address register, where ds_bpermute needs both.  The lane whose bit is clear forms
//                      v + p, the other p - v; the latter is formed as fadd(p, -v), the same float, so one
//                      v_add_f32 behind a sign-bit XOR (folded into v_bitop3 with the mask) serves both.
//   stages 8-9 (wave): one 8 KB exchange and one barrier: every thread leaves its 8 values as two float4,
//                      reads the other three waves' and forms stage 8 of its own pair and of the pair across,
//                      then stage 9, with wave-uniform sign masks.
//   stage 10 (h):      in registers.
// The pack transforms g in front of m = g + e, all four quad loads requested first as in the plain kernel;
// the update transforms between quant_accumulate and the step.
//
// The rule's adds and subtractions are single scalar instructions and both kernels are compiled
// without packed fp32 operations, as in signsgd.hip; every product feeds such an instruction, so the
// build's -ffp-contract=fast has nothing to fuse it with.
#include <hip/hip_runtime.h>

#include "counter_hash.h"
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

// ---- the rotation of the ROT instances ---------------------------------------------------------------
constexpr uint32_t kRotTag = 0x48414452u;  // "HADR": the fourth argument of the sign hash
constexpr int kDppRor8 = 0x128;            // row_ror:8, lane ^ 8 within a row of 16
constexpr int kSwizzleXor4 = 0x101F;       // ds_swizzle bit mode: and 0x1f, or 0, xor 4

__device__ __forceinline__ float flip(float v, unsigned mask) { return __builtin_bit_cast(float, bits_of(v) ^ mask); }

// the lane's sign bits of round h, bit c the sign of component c
__device__ __forceinline__ void rot_signs(unsigned seed, int j, int tid, unsigned (&sg)[kRounds]) {
#pragma unroll
  for (int h = 0; h < kRounds; ++h)
    sg[h] = counter_hash4(seed, (uint32_t)j, (uint32_t)(32 * h + (tid >> 3)), kRotTag) >> (4 * (tid & 7));
}
__device__ __forceinline__ float rot_sign(float v, unsigned sg, int c) {
  return flip(v, (sg << (31 - c)) & 0x80000000u);
}

// One butterfly stage across lanes (or waves) on a value: neg is the sign bit where this lane holds the
// pair's high element, 0 where it holds the low one.  Low: fadd(own, partner).  High: fsub(partner, own),
// formed as fadd(partner, -own): the same float, so one instruction serves both.
__device__ __forceinline__ float lane_stage(float own, float partner, unsigned neg) {
  return fadd_scalar(partner, flip(own, neg));
}

// Stage lane ^ 16 (ROWS = 16) or lane ^ 32 by v_permlane16_swap / v_permlane32_swap on two copies of x: the
// instruction swaps the odd rows (the upper half) of its first operand with the even rows (the lower half)
// of its second, so afterwards a holds the pair's low element and b its high one in every lane.  Written
// as assembly with two registers of its own: given the same value twice, the compiler's builtin took
// both results from one register.  The s_nop covers the VALU write of the copies before the swap reads them.
template <int ROWS>
__device__ __forceinline__ float swap_stage(float x, unsigned neg) {
  float a = x, b = x;
  if constexpr (ROWS == 16)
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  else
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return fadd_scalar(a, flip(b, neg));
}

// W of the header over the block, v[h][c] the element t = 1024 h + 4 tid + c: in place, unnormalised,
// stage k pairing t with t | 2^k in the order k = 0 .. 10.  xch: 8 KB of LDS, [wave][h][lane] float4.
// All 256 threads of the workgroup call it (one barrier).
__device__ __forceinline__ void fwht2048(float (&v)[kRounds][4], int lane, int wave, sign_f32x4* xch) {
  // stages 0, 1: the quad's components
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
    const float a0 = fadd_scalar(v[h][0], v[h][1]), a1 = fsub_scalar(v[h][0], v[h][1]);
    const float a2 = fadd_scalar(v[h][2], v[h][3]), a3 = fsub_scalar(v[h][2], v[h][3]);
    v[h][0] = fadd_scalar(a0, a2); v[h][2] = fsub_scalar(a0, a2);
    v[h][1] = fadd_scalar(a1, a3); v[h][3] = fsub_scalar(a1, a3);
  }
  // stages 2 .. 7: lane ^ 1, 2 (quad_perm), 4 (ds_swizzle), 8 (row rotate), 16, 32 (row / half swaps)
  const unsigned ul = (unsigned)lane;
  const unsigned n1 = (ul << 31), n2 = (ul << 30) & 0x80000000u, n4 = (ul << 29) & 0x80000000u,
                 n8 = (ul << 28) & 0x80000000u, n16 = (ul << 27) & 0x80000000u, n32 = (ul << 26) & 0x80000000u;
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float x = v[h][c];
      x = lane_stage(x, __builtin_bit_cast(float, dpp<kDppXor1>(bits_of(x))), n1);
      x = lane_stage(x, __builtin_bit_cast(float, dpp<kDppXor2>(bits_of(x))), n2);
      x = lane_stage(x, __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_ds_swizzle((int)bits_of(x), kSwizzleXor4)),
                     n4);
      x = lane_stage(x, __builtin_bit_cast(float, dpp<kDppRor8>(bits_of(x))), n8);
      x = swap_stage<16>(x, n16);
      x = swap_stage<32>(x, n32);
      v[h][c] = x;
    }
  }
  // stages 8, 9: the wave.  One exchange: every thread leaves its 8 values, reads the other three
  // waves' and forms stage 8 of its own pair and of the pair across, then stage 9
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
    sign_f32x4 t;
    t[0] = v[h][0]; t[1] = v[h][1]; t[2] = v[h][2]; t[3] = v[h][3];
    xch[(wave * kRounds + h) * 64 + lane] = t;
  }
  block_barrier();
  const unsigned w0 = ((unsigned)wave & 1u) << 31, w1 = ((unsigned)wave & 2u) << 30;  // uniform
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
    const sign_f32x4 x1 = xch[((wave ^ 1) * kRounds + h) * 64 + lane];
    const sign_f32x4 x2 = xch[((wave ^ 2) * kRounds + h) * 64 + lane];
    const sign_f32x4 x3 = xch[((wave ^ 3) * kRounds + h) * 64 + lane];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float mine = lane_stage(v[h][c], x1[c], w0);  // stage 8 of wave, wave ^ 1
      const float across = lane_stage(x2[c], x3[c], w0);  // stage 8 of wave ^ 2, wave ^ 3
      v[h][c] = lane_stage(mine, across, w1);
    }
  }
  // stage 10: the round
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float a = v[0][c], b = v[1][c];
    v[0][c] = fadd_scalar(a, b);
    v[1][c] = fsub_scalar(a, b);
  }
}

// the update's way back: acc (a rank-ordered sum in the rotated domain) becomes d o (W(acc) 2^-11)
__device__ __forceinline__ void rot_inverse(float (&acc)[kRounds][4], unsigned seed, int j, int tid, sign_f32x4* xch) {
  unsigned sg[kRounds];
  rot_signs(seed, j, tid, sg);
  fwht2048(acc, tid & 63, __builtin_amdgcn_readfirstlane(tid >> 6), xch);
#pragma unroll
  for (int h = 0; h < kRounds; ++h) {
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[h][c] = rot_sign(__fmul_rn(acc[h][c], 0x1p-11f), sg[h], c);
  }
}

template <int BITS, bool ROT>
__global__ __launch_bounds__(kThreads) NDP_NO_PACKED_F32 void quant_pack_kernel(const float* __restrict__ g,
                                                                                float* __restrict__ e,
                                                                                const int* __restrict__ table, int nb,
                                                                                int32_t* __restrict__ out,
                                                                                unsigned seed) {
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
  if constexpr (ROT) {
    __shared__ sign_f32x4 xch[4 * kRounds * 64];
    if (len == kSignBlock) {  // uniform: a full block is rotated, g becomes y = W(d o g)
      unsigned sg[kRounds];
      rot_signs(seed, j, tid, sg);
      float y[kRounds][4];
#pragma unroll
      for (int h = 0; h < kRounds; ++h) {
#pragma unroll
        for (int c = 0; c < 4; ++c) y[h][c] = rot_sign(gq[h].v[c], sg[h], c);
      }
      fwht2048(y, lane, wave, xch);
#pragma unroll
      for (int h = 0; h < kRounds; ++h) {
#pragma unroll
        for (int c = 0; c < 4; ++c) gq[h].v[c] = y[h][c];
      }
    }
  }
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

template <int BITS, bool ROT>
__global__ __launch_bounds__(kThreads) NDP_NO_PACKED_F32 void quant_update_kernel(
    float* __restrict__ x, float* __restrict__ b, const int* __restrict__ table, int nb,
    const int32_t* __restrict__ gathered, int N, float lr_arg, float lam, const float* __restrict__ hyper,
    unsigned seed) {
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
  if constexpr (ROT) {
    __shared__ sign_f32x4 xch[4 * kRounds * 64];
    if (len == kSignBlock) rot_inverse(acc, seed, j, tid, xch);  // uniform: all 256 threads or none
  }
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
// ROT instances (the same report; no spills, no scratch in any): quant_pack_kernel 50 VGPRs, 39 SGPRs, 8208 B of
// LDS, occupancy 8 (ROT = false: 30 VGPRs, 39 SGPRs, 16 B); quant_update_kernel 62 / 62 / 64 VGPRs at 2 / 4 / 8
// bits, 38 SGPRs, 8192 B, occupancy 8; quant_update_adam_kernel 76 VGPRs, 48 SGPRs, 8208 B, occupancy 6.
template <int BITS, bool ROT>
__global__ __launch_bounds__(kThreads) NDP_NO_PACKED_F32 void quant_update_adam_kernel(
    float* __restrict__ x, float* __restrict__ m, float* __restrict__ v, const int* __restrict__ table,
    const int* __restrict__ decays, int nb, const int32_t* __restrict__ gathered, int N, float lr_arg,
    const float* __restrict__ hyper, AdamBlock* block, unsigned* ctr, float beta1, float beta2, float eps,
    unsigned seed) {
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
  if constexpr (ROT) {
    __shared__ sign_f32x4 xch[4 * kRounds * 64];
    if (len == kSignBlock) rot_inverse(acc, seed, j, tid, xch);  // uniform
  }
  ef_adam_tail(x + off, m + off, v + off, tid, R, acc, N, hy, dec, pow_sh, beta1, beta2, eps, ctr, block, steps);
}

// the launch of KERNEL<bits, rotate> (bits in {2, 4, 8}; another value launches nothing)
#define NDP_QUANT_LAUNCH(KERNEL, bits, rotate, grid, s, ...)                                              \
  do {                                                                                                    \
    if ((bits) == 2 && !(rotate)) hipLaunchKernelGGL((KERNEL<2, false>), grid, dim3(kThreads), 0, s, __VA_ARGS__); \
    if ((bits) == 4 && !(rotate)) hipLaunchKernelGGL((KERNEL<4, false>), grid, dim3(kThreads), 0, s, __VA_ARGS__); \
    if ((bits) == 8 && !(rotate)) hipLaunchKernelGGL((KERNEL<8, false>), grid, dim3(kThreads), 0, s, __VA_ARGS__); \
    if ((bits) == 2 && (rotate)) hipLaunchKernelGGL((KERNEL<2, true>), grid, dim3(kThreads), 0, s, __VA_ARGS__);   \
    if ((bits) == 4 && (rotate)) hipLaunchKernelGGL((KERNEL<4, true>), grid, dim3(kThreads), 0, s, __VA_ARGS__);   \
    if ((bits) == 8 && (rotate)) hipLaunchKernelGGL((KERNEL<8, true>), grid, dim3(kThreads), 0, s, __VA_ARGS__);   \
  } while (0)

}  // namespace

void launch_quant_update_adam(float* x, float* m, float* v, int64_t n, const int32_t* table, const int32_t* decays,
                              int64_t nb, int bits, const int32_t* gathered, int world, float lr, const float* hyper,
                              EfAdamArgs a, bool rotate, uint32_t seed, hipStream_t s) {
  if (n <= 0 || n >= (1LL << 31) || nb < 1 || world < 1) return;  // the binding has refused these
  NDP_QUANT_LAUNCH(quant_update_adam_kernel, bits, rotate, dim3((unsigned)nb), s, x, m, v, table, decays, (int)nb,
                   gathered, world, lr, hyper, a.block, a.ctr, a.beta1, a.beta2, a.eps, seed);
}

void launch_quant_pack(const float* g, float* e, int64_t n, const int32_t* table, int64_t nb, int bits, int32_t* out,
                       bool rotate, uint32_t seed, hipStream_t s) {
  if (n <= 0 || n >= (1LL << 31) || nb < 1) return;  // the binding has refused these
  NDP_QUANT_LAUNCH(quant_pack_kernel, bits, rotate, dim3((unsigned)nb), s, g, e, table, (int)nb, out, seed);
}

void launch_quant_update(float* x, float* b, int64_t n, const int32_t* table, int64_t nb, int bits,
                         const int32_t* gathered, int world, float lr, float lam, const float* hyper, bool rotate,
                         uint32_t seed, hipStream_t s) {
  if (n <= 0 || n >= (1LL << 31) || nb < 1 || world < 1) return;
  NDP_QUANT_LAUNCH(quant_update_kernel, bits, rotate, dim3((unsigned)nb), s, x, b, table, (int)nb, gathered, world, lr,
                   lam, hyper, seed);
}

}  // namespace ndp
