// Top-k gradient sparsification with error feedback over flat fp32 arenas of n elements, exact:
// the k entries of m = g + e with the largest magnitude keys (ties to the lowest index), in
// ascending index order, and the owner-computes decompress + momentum + SGD update behind the
// all-gather.  Six launches, none of which ever waits for another workgroup (arrival.h tickets),
// no floating-point atomic, every store a plain vector store.
//
//   key_i = bits(m_i) & 0x7fffffff      (31 bits: NaN above inf, -0 == +0 == 0)
//   T     = the k-th largest key with multiplicity,  c = #{key > T}
//   selected: key > T, and the first k - c indices with key == T
//
// Select: a workgroup of 256 threads streams one chunk of kTopkChunk = 8192 consecutive elements,
// 8 float4 per thread, every load in flight before the first use (thread t, round q: elements
// chunk + 1024 q + 4 t .. + 3; a quad that crosses n falls back to scalar loads).
//
//   topk_pass<0,1,2>  radix select of T over the key digits 11 + 11 + 9 bits, from the top.  Pass 0
//        forms m = g + e and stores it into e; passes 1 and 2 read e and keep only the keys whose
//        higher digits equal the prefix found so far.  The digit is histogrammed in LDS
//        (ds_add_u32, <= 2048 bins) and the non-empty bins are flushed with integer atomics into
//        the global histogram.  The last arriver reads the histogram from the top (thread t owns
//        the bins [B - per (t + 1), B - per t), per = B / 256; an exclusive prefix over the threads
//        is the count above its bins), finds the digit d with  above(d) < krem <= above(d) + H[d],
//        writes {prefix = prefix << bits | d, krem -= above(d)} into the TopkBlock, clears the
//        histogram and re-arms the ticket.  After pass 2: T = prefix, ties = krem, c = k - ties.
//   topk_count  #{key > T} and #{key == T} per chunk; the last arriver turns the per-chunk counts
//        into exclusive offsets in chunk order (thread t sums a run of ceil(grid / 256) consecutive
//        chunks, one workgroup scan over the 256 runs, then the run is walked again).
//   topk_compact  re-reads the chunk and ranks its elements in index order: per round and
//        component a wave ballot, the lane's prefix by popcount below the lane (mbcnt), the wave
//        totals through LDS (one barrier).  With gr / er the number of key > T / key == T
//        elements of the chunk before an element, and left = max(ties - eq_off[chunk], 0):
//            selected = key > T  or  (key == T and er < left)
//            pos      = gt_off[chunk] + min(eq_off[chunk], ties) + gr + min(er, left)
//        out[pos] = index, out[k + pos] = bits(m), e[index] = 0.  Ascending by construction.
//
// Measured (profiles/topk): pass 0, pass 2 and the update stream at the PowerSGD P pass's rate or
// above; pass 1 is the slow launch (its survivors spread over all 2048 bins of every workgroup).
//
// Update (topk_update): a workgroup owns a tile of kTopkTile = 2048 consecutive elements and an fp32
// LDS tile acc = 0.  gathered is [N][2k] int32, rank r's row = idx (ascending) | bits(val).  Two
// threads per rank binary-search the row for the tile's bounds (all ranks of a round of 128 at
// once, so the dependent-load latency is paid once, and behind the x / b loads already in flight);
// then rank after rank, a barrier between two, the row's entries of the tile are added into acc
// (indices are unique within a rank: no conflict; rank order: bitwise reproducible).  Then
//     o  = (N != 1) ? acc / N : acc                       (IEEE division)
//     d  = (wd != 0) ? fmaf(wd, x, o) : o
//     b' = fadd(fmul(b, lambda), d);  up = fadd(d, b');  x' = fmaf(-lr, up, x)
// over the tile's 2048 elements of x and b, 2 float4 per thread.  lr / wd come from the nullable
// hyper block (hyper.h).  A tile without entries still runs the momentum rule.
#include <hip/hip_runtime.h>

#include "adam_block.h"
#include "arrival.h"
#include "hyper.h"
#include "ndp_kernels.h"

namespace ndp {

namespace {

constexpr int kThreads = 256;
constexpr int kRounds = kTopkChunk / (4 * kThreads);  // float4 rounds per thread and chunk
constexpr int kRankRound = 128;                       // ranks whose bounds are searched at once
static_assert(kTopkChunk % (4 * kThreads) == 0 && kTopkTile == 8 * kThreads, "thread maps");

typedef float topk_f32x4 __attribute__((ext_vector_type(4)));

struct Quad {
  float v[4];
  int nv;  // leading valid elements (the rest lie past n)
};

// the 4 elements at i (a multiple of 4; src is 16-byte aligned): one float4, or scalars across n
__device__ __forceinline__ Quad load_quad(const float* __restrict__ src, int64_t i, int64_t n) {
  Quad q = {{0.f, 0.f, 0.f, 0.f}, 0};
  if (i + 4 <= n) {
    const topk_f32x4 t = *reinterpret_cast<const topk_f32x4*>(src + i);
    q.v[0] = t[0]; q.v[1] = t[1]; q.v[2] = t[2]; q.v[3] = t[3];
    q.nv = 4;
  } else if (i < n) {
    q.nv = (int)(n - i);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (j < q.nv) q.v[j] = src[i + j];
  }
  return q;
}

__device__ __forceinline__ void store_quad(float* __restrict__ dst, int64_t i, const Quad& q) {
  if (q.nv == 4) {
    topk_f32x4 t;
    t[0] = q.v[0]; t[1] = q.v[1]; t[2] = q.v[2]; t[3] = q.v[3];
    *reinterpret_cast<topk_f32x4*>(dst + i) = t;
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (j < q.nv) dst[i + j] = q.v[j];
  }
}

// fadd(a, b) as one scalar instruction: the compiler pairs plain adds of neighbouring elements
// into packed fp32 adds, which this file does without
__device__ __forceinline__ float fadd_scalar(float a, float b) {
  float r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

__device__ __forceinline__ unsigned key_of(float m) { return __float_as_uint(m) & 0x7fffffffu; }

// set bits of a wave ballot below this lane
__device__ __forceinline__ unsigned below(uint64_t ballot) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// exclusive prefix of v over the 256 threads in thread order; ws: 4 words of LDS, free on return
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned* ws) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(incl, o, 64);
    if (lane >= (unsigned)o) incl += u;
  }
  if (lane == 63) ws[wave] = incl;
  __syncthreads();
  unsigned base = 0;
  for (unsigned w = 0; w < wave; ++w) base += ws[w];
  __syncthreads();
  return base + incl - v;
}

// every thread's vector stores and atomics drained, then thread 0 draws the two-level ticket
__device__ __forceinline__ bool arrive_block(unsigned* ctr, int* last) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) *last = arrive_last_grouped(ctr);
  __syncthreads();
  if (!*last) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // compiler order only: the loads that follow are sc1
  return true;
}

__device__ __forceinline__ unsigned ld_sc1(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(unsigned* p, unsigned v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int PASS>
__global__ __launch_bounds__(kThreads) void topk_pass_kernel(const float* __restrict__ g, float* __restrict__ e,
                                                             int64_t n, unsigned k, unsigned* __restrict__ hist,
                                                             unsigned* __restrict__ ctr, TopkBlock* __restrict__ blk) {
  constexpr int kBits = PASS == 2 ? 9 : 11, kBins = 1 << kBits;
  constexpr int kShift = PASS == 0 ? 20 : PASS == 1 ? 9 : 0;
  __shared__ unsigned lh[kBins];
  __shared__ unsigned ws[4];
  __shared__ int last;
  const unsigned tid = threadIdx.x;
  const unsigned prefix = PASS == 0 ? 0u : blk->prefix;  // uniform address: scalar loads
  const unsigned krem = PASS == 0 ? k : blk->krem;
  for (int i = tid; i < kBins; i += kThreads) lh[i] = 0;
  const int64_t base = (int64_t)blockIdx.x * kTopkChunk + 4 * tid;
  Quad q[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) q[r] = load_quad(e, base + r * 4 * kThreads, n);
  if (PASS == 0) {
    Quad gq[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) gq[r] = load_quad(g, base + r * 4 * kThreads, n);
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
#pragma unroll
      for (int j = 0; j < 4; ++j) q[r].v[j] = fadd_scalar(gq[r].v[j], q[r].v[j]);
      store_quad(e, base + r * 4 * kThreads, q[r]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned key = key_of(q[r].v[j]);
      if (j < q[r].nv && (PASS == 0 || (key >> (kShift + kBits)) == prefix))
        atomicAdd(&lh[(key >> kShift) & (kBins - 1)], 1u);
    }
  }
  __syncthreads();
  for (int i = tid; i < kBins; i += kThreads) {
    const unsigned c = lh[i];
    if (c) __hip_atomic_fetch_add(hist + i, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!arrive_block(ctr, &last)) return;
  // the last arriver: thread t owns the bins [kBins - per (t + 1), kBins - per t), top first
  constexpr int per = kBins / kThreads;
  const int top = kBins - per * (int)tid;
  unsigned h[per], sum = 0;
#pragma unroll
  for (int j = 0; j < per; ++j) {
    h[j] = ld_sc1(hist + top - 1 - j);
    sum += h[j];
  }
#pragma unroll
  for (int j = 0; j < per; ++j) st_sc1(hist + top - 1 - j, 0u);
  unsigned above = block_excl_scan(sum, ws);
  if (above < krem && krem <= above + sum) {  // one thread: 1 <= krem <= the keys histogrammed
#pragma unroll
    for (int j = 0; j < per; ++j) {
      if (krem <= above + h[j]) {
        const unsigned p = (prefix << kBits) | (unsigned)(top - 1 - j), left = krem - above;
        blk->prefix = p;
        blk->krem = left;
        if (PASS == 2) {
          blk->T = p;
          blk->ties = left;
          blk->c = k - left;
        }
        break;
      }
      above += h[j];
    }
  }
  if (tid == 0) arrive_rearm(ctr);
}

// cnt: [2 grid] words, #{key > T} then #{key == T} per chunk; on return their exclusive offsets
__global__ __launch_bounds__(kThreads) void topk_count_kernel(const float* __restrict__ e, int64_t n,
                                                              const TopkBlock* __restrict__ blk,
                                                              unsigned* __restrict__ cnt, unsigned* __restrict__ ctr) {
  __shared__ unsigned ws[4];
  __shared__ unsigned red[8];
  __shared__ int last;
  const unsigned tid = threadIdx.x, grid = gridDim.x;
  const unsigned T = blk->T;
  const int64_t base = (int64_t)blockIdx.x * kTopkChunk + 4 * tid;
  Quad q[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) q[r] = load_quad(e, base + r * 4 * kThreads, n);
  unsigned cg = 0, ce = 0;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned key = key_of(q[r].v[j]);
      cg += (j < q[r].nv && key > T);
      ce += (j < q[r].nv && key == T);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cg += __shfl_xor(cg, o, 64);
    ce += __shfl_xor(ce, o, 64);
  }
  if ((tid & 63) == 0) {
    red[tid >> 6] = cg;
    red[4 + (tid >> 6)] = ce;
  }
  __syncthreads();
  if (tid == 0) {
    st_sc1(cnt + blockIdx.x, red[0] + red[1] + red[2] + red[3]);
    st_sc1(cnt + grid + blockIdx.x, red[4] + red[5] + red[6] + red[7]);
  }
  if (!arrive_block(ctr, &last)) return;
  // the last arriver: thread t owns the chunks [run t, run (t + 1)) of both rows
  const unsigned run = (grid + kThreads - 1) / kThreads;
  const unsigned c0 = min(run * tid, grid), c1 = min(c0 + run, grid);
  unsigned sg = 0, se = 0;
  for (unsigned c = c0; c < c1; ++c) {
    sg += ld_sc1(cnt + c);
    se += ld_sc1(cnt + grid + c);
  }
  unsigned og = block_excl_scan(sg, ws), oe = block_excl_scan(se, ws);
  for (unsigned c = c0; c < c1; ++c) {
    const unsigned a = ld_sc1(cnt + c), b = ld_sc1(cnt + grid + c);
    cnt[c] = og;
    cnt[grid + c] = oe;
    og += a;
    oe += b;
  }
  if (tid == 0) arrive_rearm(ctr);
}

__global__ __launch_bounds__(kThreads) void topk_compact_kernel(float* __restrict__ e, int64_t n, unsigned k,
                                                                const TopkBlock* __restrict__ blk,
                                                                const unsigned* __restrict__ cnt,
                                                                int32_t* __restrict__ out) {
  __shared__ unsigned tg[kRounds][4], te[kRounds][4];
  const unsigned tid = threadIdx.x, wave = tid >> 6, grid = gridDim.x;
  const unsigned T = blk->T, ties = blk->ties;
  const unsigned gt_off = cnt[blockIdx.x], eq_off = cnt[grid + blockIdx.x];
  const unsigned left = ties > eq_off ? ties - eq_off : 0u;
  const unsigned out_base = gt_off + min(eq_off, ties);
  const int64_t base = (int64_t)blockIdx.x * kTopkChunk + 4 * tid;
  Quad q[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) q[r] = load_quad(e, base + r * 4 * kThreads, n);
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {  // the wave totals of every round first: only the popcounts live on
    unsigned wg = 0, we = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned key = key_of(q[r].v[j]);
      wg += __popcll(__ballot(j < q[r].nv && key > T));
      we += __popcll(__ballot(j < q[r].nv && key == T));
    }
    if ((tid & 63) == 0) {
      tg[r][wave] = wg;
      te[r][wave] = we;
    }
  }
  __syncthreads();
  // the ballots are formed again round by round (64 of them kept across the barrier cost 171 SGPR
  // spills); T2 is opaque so that the compiler does not carry the first loop's over
  unsigned T2 = T;
  asm volatile("" : "+s"(T2));
  unsigned rg = 0, re = 0;  // elements before (round, wave) in index order
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    unsigned mg = 0, me = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if ((unsigned)w == wave) {
        mg = rg;
        me = re;
      }
      rg += tg[r][w];
      re += te[r][w];
    }
    bool gts[4], eqs[4];
    unsigned gr = mg, er = me;  // + the key > T / key == T elements of this wave's round in lower lanes
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned key = key_of(q[r].v[j]);
      gts[j] = j < q[r].nv && key > T2;
      eqs[j] = j < q[r].nv && key == T2;
      gr += below(__ballot(gts[j]));
      er += below(__ballot(eqs[j]));
    }
    const int64_t i0 = base + r * 4 * kThreads;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool gt = gts[j], eq = eqs[j];
      const unsigned pos = out_base + gr + min(er, left);
      if ((gt || (eq && er < left)) && pos < k) {
        out[pos] = (int32_t)(i0 + j);
        out[(size_t)k + pos] = (int32_t)__float_as_uint(q[r].v[j]);
        e[i0 + j] = 0.f;
      }
      gr += gt;
      er += eq;
    }
  }
}

// first j in [0, k) with row[j] >= target, or k
__device__ __forceinline__ int lower_bound(const int32_t* __restrict__ row, int k, int target) {
  int lo = 0, hi = k;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (row[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ float topk_step(float a, float x, float& b, int N, float fN, float lr, float wd, float lam) {
  const float o = N != 1 ? __fdiv_rn(a, fN) : a;
  const float d = decayed(o, x, wd);
  float bl = __fmul_rn(b, lam);
  asm volatile("" : "+v"(bl));  // the build's -ffp-contract=fast would fuse the product into the add
  b = __fadd_rn(bl, d);
  return __fmaf_rn(-lr, __fadd_rn(d, b), x);
}

// acc[0 .. kTopkTile) = per element the rank-ordered sum of the values the ranks selected in the tile
// [tile_lo, tile_hi): the decompression both update kernels share.  bnd: 2 kRankRound words of LDS.
// Ends behind a barrier (N >= 1): acc is complete in every thread's view.
__device__ __forceinline__ void topk_accumulate(float* acc, int* bnd, const int32_t* __restrict__ gathered, int k,
                                                int N, int tile_lo, int tile_hi) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < kTopkTile / kThreads; ++i) acc[tid + i * kThreads] = 0.f;
  for (int r0 = 0; r0 < N; r0 += kRankRound) {
    const int nr = min(kRankRound, N - r0);
    __syncthreads();  // acc zeroed; the bounds of the round before are used up
    if (tid < 2 * nr)
      bnd[tid] = lower_bound(gathered + (size_t)(r0 + (tid >> 1)) * 2 * k, k, (tid & 1) ? tile_hi : tile_lo);
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
      const int32_t* __restrict__ row = gathered + (size_t)(r0 + r) * 2 * k;
      const int j1 = bnd[2 * r + 1];
      for (int j = bnd[2 * r] + tid; j < j1; j += kThreads) {
        const unsigned off = (unsigned)(row[j] - tile_lo);
        if (off < (unsigned)kTopkTile) acc[off] = __fadd_rn(acc[off], __uint_as_float((unsigned)row[k + j]));
      }
      __syncthreads();  // rank order
    }
  }
}

__global__ __launch_bounds__(kThreads) void topk_update_kernel(float* __restrict__ x, float* __restrict__ b, int64_t n,
                                                               const int32_t* __restrict__ gathered, int k, int N,
                                                               float lr_arg, float lam, const float* __restrict__ hyper) {
  __shared__ float acc[kTopkTile];
  __shared__ int bnd[2 * kRankRound];
  const Hyper hy = load_hyper(hyper, lr_arg);
  const int tid = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * kTopkTile;
  const int tile_lo = (int)lo, tile_hi = (int)min(lo + kTopkTile, n);
  Quad xq[2], bq[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    xq[h] = load_quad(x, lo + h * 4 * kThreads + 4 * tid, n);
    bq[h] = load_quad(b, lo + h * 4 * kThreads + 4 * tid, n);
  }
  topk_accumulate(acc, bnd, gathered, k, N, tile_lo, tile_hi);
  const float fN = (float)N;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int t0 = h * 4 * kThreads + 4 * tid;
    const topk_f32x4 a = *reinterpret_cast<const topk_f32x4*>(acc + t0);
#pragma unroll
    for (int j = 0; j < 4; ++j) xq[h].v[j] = topk_step(a[j], xq[h].v[j], bq[h].v[j], N, fN, hy.lr, hy.wd, lam);
    store_quad(x, lo + t0, xq[h]);
    store_quad(b, lo + t0, bq[h]);
  }
}

__device__ __forceinline__ Quad load_quad_nt(const float* __restrict__ src, int64_t i, int64_t n) {
  Quad q = {{0.f, 0.f, 0.f, 0.f}, 0};
  if (i + 4 <= n) {
    const topk_f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const topk_f32x4*>(src + i));
    q.v[0] = t[0]; q.v[1] = t[1]; q.v[2] = t[2]; q.v[3] = t[3];
    q.nv = 4;
  } else if (i < n) {
    q.nv = (int)(n - i);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (j < q.nv) q.v[j] = __builtin_nontemporal_load(src + i + j);
  }
  return q;
}

__device__ __forceinline__ void store_quad_nt(float* __restrict__ dst, int64_t i, const Quad& q) {
  if (q.nv == 4) {
    topk_f32x4 t;
    t[0] = q.v[0]; t[1] = q.v[1]; t[2] = q.v[2]; t[3] = q.v[3];
    __builtin_nontemporal_store(t, reinterpret_cast<topk_f32x4*>(dst + i));
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (j < q.nv) __builtin_nontemporal_store(q.v[j], dst + i + j);
  }
}

// topk_update with AdamW (adamw_elem.h: g := o, div = 1) behind the decompressed average: the same
// owner-computes tile, then the element rule over x (plain loads and stores), the first moment m (the
// SGD arm's momentum arena) and the second moment v (both touched once per step: non-temporal).
//   Decay.  A tile can span several tensors.  runs is int32 [nr][2] = (start, decays), start ascending
//   from runs[0].start = 0 and every start a multiple of 16 (tensors are padded to 16 elements, so a
//   float4 never straddles two runs; neighbours that decay alike are one run).  One thread finds the
//   run of the tile's first element by bisection, behind the loads already in flight and ahead of the
//   rank loop's first barrier; every thread walks on from there to the run of each of its two quads:
//   no per-element stream, and with few runs per tile no step at all.
//   The AdamBlock.  adam_block.h's protocol: thread 0 reads it ahead of the rank loop's barriers, the
//   scalars are formed behind them, thread 0 draws the ticket behind its stores.
//   Resources (hipcc --offload-arch=gfx950 -O3 -ffp-contract=fast, -Rpass-analysis=kernel-resource-usage):
//   60 VGPRs, 0 AGPRs, 61 SGPRs, no scratch (0 bytes/lane, no spills), 9228 B of LDS (the tile, the
//   bounds, 12 B for the block's products and the first run), occupancy 8 waves/SIMD
//   (topk_update_kernel: 41 VGPRs, 48 SGPRs, 9216 B, occupancy 8).
__global__ __launch_bounds__(kThreads) void topk_update_adam_kernel(
    float* __restrict__ x, float* __restrict__ m, float* __restrict__ v, int64_t n,
    const int32_t* __restrict__ gathered, int k, int N, const int* __restrict__ runs, int nr, float lr_arg,
    const float* __restrict__ hyper, AdamBlock* block, unsigned* ctr, float beta1, float beta2, float eps) {
  __shared__ float acc[kTopkTile];
  __shared__ int bnd[2 * kRankRound];
  __shared__ float pow_sh[2];
  __shared__ int run0;
  const unsigned steps = adam_block_read(block, pow_sh);
  const Hyper hy = load_hyper(hyper, lr_arg);
  const int tid = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * kTopkTile;
  const int tile_lo = (int)lo, tile_hi = (int)min(lo + kTopkTile, n);
  Quad xq[2], mq[2], vq[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    xq[h] = load_quad(x, lo + h * 4 * kThreads + 4 * tid, n);
    mq[h] = load_quad_nt(m, lo + h * 4 * kThreads + 4 * tid, n);
    vq[h] = load_quad_nt(v, lo + h * 4 * kThreads + 4 * tid, n);
  }
  if (tid == kThreads - 1) {  // the last run with start <= tile_lo (run 0 starts at 0)
    int a = 0, b = nr;
    while (b - a > 1) {
      const int mid = a + ((b - a) >> 1);
      if (runs[2 * mid] <= tile_lo) a = mid;
      else b = mid;
    }
    run0 = a;
  }
  topk_accumulate(acc, bnd, gathered, k, N, tile_lo, tile_hi);  // N >= 1: at least two barriers
  float p1, p2;
  AdamScalars S = adam_launch_scalars(pow_sh[0], pow_sh[1], hy.lr, hy.wd, beta1, beta2, eps, p1, p2);
  const float fN = (float)N;
  int r = run0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int t0 = h * 4 * kThreads + 4 * tid;
    while (r + 1 < nr && runs[2 * (r + 1)] <= tile_lo + t0) ++r;
    S.decay = hy.wd != 0.f && runs[2 * r + 1] != 0;
    const topk_f32x4 a = *reinterpret_cast<const topk_f32x4*>(acc + t0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float o = N != 1 ? __fdiv_rn(a[j], fN) : a[j];
      adamw_elem(xq[h].v[j], o, mq[h].v[j], vq[h].v[j], S);
    }
    store_quad(x, lo + t0, xq[h]);
    store_quad_nt(m, lo + t0, mq[h]);
    store_quad_nt(v, lo + t0, vq[h]);
  }
  adam_block_advance(ctr, block, p1, p2, steps);
}

}  // namespace

static int64_t topk_chunks(int64_t n) { return (n + kTopkChunk - 1) / kTopkChunk; }

int64_t topk_scratch_words(int64_t n) { return kTopkBins + arrive_ctr_words(topk_chunks(n)) + 2 * topk_chunks(n); }

void launch_topk_select(const float* g, float* e, int64_t n, int64_t k, uint32_t* scratch, TopkBlock* blk,
                        int32_t* out, int stage, hipStream_t s) {
  if (n <= 0) return;
  const int64_t grid = topk_chunks(n);
  unsigned* const hist = scratch;
  unsigned* const ctr = scratch + kTopkBins;
  unsigned* const cnt = ctr + arrive_ctr_words(grid);
  const dim3 G((unsigned)grid), B(kThreads);
  const unsigned uk = (unsigned)k;
  if (stage < 0 || stage == 0) hipLaunchKernelGGL(topk_pass_kernel<0>, G, B, 0, s, g, e, n, uk, hist, ctr, blk);
  if (stage < 0 || stage == 1) hipLaunchKernelGGL(topk_pass_kernel<1>, G, B, 0, s, g, e, n, uk, hist, ctr, blk);
  if (stage < 0 || stage == 2) hipLaunchKernelGGL(topk_pass_kernel<2>, G, B, 0, s, g, e, n, uk, hist, ctr, blk);
  if (stage < 0 || stage == 3) hipLaunchKernelGGL(topk_count_kernel, G, B, 0, s, e, n, blk, cnt, ctr);
  if (stage < 0 || stage == 4) hipLaunchKernelGGL(topk_compact_kernel, G, B, 0, s, e, n, uk, blk, cnt, out);
}

void launch_topk_update(float* x, float* b, int64_t n, const int32_t* gathered, int64_t k, int world, float lr,
                        float lam, const float* hyper, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(topk_update_kernel, dim3((unsigned)((n + kTopkTile - 1) / kTopkTile)), dim3(kThreads), 0, s, x,
                     b, n, gathered, (int)k, world, lr, lam, hyper);
}

void launch_topk_update_adam(float* x, float* m, float* v, int64_t n, const int32_t* gathered, int64_t k, int world,
                             const int32_t* runs, int64_t nr, float lr, const float* hyper, EfAdamArgs a,
                             hipStream_t s) {
  if (n <= 0 || world < 1 || nr < 1) return;  // the binding has refused these
  hipLaunchKernelGGL(topk_update_adam_kernel, dim3((unsigned)((n + kTopkTile - 1) / kTopkTile)), dim3(kThreads), 0, s,
                     x, m, v, n, gathered, (int)k, world, runs, (int)nr, lr, hyper, a.block, a.ctr, a.beta1, a.beta2,
                     a.eps);
}

}  // namespace ndp
