// The 1x1 stride-2 downsample convs (kConv1x1S2Map8 / kConv1x1S2Map4) as streamed GEMMs: the forward /
// grad-x wave body and the grad-W wave body (further down), shared by conv.hip's standalone kernels
// and its backward pair (direct_pair_kernel).  Device code only; every includer gets its own
// internal-linkage copy.
//
// Without taps the conv is a plain GEMM over gathered pixels:
//   forward  y[b, k, p, q]    = sum_c W[k, c] x[b, c, 2p, 2q]
//   grad-x   dx[b, c, 2p, 2q] = sum_k W[k, c] dy[b, k, p, q]      (odd pixels of dx: 0, or the addend)
//   grad-W   dW[k, c]         = sum_{b, p, q} dy[b, k, p, q] x[b, c, 2p, 2q]
// conv_fwd_body / conv_wgrad_body run them through LDS images of whole input planes in 8-channel
// chunks / one image at a time, each a global round trip, an LDS store and a barrier, with four to
// eight MFMAs between two barriers.  Here no operand goes through LDS and there is no barrier at all:
// a wave owns one 32 x 32 output tile, every lane loads exactly the operand values its MFMA steps
// consume (only stride-read pixels are touched), several steps' loads are in flight ahead of the
// MFMAs, and waves do not cooperate — a workgroup is just `wpw` independent waves.
//
// THE SUMMATION ORDER IS conv_fwd_body's / conv_wgrad_body's: every output element is one
// accumulator chain over the same MFMA steps, in the same order, with the same two k values per step
// (forward / grad-x: channels 8 g + t and 8 g + 4 + t at step t of chunk g; grad-W: pixels t and
// PQ / 2 + t of one image, images in slice order).  The results are bitwise the old bodies', so
// the split-K slabs, the grad-W slabs and everything downstream keep their values.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ndp {
namespace {

typedef float f32x16d __attribute__((ext_vector_type(16)));
typedef float f32x4d __attribute__((ext_vector_type(4)));
typedef float f32x2d __attribute__((ext_vector_type(2)));

// MAP: the conv's input map side (8: kConv1x1S2Map8, 4: kConv1x1S2Map4); the compact map (forward
// output / grad-x input) is P x Q = MAP/2 x MAP/2
template <int MAP>
struct DsGeom {
  static constexpr int P = MAP / 2, Q = MAP / 2, PQ = P * Q;
  static_assert(MAP == 8 || MAP == 4, "8x8 -> 4x4 or 4x4 -> 2x2");
};

struct DsArgs {
  const float *x, *w;  // forward: input, W[Kout][Cin]; grad-x: dY, W[Cin][Kout] (the same array)
  float *y, *part;
  const float* addend;  // grad-x, unsplit: added to every pixel of dx (may be dx itself)
  int Cin, Kout, B;     // reduction channels, output channels, images
  int crange;           // channels per grid z (a multiple of 8)
  int wpw, tiles;       // live waves per workgroup; 32 x 32 tiles per grid z
  int64_t slab;         // floats per split-K slab (compact [B][Kout][PQ])
};

// bid.x: workgroup along the tiles, bid.z: split-K part of gdim.z
template <int MAP, bool DGRAD>
__device__ __forceinline__ void ds_stream_body(const DsArgs& A, const uint3 bid, const uint3 gdim) {
  using G = DsGeom<MAP>;
  constexpr int PQ = G::PQ, Q = G::Q, D = 8;  // D: channel groups (4 channels per lane half) in flight
  constexpr int XPL = DGRAD ? PQ : MAP * MAP;  // floats per plane of the B operand
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = lane >> 5, l32 = lane & 31;
  const int tile = bid.x * A.wpw + wave;
  if (wave >= A.wpw || tile >= A.tiles) return;  // (wave-uniform; no barrier follows)
  const int mtl = A.Kout / 32;
  const int pt = tile / mtl, m0 = (tile - pt * mtl) * 32;  // neighbouring waves share their pixels
  const int n = pt * 32 + l32;                             // the lane's pixel of the compact maps
  const int img = n / PQ, pq = n - img * PQ, p = pq / Q, q = pq - p * Q;
  const bool valid = img < A.B;
  const int bl = valid ? img : A.B - 1;  // (loads stay in bounds; nothing is stored)
  const int nq = A.crange / 8;           // 8-channel chunks: group g = channels 8 g + 4 h .. + 3 of this half
  const int c0 = bid.z * A.crange + 4 * h;

  const float* xb = A.x + ((int64_t)bl * A.Cin + c0) * XPL + (DGRAD ? pq : 2 * p * MAP + 2 * q);
  const float* wa = DGRAD ? A.w + (int64_t)c0 * A.Kout + m0 + l32 : A.w + (int64_t)(m0 + l32) * A.Cin + c0;

  float av[D][4], bv[D][4];
  // (g clamped: a ring slot past the end reloads the last group, so that no load sits behind a
  // branch and every wait counts the loads in order)
  auto load = [&](int slot, int g) {
    g = min(g, nq - 1);
    if constexpr (DGRAD) {
#pragma unroll
      for (int i = 0; i < 4; ++i) av[slot][i] = wa[(int64_t)(8 * g + i) * A.Kout];
    } else {
      const f32x4d v = *reinterpret_cast<const f32x4d*>(wa + 8 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) av[slot][i] = v[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[slot][i] = xb[(int64_t)(8 * g + i) * XPL];
  };

  f32x16d acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  auto steps = [&](int d) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[d][i], bv[d][i], acc, 0, 0, 0);
  };

#pragma unroll
  for (int d = 0; d < D; ++d) load(d, d);
  int base = 0;
  for (; base + D < nq; base += D) {  // every slot is consumed and refilled
#pragma unroll
    for (int d = 0; d < D; ++d) {
      steps(d);
      load(d, base + d + D);
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d)  // the last ring: no more loads
    if (base + d < nq) steps(d);
  if (!valid) return;

  // accumulator register r of lane half h: output channel m0 + (r & 3) + 8 (r >> 2) + 4 h
  if (gdim.z > 1 || !DGRAD) {
    // split-K slab z of `part`, or the forward output (+ 0, as conv_fwd_body): compact [B][Kout][PQ]
    float* o = (gdim.z > 1 ? A.part + (int64_t)bid.z * A.slab : A.y) + ((int64_t)img * A.Kout + m0 + 4 * h) * PQ + pq;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[(int64_t)((r & 3) + 8 * (r >> 2)) * PQ] = gdim.z > 1 ? acc[r] : acc[r] + 0.f;
    return;
  }
  if constexpr (DGRAD) {
    // the lane's pixel (2p, 2q) of the MAP x MAP plane takes the product, its three odd neighbours
    // zero — or the addend alone.  All addends are loaded before any store.
    constexpr int OPL = MAP * MAP;
    const int64_t off = ((int64_t)img * A.Kout + m0 + 4 * h) * OPL + 2 * p * MAP + 2 * q;
    f32x2d r0[16], r1[16];
    if (A.addend != nullptr) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* ap = A.addend + off + (int64_t)((r & 3) + 8 * (r >> 2)) * OPL;
        r0[r] = *reinterpret_cast<const f32x2d*>(ap);
        r1[r] = *reinterpret_cast<const f32x2d*>(ap + MAP);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) r0[r] = r1[r] = f32x2d{0.f, 0.f};
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float* o = A.y + off + (int64_t)((r & 3) + 8 * (r >> 2)) * OPL;
      r0[r].x = acc[r] + r0[r].x;
      *reinterpret_cast<f32x2d*>(o) = r0[r];
      *reinterpret_cast<f32x2d*>(o + MAP) = r1[r];
    }
  }
}

// ---- grad-W ------------------------------------------------------------------------------------
// A wave owns one 32 x 32 block of one slice's slab: lane l32 loads its own dY row (channel k0 + l32)
// and the stride-read pixels of its own x plane (channel c0 + l32); lane half h takes the pixels
// h PQ/2 .. of every image, so no load is duplicated inside a wave.  Images in slice order, D of them
// in flight; one slab per slice in the [slice][Kout][Cin] layout.
struct DsWgArgs {
  const float *x, *dy;
  float* part;
  int Cin, Kout, imgs;  // imgs: images per slice
  int wpw, tiles;       // live waves per workgroup; slices x blocks
};

template <int MAP>
__device__ __forceinline__ void ds_wgrad_body(const DsWgArgs& A, const uint3 bid) {
  using G = DsGeom<MAP>;
  constexpr int PQ = G::PQ, Q = G::Q, XPL = MAP * MAP, HP = PQ / 2;  // HP: pixels per lane half
  constexpr int D = MAP == 8 ? 4 : 8;                                  // images in flight per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = lane >> 5, l32 = lane & 31;
  const int tile = bid.x * A.wpw + wave;
  if (wave >= A.wpw || tile >= A.tiles) return;  // (wave-uniform; no barrier follows)
  const int ncb = A.Cin / 32, blocks = (A.Kout / 32) * ncb;
  const int slice = tile / blocks, blk = tile - slice * blocks;
  const int mb = blk / ncb, k0 = mb * 32, c0 = (blk - mb * ncb) * 32;
  const int np = A.imgs;
  const int b0 = slice * A.imgs;
  // this half's pixels: rows h P/2 .. of the compact map = rows 2 (h P/2 + i) of x
  const float* xp = A.x + ((int64_t)b0 * A.Cin + c0 + l32) * XPL + h * (G::P / 2) * 2 * MAP;
  const float* yp = A.dy + ((int64_t)b0 * A.Kout + k0 + l32) * PQ + h * HP;
  const int64_t xs = (int64_t)A.Cin * XPL, ys = (int64_t)A.Kout * PQ;  // to the next image

  float xv[D][HP], yv[D][HP];
  auto load = [&](int slot, int t) {  // (t clamped: no load behind a branch, see ds_stream_body)
    t = min(t, np - 1);
    if constexpr (MAP == 8) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f32x4d v = *reinterpret_cast<const f32x4d*>(yp + t * ys + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) yv[slot][4 * i + j] = v[j];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {  // rows 2 (2h), 2 (2h + 1): two float4 each, even columns
        const f32x4d v = *reinterpret_cast<const f32x4d*>(xp + t * xs + (i / 2) * 2 * MAP + 4 * (i % 2));
        xv[slot][2 * i] = v.x;
        xv[slot][2 * i + 1] = v.z;
      }
    } else {
      const f32x2d u = *reinterpret_cast<const f32x2d*>(yp + t * ys);
      yv[slot][0] = u.x;
      yv[slot][1] = u.y;
      const f32x4d v = *reinterpret_cast<const f32x4d*>(xp + t * xs);
      xv[slot][0] = v.x;
      xv[slot][1] = v.z;
    }
  };
  f32x16d acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  auto steps = [&](int slot) {
#pragma unroll
    for (int t = 0; t < HP; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(yv[slot][t], xv[slot][t], acc, 0, 0, 0);
  };

#pragma unroll
  for (int d = 0; d < D; ++d) load(d, d);
  int base = 0;
  for (; base + D < np; base += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      steps(d);
      load(d, base + d + D);
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (base + d < np) steps(d);

  // register r of lane half h: row k0 + (r & 3) + 8 (r >> 2) + 4 h, column c0 + l32
  float* out = A.part + ((int64_t)slice * A.Kout + k0 + 4 * h) * A.Cin + c0 + l32;
#pragma unroll
  for (int r = 0; r < 16; ++r) out[(int64_t)((r & 3) + 8 * (r >> 2)) * A.Cin] = acc[r];
}

}  // namespace
}  // namespace ndp
