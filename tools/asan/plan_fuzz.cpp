// Host-side AddressSanitizer / UBSan fuzz of the PowerSGD plan builder (csrc/plan.cpp):
// random model shapes and ranks -> build_plan / build_orth_items / build_seg_table, with
// the invariants the GPU kernels rely on checked on every plan (sanitizers
// on host code only — GPU ASan is not available on this pool).  Half of the plans get random
// live-tap supports (dead-tap compaction): the compact Q / update items must cover every live
// column exactly once, the P items and every offset must be those of the plan without supports.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Inetwork_distributed_pytorch_amd/csrc \
//       tools/asan/plan_fuzz.cpp network_distributed_pytorch_amd/csrc/plan.cpp -o /tmp/plan_fuzz
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "plan.h"

namespace ndp {
// the device-occupancy query lives in orth.hip; on the host fuzz use the conservative path
int orth_coresident_cap(int) { return -1; }
int orth_rows_per_thread(int max_rank) {
  if (max_rank <= 8) return 8;
  if (max_rank <= 16) return 4;
  if (max_rank <= 32) return 2;
  return 1;
}
}  // namespace ndp

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::fprintf(stderr, "invariant failed: %s (line %d)\n", #c, __LINE__); \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

int main(int argc, char** argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 300;
  std::mt19937_64 rng(1234);
  int64_t plans = 0;
  for (int it = 0; it < iters; ++it) {
    const int n_mats = 1 + (int)(rng() % 60);
    const int rank = 1 + (int)(rng() % 64);
    std::vector<std::pair<int64_t, int64_t>> shapes;
    for (int i = 0; i < n_mats; ++i) {
      const int64_t n = 1 + (int64_t)(rng() % (rng() % 4 == 0 ? 40000 : 600));
      const int64_t m = 1 + (int64_t)(rng() % (rng() % 4 == 0 ? 5000 : 600));
      shapes.emplace_back(n, m);
    }
    ndp::Plan pl;
    try {
      pl = ndp::build_plan(shapes, rank);
    } catch (const std::exception&) {
      continue;  // e.g. a matrix whose MGS needs more workgroups than the conservative cap
    }
    ++plans;
    // random supports: conv-like matrices (m a multiple of the tap period) among arbitrary ones
    std::vector<ndp::TapSupport> sup(n_mats, ndp::TapSupport{0, 0u});
    for (int i = 0; i < n_mats; ++i) {
      const int T = 1 + (int)(rng() % 20);  // also periods the plan must refuse (1, > 16)
      if (rng() % 2) sup[i] = ndp::TapSupport{T, (uint32_t)rng()};
      if (rng() % 4 == 0) sup[i].T = (int32_t)(rng() % 3) - 1;  // -1, 0, 1
    }
    const ndp::Plan pc = ndp::build_plan(shapes, rank, sup);
    {  // no supports (absent or all empty): byte-for-byte the plan above
      const ndp::Plan pe = ndp::build_plan(shapes, rank, std::vector<ndp::TapSupport>(n_mats, ndp::TapSupport{0, 0u}));
      CHECK(pe.geom.size() == pl.geom.size() && pe.q_items.size() == pl.q_items.size() &&
            pe.u_items.size() == pl.u_items.size() && pe.p_items.size() == pl.p_items.size());
      CHECK(std::memcmp(pe.geom.data(), pl.geom.data(), pl.geom.size() * sizeof(ndp::MatGeom)) == 0);
      CHECK(std::memcmp(pe.q_items.data(), pl.q_items.data(), pl.q_items.size() * sizeof(ndp::QItem)) == 0);
      CHECK(std::memcmp(pe.u_items.data(), pl.u_items.data(), pl.u_items.size() * sizeof(ndp::UItem)) == 0);
      CHECK(std::memcmp(pe.p_items.data(), pl.p_items.data(), pl.p_items.size() * sizeof(ndp::PItem)) == 0);
      CHECK(pe.n_q_blocks == pl.n_q_blocks && pe.n_p_blocks == pl.n_p_blocks);
    }
    // P items, offsets, chunking and totals do not depend on the supports
    CHECK(pc.p_items.size() == pl.p_items.size() && pc.n_p_blocks == pl.n_p_blocks && pc.p_cols == pl.p_cols);
    CHECK(pl.p_items.empty() ||
          std::memcmp(pc.p_items.data(), pl.p_items.data(), pl.p_items.size() * sizeof(ndp::PItem)) == 0);
    CHECK(pc.p_total == pl.p_total && pc.q_total == pl.q_total && pc.pp_total == pl.pp_total &&
          pc.qp_total == pl.qp_total && pc.max_rank == pl.max_rank && pc.q_rows == pl.q_rows);
    const bool wide = pl.max_rank <= ndp::kUWideMaxRank;
    std::vector<std::vector<int>> q_cover(n_mats), u_cover(n_mats);
    int64_t q_blocks = 0;
    for (int i = 0; i < n_mats; ++i) {
      const ndp::MatGeom& g = pc.geom[i];
      const ndp::MatGeom& f = pl.geom[i];
      CHECK(g.n == f.n && g.m == f.m && g.r == f.r && g.p_off == f.p_off && g.q_off == f.q_off &&
            g.pp_off == f.pp_off && g.qp_off == f.qp_off && g.p_chunks == f.p_chunks && g.q_chunks == f.q_chunks);
      const int64_t mc = ndp::compact_cols(g);
      if (g.tap_T) {
        CHECK(wide && g.tap_T == sup[i].T && g.tap_T >= 2 && g.tap_T <= ndp::kMaxTapPeriod && g.m % g.tap_T == 0);
        CHECK(g.tap_L >= 1 && g.tap_L < g.tap_T && g.tap_L == __builtin_popcount(g.tap_mask));
        CHECK(g.tap_mask == (sup[i].mask & ((1u << g.tap_T) - 1u)) && mc < g.m && mc >= 1);
        int64_t prev = -1;
        for (int64_t j = 0; j < mc; ++j) {  // the map is increasing, lands on live taps, and inverts
          const int64_t b = ndp::full_col(g, j);
          CHECK(b > prev && b < g.m && (g.tap_mask >> (b % g.tap_T) & 1u) && ndp::compact_col(g, b) == j);
          prev = b;
        }
        int64_t live = 0;
        for (int64_t b = 0; b < g.m; ++b) live += ndp::compact_col(g, b) >= 0;
        CHECK(live == mc);
      } else {
        CHECK(mc == g.m && g.tap_L == 0 && g.tap_mask == 0u && g.taps[0] == 0u && g.taps[1] == 0u);
      }
      q_cover[i].assign((size_t)(mc * g.q_chunks), 0);
      u_cover[i].assign((size_t)mc, 0);
      q_blocks += (mc + ndp::kQCols - 1) / ndp::kQCols;
    }
    CHECK(pc.n_q_blocks == q_blocks);
    for (const auto& q : pc.q_items) {  // every (compact column, row chunk) exactly once, cb in range
      const ndp::MatGeom& g = pc.geom[q.mat];
      const int64_t mc = ndp::compact_cols(g);
      CHECK(q.col0 >= 0 && q.col0 < mc && q.col0 % ndp::kQCols == 0 && q.chunk >= 0 && q.chunk < g.q_chunks);
      CHECK(q.row0 >= 0 && q.row0 < q.row1 && q.row1 <= g.n && q.row1 - q.row0 <= ndp::kQRowsMax);
      CHECK(q.cb >= 0 && q.cb < pc.n_q_blocks);
      for (int64_t j = q.col0; j < std::min<int64_t>(mc, q.col0 + ndp::kQCols); ++j)
        ++q_cover[q.mat][(size_t)(j * g.q_chunks + q.chunk)];
    }
    const int64_t u_rows = wide ? ndp::kUWideRows : ndp::kURows, u_cols = wide ? ndp::kUWideCols : ndp::kUCols;
    for (const auto& u : pc.u_items) {  // row block 0's tiles cover every compact column once
      const ndp::MatGeom& g = pc.geom[u.mat];
      const int64_t mc = ndp::compact_cols(g);
      CHECK(u.col0 >= 0 && u.col0 < mc && u.col0 % u_cols == 0 && u.row0 >= 0 && u.row0 < g.n && u.row0 % u_rows == 0);
      if (u.row0 == 0)
        for (int64_t j = u.col0; j < std::min<int64_t>(mc, u.col0 + u_cols); ++j) ++u_cover[u.mat][(size_t)j];
    }
    for (int i = 0; i < n_mats; ++i) {
      for (int c : q_cover[i]) CHECK(c == 1);
      for (int c : u_cover[i]) CHECK(c == 1);
    }
    int64_t n_u = 0;
    for (int i = 0; i < n_mats; ++i)
      n_u += ((pc.geom[i].n + u_rows - 1) / u_rows) * ((ndp::compact_cols(pc.geom[i]) + u_cols - 1) / u_cols);
    CHECK((int64_t)pc.u_items.size() == n_u);
    CHECK((int)pl.geom.size() == n_mats);
    int64_t p_off = 0, q_off = 0;
    for (int i = 0; i < n_mats; ++i) {
      const ndp::MatGeom& g = pl.geom[i];
      CHECK(g.n == shapes[i].first && g.m == shapes[i].second);
      CHECK(g.r >= 1 && g.r <= rank && g.r <= g.n && g.r <= g.m);
      CHECK(g.p_off == p_off && g.q_off == q_off);
      p_off += g.n * g.r;
      q_off += g.m * g.r;
    }
    CHECK(pl.p_total == p_off && pl.q_total == q_off);
    for (const auto& it2 : pl.p_items) CHECK(it2.mat >= 0 && it2.mat < n_mats && it2.k0 < it2.k1);
    for (const auto& it2 : pl.q_items) CHECK(it2.mat >= 0 && it2.mat < n_mats && it2.row0 < it2.row1);
    for (const auto& it2 : pl.orth_items) {
      CHECK(it2.mat >= 0 && it2.mat < n_mats && it2.row0 < it2.row1 && it2.wg < it2.nwg);
      CHECK(it2.row1 <= pl.geom[it2.mat].n);
    }
    std::vector<ndp::SegSpec> specs;
    for (int i = 0; i < n_mats; ++i)
      specs.push_back({(uintptr_t)(16 * (i + 1)), (uintptr_t)(16 * (i + 7)), shapes[i].first * (i % 3 + 1),
                       shapes[i].first, (int32_t)(i % 4 + 1), 1.f});
    const ndp::SegTable t = ndp::build_seg_table(specs);
    CHECK(t.entries.size() == t.prefix.size());
  }
  std::printf("plan_fuzz ok: %lld plans\n", (long long)plans);
  return 0;
}
