#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "ndp_kernels.h"

namespace ndp {

struct Plan {
  std::vector<MatGeom> geom;
  std::vector<int32_t> q_rows;  // rows per Q split-K chunk, per matrix
  std::vector<PItem> p_items;
  int64_t n_p_blocks = 0;  // P row blocks / Q column blocks (in-kernel split-K arrival counters)
  int64_t n_q_blocks = 0;
  std::vector<QItem> q_items;
  std::vector<UItem> u_items;
  std::vector<OrthItem> orth_items;
  int64_t p_total = 0, q_total = 0, pp_total = 0, qp_total = 0;
  int max_rank = 1;
  int32_t p_cols = kPKW;  // columns per P item (wide plans)
};

// shapes[i] = (n_i, m_i) of every >1-D tensor, in model.parameters() order.
// supports (empty, or one per matrix): the live taps of conv weights; a matrix with dead taps in a
// wide plan (max rank <= kUWideMaxRank) keeps its error memory and momentum compact (MatGeom
// tap_*): its Q and update items tile the compact columns, its P items are unchanged.
Plan build_plan(const std::vector<std::pair<int64_t, int64_t>>& shapes, int rank,
                const std::vector<TapSupport>& supports = {});

// columns of a matrix's error-memory / momentum slot (m unless compacted)
inline int64_t compact_cols(const MatGeom& g) {
  return g.tap_T ? (int64_t)(g.m / g.tap_T) * g.tap_L : (int64_t)g.m;
}
// full column of compact column j (identity unless compacted), and the inverse (-1: dead tap)
inline int64_t full_col(const MatGeom& g, int64_t j) {
  if (!g.tap_T) return j;
  const int64_t k = j % g.tap_L;
  return (j / g.tap_L) * g.tap_T + (g.taps[k >> 3] >> (4 * (k & 7)) & 15u);
}
inline int64_t compact_col(const MatGeom& g, int64_t b) {
  if (!g.tap_T) return b;
  const int t = (int)(b % g.tap_T);
  if (!(g.tap_mask >> t & 1u)) return -1;
  return (b / g.tap_T) * g.tap_L + __builtin_popcount(g.tap_mask & ((1u << t) - 1u));
}

// multi-workgroup MGS work list for the given matrices (rows split in 256*RPT blocks)
std::vector<OrthItem> build_orth_items(const std::vector<MatGeom>& geom, int max_rank);

struct SegSpec {
  uintptr_t src, dst;
  int64_t numel, stride;
  int32_t chunks;
  float div;
};

struct SegTable {
  std::vector<SegEntry> entries;
  std::vector<int64_t> prefix;
  int64_t n_blocks = 0;
};

SegTable build_seg_table(const std::vector<SegSpec>& specs);

// The AdamW kernel's table (adamw.hip): src = gradient, dst = parameter, stride = `off`, the
// entry's element offset into the two moment arenas at m_base / v_base (arena_numel floats each),
// pad bit 0 (kAdamNoDecay) = no weight decay, vec = gradient, parameter and both moments 16-byte
// aligned.  Throws std::invalid_argument for a moment range outside the arenas.
struct AdamSpec {
  uintptr_t g, x;
  int64_t numel, off;
  bool decay;
};
SegTable build_adamw_table(const std::vector<AdamSpec>& specs, uintptr_t m_base, uintptr_t v_base,
                           int64_t arena_numel);

}  // namespace ndp
