// Shared device-table layouts and host launch entry points for the gfx950 kernels.
//
// Every hot op of the reference's PowerSGD step is a grouped
// kernel driven by a device-side table built once per model by the plan builder
// (plan.cpp).  The tables replace the reference's per-tensor Python loops
// (reference: ddp_powersgd_guide_cifar10/reducer.py:86-168).
//
// All launchers take raw device pointers + a hipStream_t and never allocate or
// synchronise, so every call is hipGraph-capturable.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace ndp {

// ---- PowerSGD plan geometry (one per high-rank matrix, 64 B) ----------------------
struct MatGeom {
  int32_t n, m, r;      // matrix = param.view(n, m); r = min(n, m, R)
  int32_t vec;          // 1 -> m % 4 == 0 and every bound pointer 16-B aligned (float4 path)
  int32_t p_off, q_off; // element offsets into the flat P / Q buffers (reference order)
  int32_t pp_off, qp_off;     // element offsets into the P / Q split-K partial scratch
  int32_t p_chunks, q_chunks; // number of split-K slabs for P (over m) and Q (over n)
  // Dead-tap compaction (wide plans only; tap_T == 0: none).  The matrix is a conv weight whose
  // columns repeat with period tap_T = KH*KW, and only tap_L of those taps can ever receive
  // gradient.  Its error memory and momentum are then stored as [n, (m / tap_T) * tap_L]:
  // compact column j is full column (j / tap_L) * tap_T + tap[j % tap_L].  The parameter, its
  // gradient and the P / Q buffers keep the full layout.  With tap_T != 0, `vec` is two bits:
  // 1 = float4 on the full-width gradient (P pass), 2 = float4 on the compact M (Q pass).
  int32_t tap_T, tap_L;
  uint32_t taps[2];           // live taps, ascending, 4 bits each (tap_T <= kMaxTapPeriod)
  uint32_t tap_mask;          // bit t set = tap t is live
  int32_t pad;
};
constexpr int kMaxTapPeriod = 16;
// live taps of one matrix for the plan builder: period T (0 = no support known) and bitmask
struct TapSupport { int32_t T; uint32_t mask; };

// ---- per-matrix bound pointers (64 B) -------------------------------------------
// engine mode : min = grad, e = error memory (M = g + e is written back into e),
//               mread = e, mom = momentum, x = parameter, g = grad (optional write)
// api mode    : min = M (caller's send buffer), e = nullptr, mread = M,
//               out = grad_out, mem = memory_out
struct MatPtrs {
  const float* min;
  float* e;
  const float* mread;
  float* out;
  float* mem;
  float* mom;
  float* x;
  float* g;
};

// Work items.  One workgroup (4 waves) per item.
// rb / cb: ordinal of the item's P row block / Q column block in the plan (the arrival counter
// of the in-kernel split-K finish, PFin / QFin)
struct PItem { int32_t mat, row0, k0, k1, chunk, rb, pad[2]; };   // 64 rows x [k0,k1)
struct QItem { int32_t mat, col0, row0, row1, chunk, cb, pad[2]; }; // [row0,row1) x 256 cols
struct UItem { int32_t mat, row0, col0, pad; };                 // 64 rows x 64 cols
// orth: rows [row0,row1) of matrix `mat`; workgroup `wg` of `nwg`; slab0 = first item of mat
struct OrthItem { int32_t mat, row0, row1, wg, nwg, slab0, pad[2]; };

// Segmented reduce-copy entry: dst[k] = (sum_c src[c*stride + k]) / div
struct SegEntry {
  const float* src;
  float* dst;
  int64_t numel;
  int64_t stride;
  int32_t chunks;
  float div;
  int32_t vec;
  int32_t pad;
};

constexpr int kPRows = 64;    // rows per P item (4 waves x 16)
constexpr int kPK = 256;      // k-chunk of a P item
// plans whose max rank is <= kUWideMaxRank use kPWRows x kPKW P items (psgd_p_wide_kernel)
constexpr int kPWRows = 16;
constexpr int kPKW = 1024;
constexpr int kQCols = 256;   // columns per Q item (4 waves x 64)
constexpr int kQRowsMax = 256;  // max rows per Q item (LDS: 256 x (16*NCG+pad) floats)
constexpr int kURows = 64;
constexpr int kUCols = 64;
// plans whose max rank is <= kUWideMaxRank use 16 x 256 update tiles (psgd_update_wide_kernel)
constexpr int kUWideRows = 16;
constexpr int kUWideCols = 256;
constexpr int kUWideMaxRank = 16;
constexpr int kMaxRank = 64;
constexpr int kSegBlockElems = 2048;  // elements per workgroup of a SegEntry table (seg_block.h)

// ---- launchers (powersgd.hip) --------------------------------------------------
// p_prev (rank <= kUWideMaxRank only): lazy error feedback, e = M_prev - P_prev Qs^T formed here
// In-kernel split-K finish of the P / Q passes: every chunk item stores its
// partial write-through (sc1), drains, and bumps its row / column block's monotonic arrival
// counter; the block's last arriver sums the chunk partials in chunk order (the order of the
// seg_reduce it replaces: bitwise identical) and writes the final P / Q.  out == nullptr: leave
// the partials for a separate seg_reduce.  P's extra blocks [n_items, grid) run a seg table (the
// rank-1 group's pack into the comm buffer), so the P stage is ONE launch.
struct PFin {
  unsigned* err;                 // sticky error word: |= kErrDeadTapGrad on a nonzero dead-tap gradient
  float* out;                    // final P (comm buffer, MatGeom.p_off)
  unsigned long long* ctr;       // [n row blocks]
  const SegEntry* seg;           // optional reduce-copy table run by the extra blocks
  const int64_t* seg_prefix;
  int n_seg;
  int n_items;
};
struct QFin {
  float* out;                    // final Q sums (q_memory, MatGeom.q_off)
  unsigned long long* ctr;       // [n column blocks]
  int max_chunks;                // matrices with more row chunks leave their partials to seg_reduce
};
// the rank-1 (<= 1-D) group's momentum / SGD step, run by the update pass's extra blocks
struct R1Step {
  const float* buf;
  float* mom;
  float* x;
  float* g;
  int64_t n;
  float div;
  int n_items;
};

void launch_psgd_p(const MatGeom* geom, const MatPtrs* ptrs, const PItem* items, int n_items,
                   const float* q_warm, float* p_part, int fuse_ef, int max_rank, hipStream_t s,
                   const float* p_prev = nullptr, PFin fin = PFin{}, int64_t n_seg_blocks = 0,
                   int item_cols = kPKW);
void launch_psgd_q(const MatGeom* geom, const MatPtrs* ptrs, const QItem* items, int n_items,
                   const float* p_hat, float* q_part, int max_rank, hipStream_t s, QFin fin = QFin{});
// partial: 2 * n_items_total * kMaxRank floats; counters: n_mats uint64 (zeroed once, never reset);
// items may be a slice [k0, k0 + n_items) of an n_items_total list (slab0 indexes are global)
void launch_psgd_orth(const MatGeom* geom, const OrthItem* items, int n_items, int n_mats, float* p,
                      float p_div, float eps, int max_rank, float* partial, unsigned long long* counters,
                      unsigned* err, int n_items_total, unsigned max_spins, hipStream_t s);
int orth_rows_per_thread(int max_rank);
// workgroups of ONE matrix the MGS barrier may span: occupancy x CUs / 2 (-1: no device)
int orth_coresident_cap(int max_rank);
constexpr unsigned kOrthMaxSpins = 1u << 25;  // ~seconds of s_sleep 2
// bits of the sticky device error word shared by the orth and P kernels
constexpr unsigned kErrOrthTimeout = 1u;
constexpr unsigned kErrDeadTapGrad = 2u;
// mode 0 = api (out/mem), 1 = engine (EF + momentum + SGD), 2 = engine + write grad,
// 3 = e -= p_hat q_sum^T / q_div only (materialise the lazy error, rank <= kUWideMaxRank);
// p_prev (modes 1 / 2, rank <= kUWideMaxRank): lazy error feedback — e is not written, the
// P-hat rows are kept in p_prev for the next P pass.
// hyper (every update launcher below; hyper.h): the device block [lr, weight_decay, 0, 0] the
// kernels read instead of the by-value lr — nullptr keeps lr by value and weight_decay = 0.
// With d = (wd != 0 ? fmaf(wd, x, out) : out):  m = lam*m + d;  x -= lr*(d + m)
void launch_psgd_update(const MatGeom* geom, const MatPtrs* ptrs, const UItem* items,
                        int n_items, const float* p_hat, const float* q_sum, float q_div,
                        float* q_warm, int mode, float lr, float momentum, int max_rank,
                        hipStream_t s, float* p_prev = nullptr, R1Step r1 = R1Step{},
                        const float* hyper = nullptr);
// rank-1 (<=1-D) group of the fused engine: out = buf/div; m = lam*m + out; x -= lr*(out+m)
void launch_rank1_step(const float* buf, float div, float* mom, float* x, float* g,
                       int64_t n, float lr, float momentum, hipStream_t s, const float* hyper = nullptr);

// ---- launchers (multitensor.hip) -----------------------------------------------
void launch_seg_reduce(const SegEntry* entries, const int64_t* block_prefix, int n_entries,
                       int64_t n_blocks, hipStream_t s);
// dense arm: b = mu*b + g/div ; x -= lr*b   (torch.optim.SGD(momentum) with zero-init buf);
// with a hyper block: b = mu*b + (g/div + wd*x), torch.optim.SGD(momentum, weight_decay)
void launch_sgd_momentum(float* x, const float* g, float* buf, int64_t n, float lr, float mu,
                         float div, hipStream_t s, const float* hyper = nullptr);
// out = a + b  (EF pack: send = g + e)
void launch_add(const float* a, const float* b, float* out, int64_t n, hipStream_t s);
// spin the stream for `ns` nanoseconds of wall time (link-emulation pacing)
void launch_delay_ns(int64_t ns, hipStream_t s);
// device-flag ordering between two queues: signal bumps *ctr; wait spins until *ctr has
// been bumped once more than *seen records (then records it); err |= 1 on spin timeout
void launch_flag_signal(unsigned* ctr, hipStream_t s);
void launch_flag_wait(unsigned* ctr, unsigned* seen, unsigned* err, int64_t timeout_us, hipStream_t s,
                      unsigned* host_err = nullptr);
// deterministic fp64-accumulated checksum of a flat buffer (replica divergence detector)
void launch_checksum(const float* x, int64_t n, double* out, hipStream_t s);

}  // namespace ndp

// ---- fused BatchNorm2d (+residual) (+ReLU), NCHW fp32 (batchnorm.hip) -------------------
// A call is decided once: the binding states what it offers in a BnQuery, bn_make_route answers
// with a BnRoute, validates against it and hands it to the launcher, which only executes it.
namespace ndp {
enum BnPath { kBnNone = 0, kBnFused, kBnFused64, kBnThreeKernel, kBnTwoKernel };
// deferred split-K slabs of the input: none (fewer than two count as none), added inside the BN
// launch, or by a launch_slab_sum of their own first (with the grad-x addend when one came along)
enum BnSlab { kBnSlabNone = 0, kBnSlabInKernel, kBnSlabSumFirst };

// 16-byte alignment of the operand sets the float4 kernels read or write (bn_alignment)
struct BnAlign {
  bool fused = true;   // single-launch set: forward x, res, out; backward x, dy, yin, out, dres; the pair's x2, out2
  bool two = true;     // two-kernel set: forward x, out, res; backward dy, x, out, dres and yin under relu
  bool slabs = true;   // the slabs of the main input and the addend
  bool slabs2 = true;  // the slabs of the pair's x2
};

struct BnQuery {
  int bwd = 0;
  int N = 0, C = 0, HW = 0;
  bool training = true;  // forward only
  bool single = false;   // allow the single-launch paths
  bool pair = false;     // the downsample block's two BNs in one launch (BnPair)
  int pool_w = 0;        // > 0: the stem tail (BN -> ReLU -> max-pool) on maps of this width
  int nslab = 0, nslab2 = 0;  // slabs offered for x / dy, and for the pair's x2
  int ext_slices = 0;    // > 0: xstats / dstats offered, this many partials per channel
  bool relu = false;
  bool addend = false;   // dyadd
  bool mbeta = false;    // ReLU mask recomputed from x
  BnAlign al;
};

struct BnRoute {
  int bwd, N, C, HW, pool_w, pair;
  int training;  // batch statistics (every backward, the stem tail, a training forward)
  int path;      // BnPath; kBnNone: the query cannot be served (pair or mbeta outside their paths)
  // single-launch paths
  int v4;        // the float4 kernel (else the scalar one)
  int CW, MAXN;  // column-block width, rows the register arrays hold
  int split;     // workgroups per column block (8x8 maps: 1, 2 or 4)
  int grid;
  // two-kernel path
  int vec;         // float4 kernels
  int S, Sa;       // slices of the statistics pass, of the apply pass
  int stats_pass;  // the statistics pass runs
  int Sp;          // > 0: the apply folds this many external partials per channel instead of `part`
  // three-kernel path
  int Ss;
  int slab, slab2;     // BnSlab of x / dy, of the pair's x2
  int addend;          // dyadd goes wherever the slabs are summed (dropped when there are none)
  int64_t part_numel;  // doubles of `part` scratch the call may touch
};
BnRoute bn_make_route(const BnQuery& q);

// the downsample block's second BN (over x2, same shape) for the single-launch kernels
struct BnPair {
  const float* x2;
  const float* gamma2;
  const float* beta2;
  float* rmean2;
  float* rvar2;
  int64_t* nbt2;
  float* save_mean2;
  float* save_invstd2;
  float* dgamma2;
  float* dbeta2;
  float* out2;
  const float* src2;  // forward: x2 as nslab2 unsummed split-K slabs (summed here, stored to x2), or null
  int nslab2;
};

// Operands of one BN call; unused ones stay null.  Forward: x, res -> out.  Backward: dy, yin (the
// forward output, for the ReLU mask), x -> out (dx), dres, dgamma, dbeta.
struct BnOps {
  const float *x = nullptr, *res = nullptr, *dy = nullptr, *yin = nullptr, *gamma = nullptr, *beta = nullptr;
  float *rmean = nullptr, *rvar = nullptr;
  int64_t* nbt = nullptr;
  float *save_mean = nullptr, *save_invstd = nullptr, *dgamma = nullptr, *dbeta = nullptr, *out = nullptr, *dres = nullptr;
  float eps = 0.f, momentum = 0.f;
  int relu = 0;
  double* part = nullptr;  // BnRoute::part_numel doubles of scratch
  // x (forward) / dy (backward) as `nslab` unsummed split-K slabs of numel(x) floats (a deferred conv
  // sum; the forward also writes the sum to x), and dyadd: dy = sum of the slabs + addend, added last
  const float* slabs = nullptr;
  int nslab = 0;
  const float* addend = nullptr;
  // xstats / dstats: [C][BnRoute::Sp][2] fp64 partial sums from the producing conv's epilogue
  const double* stats = nullptr;
  // y was never stored (stem tail): the ReLU mask is recomputed from x as
  // fmaf(x, gamma * invstd, mbeta - mean * gamma * invstd) > 0 (the forward's own ops)
  const float* mbeta = nullptr;
  uint8_t* idx = nullptr;  // stem tail: the pooled output's uint8 window offsets (pool.hip layout)
};
BnAlign bn_alignment(int bwd, const BnOps& o, const BnPair* pr = nullptr);

void launch_bn_fwd(const BnOps& o, const BnRoute& r, hipStream_t s);
void launch_bn_bwd(const BnOps& o, const BnRoute& r, hipStream_t s);
void launch_bn_pair_fwd(const BnOps& o, const BnPair& pr, const BnRoute& r, hipStream_t s);
void launch_bn_pair_bwd(const BnOps& o, const BnPair& pr, const BnRoute& r, hipStream_t s);
// BN (training) -> ReLU -> MaxPool(3, 2, 1) in one pass without storing the BN output (the
// ResNet stem tail); o.out / o.idx: the pooled output and its window offsets
void launch_bn_relu_maxpool(const BnOps& o, const BnRoute& r, hipStream_t s);
// shape-only views of the route
int bn_slices(int N, int C, int HW);
int64_t bn_part_numel(int N, int C, int HW);
bool bn_two_kernel_path(int N, int C, int HW, int single);
bool bn_pair_ok(int N, int C, int HW);
void bn_set_vec4(bool on);
}  // namespace ndp

// ---- embedding backward (embedding.hip) -------------------------------------------------
// grad_W [V, D] (dense, zeros for unreferenced rows and `pad`) from ids [T] int64 and
// grad_out [T, D]; perm [T], row_start [V] int32 scratch, row_cnt [V] int32 zeroed once
// at allocation (the kernels re-arm it).  Deterministic (fixed summation order).
namespace ndp {
// column sums of a row-major [M, N] fp32 matrix (N % 4 == 0): Linear bias gradient
// (linear.hip); part: colsum_chunks(M, N) * N floats of scratch
int colsum_chunks(int64_t M, int N);
void launch_colsum(const float* g, int64_t M, int N, float* part, float* out, hipStream_t s);
// dh = g * gelu'(h) (exact GELU) and out = column sums of dh, one pass over g / h (+ slab sum)
void launch_gelu_bwd_colsum(const float* g, const float* h, float* dh, int64_t M, int N, float* part, float* out,
                            hipStream_t s);
void launch_embedding_backward(const int64_t* ids, int T, const float* gout, int V, int D, int pad, int* perm,
                               int* row_start, int* row_cnt, float* gw, hipStream_t s);
}  // namespace ndp

// ---- fused softmax cross-entropy, mean reduction (loss.hip) -----------------------------
// x [B, K] logits, tgt [B] int64; dl [B, K] saved gradient (unscaled softmax - onehot),
// rowloss [B] scratch, loss / inv device scalars, ctr: one zeroed uint32 (re-armed by the kernel)
namespace ndp {
// acc (nullable): acc[0] += loss (a running loss sum)
void launch_ce_fwd(const float* x, const int64_t* tgt, int B, int K, int64_t ignore, float* dl, float* rowloss,
                   float* loss, float* inv, unsigned* ctr, hipStream_t s, float* acc = nullptr);
// the same with label smoothing eps and an optional second target per row (mixup / CutMix):
// row loss = (1 - eps) * (lam * nll(tgt) + (1 - lam) * nll(tgt_b)) + eps * (lse - mean_k x[k]);
// tgt_b / lam nullable together (then lam = 1); same scratch layout, launch_ce_bwd serves it
void launch_ce_soft_fwd(const float* x, const int64_t* tgt, const int64_t* tgt_b, const float* lam, float eps, int B,
                        int K, int64_t ignore, float* dl, float* rowloss, float* loss, float* inv, unsigned* ctr,
                        hipStream_t s, float* acc = nullptr);
// dx = dl * (g[0] * inv[0])
void launch_ce_bwd(const float* dl, const float* g, const float* inv, float* dx, int64_t n, hipStream_t s);
// fused evaluation metrics: state[4] (fp64) += [loss sum, valid rows, top-1 correct, top-k correct]
// over the rows whose target is not `ignore`; rowbuf [2 * B] scratch (row loss, then the target's
// rank as int32 bits), ctr: one zeroed uint32 (re-armed), pred (nullable) [B]: first-maximum index
void launch_cls_metrics(const float* x, const int64_t* tgt, int B, int K, int64_t ignore, int k, double* state,
                        float* rowbuf, unsigned* ctr, int64_t* pred, hipStream_t s);
}  // namespace ndp

// ---- global-norm gradient clipping (gradclip.hip) -----------------------------------------
// A SegEntry table over the gradients (src read, dst written, chunks = 1); partial [n_blocks]
// fp64 scratch, ctr: arrive_ctr_words(n_blocks) zeroed uint32 (the two-level arrival tickets of
// arrival.h, re-armed by the kernel), clip: the 16-byte ClipBlock.
namespace ndp {
struct ClipBlock {
  float norm;        // (float)(sqrt(sum v^2) / div) of the last run
  float coef;        // q = max_norm / (norm + 1e-6f);  q < 1 or NaN ? q : 1
  uint32_t clipped;  // runs whose coef != 1
  uint32_t steps;    // runs
};
void launch_grad_sqnorm(const SegEntry* entries, const int64_t* block_prefix, int n_entries, int64_t n_blocks,
                        double* partial, unsigned* ctr, ClipBlock* clip, float max_norm, float div, hipStream_t s);
// v *= clip->coef over the table; every workgroup returns at once when coef == 1
void launch_grad_scale(const SegEntry* entries, const int64_t* block_prefix, int n_entries, int64_t n_blocks,
                       const ClipBlock* clip, hipStream_t s);

// ---- exponential moving average of the weights (ema.hip) ----------------------------------
// A SegEntry table with src = live tensor, dst = shadow (chunks = 1; vec: both 16-byte aligned);
// ctr: arrive_ctr_words(n_blocks) zeroed uint32 (the two-level tickets of arrival.h, re-armed by
// the kernel), block: the 16-byte EmaBlock.
struct EmaBlock {
  float decay;       // d of the last run
  float weight;      // w = 1 - d of the last run
  uint32_t updates;  // runs so far
  uint32_t pad;
};
// s += w * (x - s) over the table with the decay of run block->updates (decay, warmup by value)
void launch_ema_update(const SegEntry* entries, const int64_t* block_prefix, int n_entries, int64_t n_blocks,
                       unsigned* ctr, EmaBlock* block, float decay, int warmup, hipStream_t s);
// x <-> s over the table, bitwise
void launch_ema_swap(const SegEntry* entries, const int64_t* block_prefix, int n_entries, int64_t n_blocks,
                     hipStream_t s);

// ---- AdamW (adamw.hip) ----------------------------------------------------------------------
// A SegEntry table from build_adamw_table (plan.h) with src = gradient, dst = parameter, stride =
// the entry's element offset into the moment arenas m / v, pad bit 0 = no decay, vec: all four
// streams 16-byte aligned; ctr: arrive_ctr_words(n_blocks) zeroed uint32 (re-armed by the kernel),
// block: the 16-byte AdamBlock, hyper: the device block [lr, weight_decay, 0, 0] (never null).
struct AdamBlock {
  float b1pow;     // beta1^steps as a running fp32 product
  float b2pow;     // beta2^steps
  uint32_t steps;  // launches so far
  uint32_t pad;
};
constexpr int kAdamNoDecay = 1;  // SegEntry.pad bit: the entry takes no weight decay
void launch_adamw_step(const SegEntry* entries, const int64_t* block_prefix, int n_entries, int64_t n_blocks,
                       unsigned* ctr, AdamBlock* block, const float* hyper, float* m, float* v, float beta1,
                       float beta2, float eps, float div, hipStream_t s);

// ---- AdamW inside the PowerSGD update pass (powersgd.hip) -----------------------------------
// The wide update launch (16 x 256 tiles, plan rank <= kUWideMaxRank, full layout only) with the
// element rule above in the place of momentum SGD: g := the decompressed value, div = 1, every
// matrix decays; the rank-1 tail takes g := buf / div and decays when decay_1d.  Modes 1 / 2 only,
// and mode 2 writes g = the decompressed, averaged gradient.  m is MatPtrs.mom / R1Step.mom, v lies
// v_delta elements behind it.  lr and wd always come from the hyper block (never null).
// A step may hold several of these launches (one per overlap group, then the rank-1 one): all read
// the block as it was before the step, and only the last one, advance != 0, draws the tickets (ctr:
// arrive_ctr_words(grid) zeroed uint32, re-armed) and has its last arriver write {p1, p2, steps + 1, 0}.
struct AdamArgs {
  AdamBlock* block;
  unsigned* ctr;
  int64_t v_delta;
  float beta1, beta2, eps;
  int decay_1d;
  int advance;
};
// workgroups of one launch_psgd_update_adam / launch_rank1_adam_step (what ctr is sized by)
int64_t psgd_update_adam_grid(int n_items, int64_t r1_n);
int64_t rank1_adam_grid(int64_t n);
void launch_psgd_update_adam(const MatGeom* geom, const MatPtrs* ptrs, const UItem* items, int n_items,
                             const float* p_hat, const float* q_sum, float q_div, float* q_warm, int mode,
                             int max_rank, hipStream_t s, float* p_prev, R1Step r1, const float* hyper, AdamArgs a);
void launch_rank1_adam_step(const float* buf, float div, float* mom, float* x, float* g, int64_t n, hipStream_t s,
                            const float* hyper, AdamArgs a);
}  // namespace ndp

// ---- batch assembly from byte images (image_batch.hip) ------------------------------------
// src [N, C, 32, 32] bytes, labels [N], idx [m]; out [B, C, 32, 32] fp32 and out_target [B] are
// written in full: rows < m gathered, normalised (fmaf(byte, scale[c], shift[c])) and optionally
// cropped / flipped by a hash of (seed, epoch, index); rows >= m and rows whose index is outside
// [0, N) are zero with target = pad_target, and the latter store 1 into *err.
namespace ndp {
constexpr int kImageMaxC = 8;
struct ImageNorm {
  float scale[kImageMaxC];
  float shift[kImageMaxC];
};
void launch_image_batch(const uint8_t* src, const int64_t* labels, const int64_t* idx, float* out,
                        int64_t* out_target, int m, int B, int64_t N, int C, const ImageNorm& norm, int pad,
                        int flip_on, uint32_t seed, uint32_t epoch, int64_t pad_target, int* err, hipStream_t s);
// the same batch with mixup / CutMix against the reversed batch (row b with row m - 1 - b): also
// writes out_target_b [B] (the partner's label, the own one when unmixed) and out_lam [B] (the own
// label's weight, 1 when unmixed).  mode: 1 mixup, 2 CutMix, 3 either by a hash bit; thr =
// int(mix_prob * 2^24): a row is mixed when its 24-bit hash draw is below thr.
void launch_image_mix_batch(const uint8_t* src, const int64_t* labels, const int64_t* idx, float* out,
                            int64_t* out_target, int64_t* out_target_b, float* out_lam, int m, int B, int64_t N,
                            int C, const ImageNorm& norm, int pad, int flip_on, uint32_t seed, uint32_t epoch,
                            int64_t pad_target, int* err, int mode, uint32_t thr, hipStream_t s);
}  // namespace ndp

// ---- fused residual add + LayerNorm over the last dim (layernorm.hip) --------------------
namespace ndp {
bool ln_supported(int D);  // D in {256, 512, 768, 1024}
// hash dropout fused into the LayerNorm: mode 0 none, 1 on a (before the residual add; the
// backward also writes da = dropout'(dx)), 2 on the output; keep = hash >= thr (= p * 2^32)
struct LnDrop {
  const int32_t* seed;
  uint32_t thr;
  float scale;  // 1 / (1 - p)
  int mode;
  float* da;
};
// y = LN(a (+ b)) * gamma + beta; s = a (+ b), mean / rstd [R] saved for backward
void launch_ln_fwd(const float* a, const float* b, const float* gamma, const float* beta, float* y, float* s,
                   float* mean, float* rstd, int64_t R, int D, float eps, hipStream_t st, const LnDrop& dp);
int ln_bwd_wgs(int64_t R);
// dx [R, D]; part: ln_bwd_wgs(R) * 2D floats of scratch; dgb: [dgamma | dbeta] (2D floats)
void launch_ln_bwd(const float* dy, const float* s, const float* mean, const float* rstd, const float* gamma,
                   float* dx, float* part, float* dgb, int64_t R, int D, hipStream_t st, const LnDrop& dp);
}  // namespace ndp

// ---- convolutions, NCHW fp32 (conv.hip) -------------------------------------------------
namespace ndp {
struct ConvGeom {
  int32_t C, H, W;        // input channels / spatial
  int32_t Co, KH, KW;     // output channels / kernel
  int32_t stride, pad;
  int32_t OH, OW;         // output spatial
};
// Wt_big [Co*OH*OW, C*H*W] <- W [Co, C, KH, KW]  (transposed Toeplitz form of a small-spatial conv)
void launch_toeplitz_expand(const float* w, float* wb, const ConvGeom& g, hipStream_t s);
// several layers' W_big^T in one launch (by-value kernel arguments)
constexpr int kMaxExpand = 24;
struct ExpandBatch {
  const float* w[kMaxExpand];
  float* wt[kMaxExpand];
  ConvGeom g[kMaxExpand];
  int64_t end[kMaxExpand];  // inclusive prefix sums of the W_big^T row counts N = Co*OH*OW
  int n;
};
void launch_toeplitz_expand_many(const ExpandBatch& b, hipStream_t s);
// several layers' grad-W folds in one launch
struct FoldBatch {
  const float* dwt[kMaxExpand];
  float* dw[kMaxExpand];
  ConvGeom g[kMaxExpand];
  int64_t end[kMaxExpand];  // inclusive prefix sums of the (co, ci) pair counts Co*C
  int n;
};
void launch_toeplitz_fold_many(const FoldBatch& b, hipStream_t s);
// several grad-W slab sums in one launch: dw_e = sum over slices of part_e (numel % 4 == 0)
struct SlabBatch {
  const float* part[kMaxExpand];
  float* dw[kMaxExpand];
  int64_t numel[kMaxExpand];
  int slices[kMaxExpand];
  int64_t end[kMaxExpand];  // inclusive prefix sums of blocks (64 floats per block)
  int n;
  int nt;  // non-temporal slab loads (set by launch_slab_sum_many)
};
void launch_slab_sum_many(const SlabBatch& b, hipStream_t s);
// both of the above in one launch (the end-of-backward grad-W finish)
void launch_gradw_finish(const SlabBatch& sb, const FoldBatch& fb, hipStream_t s);
// dW [Co, C, KH, KW] <- fold of dWt_big [Co*OH*OW, C*H*W]  (fixed-order sum, deterministic)
void launch_toeplitz_fold(const float* dwb, float* dw, const ConvGeom& g, hipStream_t s);
// direct fp32-MFMA convolutions: the shape classes with a kernel (C, Co % 64 == 0, the stem C = 3; conv_plan
// returns the values to Python).  ResNet layer1 / layer2 3x3 s1 p1 on 8x8 / 4x4 maps, layer2's first conv 3x3 s2
// p1 8x8 -> 4x4, the 7x7 s2 p3 stem 32x32 -> 16x16, the layer2 / layer3 downsamples 1x1 s2 p0 on 8x8 / 4x4
enum ConvClass : int {
  kConvNone = -1, kConv3x3Map8 = 0, kConv3x3Map4 = 1, kConv3x3S2 = 2, kConvStem = 3, kConv1x1S2Map8 = 4, kConv1x1S2Map4 = 5
};
// What the three launchers below do for (geometry, batch): computed once per call by conv_make_plan
// (the Winograd and stem-split switches are mutable at run time), checked against the tensors by
// the caller and handed to the launcher.  cls == kConvNone (no direct kernel) leaves the defaults.
// The forward / grad-x kernels need B % fwd_imgs == 0, the grad-W B % wgrad_imgs == 0.
struct ConvPlan {
  int cls = kConvNone;
  int fwd_imgs = 0, wgrad_imgs = 0;  // images per forward / grad-x workgroup, per grad-W slice
  bool dgrad_direct = false;         // the class has a grad-x kernel
  // split-K factor (1 = none) of the forward / grad-x kernel; with ksplit > 1 the launchers need
  // `part` scratch of ksplit slabs: B * Co * OH * OW floats forward, dgrad_slab floats grad-x
  // (B * C * H * W; the stride-2 1x1 classes B * C * OH * OW, their product before the even-pixel
  // scatter, which only the launcher can sum: dgrad_defer_ok false)
  int fwd_ksplit = 1, dgrad_ksplit = 1;
  int64_t dgrad_slab = 0;
  bool dgrad_defer_ok = false;
  bool fwd_wino = false, dgrad_wino = false;  // the launch takes the Winograd kernel (given wino_u)
  int fwd_psplit = 1;                         // output-row blocks per image (the stem forward)
  int fwd_stats_slices = 0, dgrad_stats_slices = 0;  // BatchNorm statistics partials of the epilogue (0 = none)
};
ConvPlan conv_make_plan(const ConvGeom& g, int B);
// defer: with split-K, skip the slab sum and return the number of slabs left in `part`
// (compact output layout, slab = numel(out)); returns 1 when `y` / `dx` holds the result
// stats (nullable; only where the plan has fwd_stats_slices > 0): BatchNorm partial sums of y from the
// epilogue, [Co][S][2] fp64 (sum, sum of squares per channel and batch tile)
// BatchNorm partial sums from the epilogue (out != nullptr): forward mode (bx == nullptr) sums
// the output v and v^2 for the BN that consumes it; backward mode sums dz = v * (by > 0) and
// dz * (bx - mean) * invstd for the BN whose output gradient v is (bx / by: that BN's input and
// ReLU output, mean / invstd its saved statistics) — the BN backward's statistics pass
struct ConvBnStats {
  double* out;
  const float* bx;
  const float* by;
  const float* mean;
  const float* invstd;
};
// wino_u (nullable): the conv's Winograd weight transforms (launch_wino_weights: forward + grad-x
// layouts, 32 * Co * C floats) when the plan says fwd_wino / dgrad_wino — the launch then runs the Winograd kernel
// pair: a downsample conv (kConv1x1S2Map8) forward may be held back and launched together with the next
// kConv3x3S2 forward of the same input (ds_fwd_pair_kernel); conv_flush_pending_fwd() launches it alone
int launch_conv_fwd(const float* x, const float* w, float* y, int B, const ConvGeom& g, const ConvPlan& p, float* part,
                    hipStream_t s, bool defer = false, double* stats = nullptr, float* wino_u = nullptr,
                    bool pair = false);
void conv_flush_pending_fwd();
// stem forward output-row blocks per image (A/B override 1 / 2 / 4, 0 = by batch)
void conv_set_stem_psplit(int p);
// addend (nullable, 3x3 classes): dx += addend in the epilogue / split-K sum; with defer the
// slabs are left unsummed and the consumer adds the addend after them (launch_bn_bwd dyadd)
// bst (nullable; the layer1 3x3 class, unsplit: dgrad_stats_slices > 0): backward-mode BN partial
// sums of dx for the BN whose output gradient dx is
int launch_conv_dgrad(const float* dy, const float* w, float* dx, int B, const ConvGeom& g, const ConvPlan& p,
                      float* part, hipStream_t s, const float* addend = nullptr, bool defer = false,
                      const ConvBnStats* bst = nullptr, float* wino_u = nullptr);
// Winograd F(2x2, 3x3) path of the 8x8 3x3 classes (winograd.hip): whether a launch can take it,
// and the U scratch it needs (16 * inC * outC floats)
bool wino_ok(int inC, int outC, int B, int H, int W, int ks);
bool wino_disabled();
void wino_set_enabled(bool on);
int wino_imgs(int H);
int64_t wino_u_numel(int inC, int outC);
void launch_wino_weights(const float* w, float* u, int Co, int C, hipStream_t s);
bool wino_wgrad_red(int B, int imgs);
bool wino_wgrad_ok(int C, int Co, int H);
void launch_wino_wgrad(const float* x, const float* dy, float* part, int B, int C, int Co, int H, int imgs,
                       hipStream_t s);
// grad-W operand pipelining (fusion `wgrad_pipe`; A/B overrides): the layer1 Winograd grad-W's LDS
// prefetch of the next image, and the layer2 3x3 direct grad-W's images per stage (0 = auto, 1 = the
// one-image loop, 4 = staged where the slice allows; 2-image stages measured slower and are not built)
bool wgrad_pipe_off();  // NDP_FUSION_OFF=wgrad_pipe
void wino_set_wgrad_prefetch(bool on);
bool conv_set_wgrad_stage(int n);  // false: a value that is not built (nothing changed)
int64_t conv_pair_launches();
// the streamed forward / grad-x bodies of the 1x1 stride-2 classes (fusion `ds_stream`, ds_stream.h):
// 1 = on, 0 = off (conv_fwd_body on the 8-channel chunk tiles), -1 = by NDP_FUSION_OFF (the default)
void conv_set_ds_stream(int on);
// several layers' transforms in one launch (ops/conv.py WinoBank)
constexpr int kMaxWino = 16;
struct WinoBatch {
  const float* w[kMaxWino];
  float* u[kMaxWino];
  int Co[kMaxWino];
  int C[kMaxWino];
  int end[kMaxWino];  // inclusive prefix sums of the (Co / 16) * (C / 16) block counts
  int n;
};
void launch_wino_weights_many(const WinoBatch& b, hipStream_t s);
void launch_wino_conv(const float* x, const float* u, float* y, int B, int inC, int outC, int H, bool transw,
                      int iups, const float* addend, const ConvBnStats& st, int ks, float* part, hipStream_t s);
// out[i] = sum_{z < nslab} part[z * n + i] (+ addend[i]) in z order (n % 4 == 0), same order as
// the split-K sums; out may alias addend
void launch_slab_sum(const float* part, float* out, int64_t n, int nslab, hipStream_t s,
                     const float* addend = nullptr);
// part: (B / p.wgrad_imgs) * Co*C*KH*KW floats of scratch.  pair: a layer1 Winograd
// grad-W into `part` (dw == nullptr) may be held back and launched together with the next
// launch_conv_dgrad of the same dY (one wino_bwd_pair_kernel launch); conv_flush_pending() launches
// a held-back grad-W on its own (the caller's end of the conv backward)
void launch_conv_wgrad(const float* x, const float* dy, float* part, float* dw, int B, const ConvGeom& g,
                       const ConvPlan& p, hipStream_t s, bool pair = false);
void conv_flush_pending();
void launch_wino_bwd_pair(const float* dy, const float* u, float* dx, int B, int inC, int outC, const float* addend,
                          const ConvBnStats& st, int ks, float* part_x, const float* x, float* part_w, int imgs,
                          hipStream_t s);

// ---- strided / tabled implicit-GEMM convolutions (tgemm.hip) ------------------------------
// operand index i -> element offset (i >> sh) * so + (i & (2^sh - 1)) * si
struct TgIndex {
  int64_t so, si;
  int32_t sh, pad;
};
// C[m, n] (+)= sum_k A[m, k] B[k, n];  A(m,k) = a[am(m) + ak(k)], B(k,n) = b[bk(k) + bn(n)];
// C(m,n) = c[cm(m) + cn(n)]; split z writes part + z * slab when part != null
struct TgArgs {
  const float* a;
  const float* b;
  float* c;
  float* part;
  const float* addend;  // C += addend (same offsets; may alias c); single-split launches only
  TgIndex am, ak, bk, bn, cm, cn;
  int32_t M, N, K, kchunk;
  int64_t slab;
};
constexpr int TG_POINTWISE = 0;  // 1x1 stride-1, power-of-two map of >= 2 pixels
int tg_class(const ConvGeom& g);
// the GEMM description of direction dir (pointers null) + the load mappings of its launch
TgArgs tg_args(const ConvGeom& g, int B, int dir, bool* akf, bool* bnf);
// split-K slabs of direction dir (0 fwd, 1 grad-x, 2 grad-W) for batch B (1 = no scratch)
int tg_splits(const ConvGeom& g, int B, int dir);
// what run() launches for a described GEMM and `splits` allotted slabs: the load widths of A / B
// (4 = 16-B loads; only the 16-B alignment of a.a / a.b is read), the k range of one split and
// the slabs left after rounding it to whole k-tiles (<= splits)
struct TgLaunch {
  int wa, wb, slabs, kchunk;
};
TgLaunch tg_launch(const TgArgs& a, bool akf, bool bnf, int splits);
// defer: leave the split-K slabs in part and return their count (1 = y / dx final)
int launch_tg_fwd(const float* x, const float* w, float* y, int B, const ConvGeom& g, float* part, hipStream_t s,
                  bool defer = false);
// addend (nullable, may alias dx): dx = grad-x + addend (never deferred)
int launch_tg_dgrad(const float* dy, const float* w, float* dx, int B, const ConvGeom& g, float* part,
                    hipStream_t s, const float* addend = nullptr, bool defer = false);
// POINTWISE: out = dW; SMALL: out = dWbig^T [Co*OH*OW, C*H*W] (fold with toeplitz_fold).
// defer: leave the split-K slabs in part, return their count (1 = out final)
int launch_tg_wgrad(const float* x, const float* dy, float* out, int B, const ConvGeom& g, float* part,
                    hipStream_t s, bool defer = false);
}  // namespace ndp

// ---- fused fp32 attention, q/k/v/o [B, S, H, 64] (attention.hip) ------------------------
namespace ndp {
// mask: [B, S] int32 (nonzero = attend) or null; lse: [B, H, S]; p_drop in [0, 1);
// seed: device int32[1] read by the kernels (so a replayed hipGraph sees fresh seeds)
void launch_attn_fwd(const float* q, const float* k, const float* v, const int32_t* mask, float* o, float* lse,
                     int B, int S, int H, float scale, const int32_t* seed, double p_drop, hipStream_t s,
                     int64_t ldq = 0);
// ldq: token row stride of q / k / v (and dq / dk / dv): 0 = H*64 (contiguous), 3*H*64 for
// views into a packed [B, S, 3, H, 64] QKV projection.  delta: [B, H, S] scratch
void launch_attn_bwd(const float* q, const float* k, const float* v, const int32_t* mask, const float* o,
                     const float* dout, const float* lse, float* delta, float* dq, float* dk, float* dv, int B,
                     int S, int H, float scale, const int32_t* seed, double p_drop, hipStream_t s,
                     int64_t ldq = 0);
}  // namespace ndp

// ---- max-pool 2-D, NCHW fp32, deterministic gather backward (pool.hip) ---------------
namespace ndp {
struct PoolGeom {
  int32_t H, W, OH, OW;
  int32_t KH, KW, stride, pad;
};
// idx: uint8 window offset (kh*KW + kw) of each output's maximum
void launch_maxpool_fwd(const float* x, float* y, uint8_t* idx, int planes, const PoolGeom& g, hipStream_t s);
// BatchNorm backward statistics from the pool backward (stats != nullptr; ResNet stem tail, the
// BN output never stored): per plane (n, c) the sums of dz = dx * mask(x) and dz * xhat into
// stats[(c * N + n) * 2], the mask recomputed from x as bn_relu_maxpool computed its output
struct PoolBnStats {
  const float* x;
  const float* gamma;
  const float* beta;
  const float* mean;
  const float* invstd;
  double* stats;
  int C, N;
};
bool maxpool_bwd_bnstats_ok(const PoolGeom& g);
// the stem BN input gradient straight from the pooled gradient (batchnorm.hip): 16x16 -> 8x8 maps,
// statistics [C][N][2] from the statistics-only pool backward
void launch_stem_pool_bwd_apply(const float* dy, const uint8_t* idx, const float* x, const float* gamma,
                                const float* beta, const float* save_mean, const float* save_invstd,
                                const double* stats, float* dx, float* dgamma, float* dbeta, int N, int C, int H,
                                int W, hipStream_t s);
void launch_maxpool_bwd(const float* dy, const uint8_t* idx, float* dx, int planes, const PoolGeom& g,
                        hipStream_t s,
                        const PoolBnStats& bs = PoolBnStats{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0});
}  // namespace ndp
