// Launcher declarations for the gfx950 kernel library.
// Raw-pointer interfaces; the torch glue lives in bindings.cpp only.
#pragma once

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdlib>

using bf16_t = unsigned short;  // raw bf16 bits at the ABI boundary

// ---- counter-RNG dropout parameters (chain: dta_common.h) ------------------
// rng: device uint64 step counter; site: per-call-site salt; thr16 == 0
// disables dropout.
struct DropParams {
  const unsigned long long* rng = nullptr;
  unsigned long long site = 0;
  unsigned int thr16 = 0;
  float inv_keep = 1.0f;
};
// The one place p is quantised: thr16 = min(ceil(p * 2^16), 2^16 - 1) and
// inv_keep is the reciprocal of the REALIZED keep probability, so the
// expectation stays unbiased.
inline void dta_drop_quantize(double p, DropParams& d) {
  const double full = 65536.0;
  d.thr16 = (unsigned int)std::fmin(std::ceil(p * full), full - 1.0);
  d.inv_keep = float(full / (full - double(d.thr16)));
}

// ---- elementwise ----------------------------------------------------------
void launch_gelu_fwd(const bf16_t* x, bf16_t* y, int64_t n, hipStream_t s);
void launch_gelu_bwd(const bf16_t* dy, const bf16_t* x, bf16_t* dx, int64_t n,
                     hipStream_t s);
void launch_gelu_fwd_f32(const float* x, float* y, int64_t n, hipStream_t s);
void launch_gelu_bwd_f32(const float* dy, const float* x, float* dx,
                         int64_t n, hipStream_t s);
void launch_swiglu_fwd(const bf16_t* g, const bf16_t* u, bf16_t* y, int64_t n,
                       hipStream_t s);
void launch_swiglu_bwd(const bf16_t* dy, const bf16_t* g, const bf16_t* u,
                       bf16_t* dg, bf16_t* du, int64_t n, hipStream_t s);
// counter-based dropout (fwd and bwd are the same masked scale; the mask
// is regenerated, never stored). rng: device uint64 step counter.
void launch_dropout(const bf16_t* x, bf16_t* y, int64_t n,
                    const DropParams& drop, hipStream_t s);
void launch_rng_tick(unsigned long long* ctr, hipStream_t s);
// dst (bf16 grad view) += src (fp32): replaces cast + autograd-add pairs
void launch_accum_f32_bf16(bf16_t* dst, const float* src, int64_t n,
                           hipStream_t s);

// ---- flat-plane ops -------------------------------------------------------
void launch_delta_sub(const float* w, const float* base, float* out,
                      int64_t n, hipStream_t s);
void launch_axpy(float* w, const float* x, float alpha, int64_t n,
                 hipStream_t s);
void launch_nan_any(const float* x, int64_t n, int* flag, hipStream_t s);
void launch_l2norm_sq(const float* x, int64_t n, float* out, hipStream_t s);
// beta1/beta2 stay double up to here: 1 - beta and the bias corrections
// 1 - beta^t are formed in double and rounded once (in fp32, 1 - 0.999f is
// 1.3e-5 off 0.001, and v with it)
void launch_adamw(float* master, const void* grad, bool grad_is_bf16,
                  float* m, float* v, bf16_t* out_bf16, int step,
                  const float* bc_p, float lr, double beta1, double beta2,
                  float eps, float wd, int64_t n, hipStream_t s);
void launch_adamw_tick(int* t, float* bc, double beta1, double beta2,
                       hipStream_t s);
// Guarded step (control block layout: adamw.hip header). The norm pass
// stores dta_gradnorm_blocks(n, bf16) fp32 partials, every one of them, so
// part needs no zero-fill; grad must be 16 B aligned.
int dta_gradnorm_blocks(int64_t n, bool grad_is_bf16);
void launch_gradnorm_part(const void* grad, bool grad_is_bf16, float* part,
                          int64_t n, hipStream_t s);
enum LrSchedule { LR_CONSTANT = 0, LR_LINEAR = 1, LR_COSINE = 2 };
// part null (nparts 0): no norm was taken; the kernel ticks and evaluates
// the schedule only. max_norm <= 0: no clipping. linear/cosine need
// total_steps > warmup_steps >= 0.
struct StepCtlArgs {
  const float* part;
  int nparts;
  float* ctl_f;   // fp32[6]
  int* ctl_i;     // int32[4]
  double beta1, beta2;
  float max_norm;
  int skip_nonfinite;
  int schedule;   // LrSchedule
  double lr_max, min_lr;
  int warmup_steps, total_steps;
};
void launch_step_ctl(const StepCtlArgs& a, hipStream_t s);
void launch_adamw_guarded(float* master, const void* grad, bool grad_is_bf16,
                          float* m, float* v, bf16_t* out_bf16,
                          const float* ctl_f, const int* ctl_i, double beta1,
                          double beta2, float eps, float wd, int64_t n,
                          hipStream_t s);
// Column reductions run in two phases: a producer writes a [stripes, ld]
// fp32 partial panel, launch_colred_finish folds it over the stripes in a
// fixed order and writes every output once. Per panel k: dstk non-null
// accumulates into a bf16 destination of any alignment,
// dstk = bf16(float(dstk) + sum); else outk [cols] fp32 is stored (it need
// not be zeroed). p1 null: one panel. ld % 4 == 0, cols <= ld.
struct ColFinishArgs {
  const float *p0, *p1;
  float *out0, *out1;
  bf16_t *dst0, *dst1;
  int stripes, cols, ld;
};
void launch_colred_finish(const ColFinishArgs& a, hipStream_t s);
// panel row length of launch_colsum: cols, padded to 4 where cols % 8 != 0
// (those shapes take a one-column-per-lane producer)
inline int dta_colred_ld(int cols) { return (cols + 3) / 4 * 4; }
// out[c] (or dst[c] +=) sum_r x[r,c]; part: [stripes, dta_colred_ld(cols)]
void launch_colsum(const bf16_t* x, float* part, float* out, bf16_t* dst,
                   int64_t rows, int cols, int stripes, hipStream_t s);
// dx = bf16(dy * gelu'(x)) and the column sums of dx in one pass over
// [rows, cols], cols % 8 == 0; part: [stripes, cols]; out/dst as above
void launch_gelu_bwd_colsum(const bf16_t* dy, const bf16_t* x, bf16_t* dx,
                            float* part, float* out, bf16_t* dst,
                            int64_t rows, int cols, int stripes,
                            hipStream_t s);
// launch config for the two-phase column reductions (colsum / norm dγdβ):
// block sized to the active lane count (cols/8 threads, 64-multiple),
// stripe count targeting ~512 blocks of 256-thread-equivalents.
struct ColRedCfg { int threads; int gx; int stripes; };
inline ColRedCfg dta_colred_cfg(int64_t rows, int cols) {
  const int lanes = cols / 8;
  // balance lanes across gx blocks (a 256-thread split left trailing
  // blocks ~12% occupied at lanes=288, e.g. the qkv dbias shape)
  const int gx = lanes > 0 ? (lanes + 255) / 256 : 1;   // cols < 8: one block
  int threads = ((lanes + gx - 1) / gx + 63) / 64 * 64;
  if (threads < 64) threads = 64;
  // target ~1024 blocks of 256-thread-equivalents (measured best; halving
  // it cost colsum_part 24us -> 33us avg)
  int64_t st = (1024 * 256) / (int64_t(gx) * threads);
  const int64_t mx = (rows + 31) / 32;
  if (st > mx) st = mx;
  if (st < 1) st = 1;
  return ColRedCfg{threads, gx, int(st)};
}
inline int dta_colred_stripes(int64_t rows, int cols) {
  return dta_colred_cfg(rows, cols).stripes;
}
// row stripes of launch_gelu_bwd_colsum: 1.5 x the colsum value. Its loop
// body is ~10x longer per row than colsum_part_k's, and at [65536, 3072]
// the 682 stripes of dta_colred_cfg are 4 waves per SIMD: measured 0.301 ms
// there, 0.283 at 1024, 0.281 at 2048 (tools/bias_grad_ab.py
// --gelu-stripes), against 4 MB more panel per 341 stripes.
inline int dta_gelu_colsum_stripes(int64_t rows, int cols) {
  const int64_t st = int64_t(dta_colred_stripes(rows, cols)) * 3 / 2;
  const int64_t mx = (rows + 31) / 32;
  return int(st > mx ? (mx > 0 ? mx : 1) : st);
}

// ---- merge plane ----------------------------------------------------------
void launch_weighted_merge(const float* base, const float* deltas,  // [N,P]
                           const float* W,                          // [N,S]
                           const int64_t* offsets, int n_models, int n_segs,
                           int64_t P, float* out, hipStream_t s);
// chunks: [n_chunks,3] int64 (start,end,seg) rows, none crossing a segment
void launch_grad_merge_weights(const void* g, bool g_is_bf16,
                               const float* base, const float* deltas,
                               const float* merged, const int64_t* chunks,
                               int n_models, int n_chunks, int64_t P,
                               float* grad_w,  // [N,S] pre-zeroed
                               int n_segs, hipStream_t s);
// Gathered deltas kept in their wire form. bf16: data [N, ld = P]. int8:
// data [N, ld = nb*block] codes, scales [N, nb] fp32, block == 1 << shift;
// element e of row i is float(code) * scales[i, e >> shift], one rounded
// fp32 multiply. The packed kernels produce what the fp32 ones produce on
// the dequantised rows, bit for bit (grad_W keeps the fp32 kernel's
// summation order). Merge and axpy read 4 elements per lane: base/out/w must
// be 16 B aligned and data 8 B; bf16 with P % 4 != 0 falls back to one
// element per lane.
enum DeltaKind { DELTA_F32 = 0, DELTA_BF16 = 1, DELTA_I8 = 2 };
struct PackedView {
  const void* data;
  const float* scales;   // int8 only
  int64_t ld;            // elements per row of data
  int64_t nb;            // scales per row (int8 only)
  int shift;             // log2(block) (int8 only)
  int kind;              // DeltaKind
};
constexpr int DTA_MERGE_MAX_MODELS = 32;   // miners per node (8 GPUs typical)
constexpr size_t DTA_MERGE_LDS_LIMIT = 64 * 1024;   // offsets + W, per block
// dynamic LDS weighted_merge needs for its offsets and W cache
size_t dta_merge_shmem(int n_models, int n_segs);
void launch_weighted_merge_packed(const float* base, const PackedView& d,
                                  const float* W, const int64_t* offsets,
                                  int n_models, int n_segs, int64_t P,
                                  float* out, hipStream_t s);
void launch_grad_merge_weights_packed(const void* g, bool g_is_bf16,
                                      const float* base, const PackedView& d,
                                      const float* merged,
                                      const int64_t* chunks, int n_models,
                                      int n_chunks, int64_t P, float* grad_w,
                                      int n_segs, hipStream_t s);
// Robust merge: out[e] = base[e] + mean of the sorted positions trim ..
// n_models-1-trim of the n_models values delta_i[e] (0 <= 2*trim < n_models;
// trim = (n_models-1)/2 is the median), and outside[i] += the number of
// elements at which row i lies strictly outside that kept interval. The
// order is total: -inf < .. < -0 < +0 < .. < +inf < NaN. d: fp32 (kind
// DELTA_F32, data [N, ld = P]), bf16 or int8. Bit-equal to the CPU path of
// ops.trimmed_merge, independent of the row order. outside: int64
// [n_models], zero-filled by the caller, integer atomics only; null: no
// counts. The rows are padded to dta_trimmed_pad(n_models) sort keys per
// element; dta_trimmed_vec elements per lane: where that is 4, base and out
// must be 16 B aligned and data 16 B (fp32), 8 B (bf16) or 4 B (int8).
inline int dta_trimmed_pad(int n_models) {
  return n_models <= 4 ? 4 : n_models <= 8 ? 8 : n_models <= 16 ? 16 : 32;
}
inline int dta_trimmed_vec(int kind, int n_models, int64_t P) {
  // 32 keys, their sorted copy and 32 counters per ELEMENT: one per lane
  if (dta_trimmed_pad(n_models) == 32) return 1;
  // as the packed merge: a row start must be aligned, int8 rows are padded
  return (kind == DELTA_I8 || P % 4 == 0) ? 4 : 1;
}
void launch_trimmed_merge(const float* base, const PackedView& d,
                          int n_models, int trim, int64_t P, float* out,
                          int64_t* outside, hipStream_t s);
// elements one sweep of its capped grid covers; more take the grid-stride loop
int64_t dta_trimmed_sweep(int kind, int n_models, int64_t P);
// w += alpha * row `row` of d, dequantised in registers
void launch_axpy_packed(float* w, const PackedView& d, int row, float alpha,
                        int64_t P, hipStream_t s);
// Blockwise int8 of d = w - base (base null: of w), bit-equal to
// comm.quantize_blockwise_int8 on the CPU. codes [nb*block], scales [nb],
// nb = ceil(P / block); block a power of two in [DTA_QUANT_MIN_BLOCK,
// DTA_QUANT_MAX_BLOCK]; w, base and codes 16 B aligned.
constexpr int DTA_QUANT_MIN_BLOCK = 16;
constexpr int DTA_QUANT_MAX_BLOCK = 16384;
void launch_delta_quantize_int8(const float* w, const float* base, int64_t P,
                                int block, int64_t nb, signed char* codes,
                                float* scales, hipStream_t s);
// Blockwise top-k with error feedback of d = (w - base) + residual_in (base
// and residual_in may be null), bit-equal to comm.topk_compress_blockwise on
// the CPU. entries [nb*k] int32, (idx << 16) | bf16 bits, ascending idx per
// block; residual_out [P] (null: not written; may alias residual_in). block
// a power of two in [DTA_TOPK_MIN_BLOCK, DTA_TOPK_MAX_BLOCK], k % 4 == 0,
// 4 <= k <= block / 4; every pointer 16 B aligned. No host sync.
constexpr int DTA_TOPK_MIN_BLOCK = 1024;
constexpr int DTA_TOPK_MAX_BLOCK = 16384;
void launch_delta_topk(const float* w, const float* base,
                       const float* residual_in, float* residual_out,
                       int64_t P, int block, int k, int64_t nb, int* entries,
                       hipStream_t s);
// Gathered top-k deltas: data [N, ld = nb*k] entries, block == 1 << shift.
// Entries whose element lies past P are skipped. Each consumer produces what
// its fp32 kernel produces on the densified rows, bit for bit (axpy: as
// numbers; it touches only the elements on the support). base/out/w 16 B
// aligned.
struct TopkView {
  const int* data;
  int64_t ld;
  int shift;
  int k;
};
// dynamic LDS of the merge: two tiles of min(block, 4096) fp32 + offsets + W
size_t dta_topk_merge_shmem(int n_models, int n_segs, int block);
void launch_weighted_merge_topk(const float* base, const TopkView& d,
                                const float* W, const int64_t* offsets,
                                int n_models, int n_segs, int64_t P,
                                float* out, hipStream_t s);
void launch_grad_merge_weights_topk(const void* g, bool g_is_bf16,
                                    const float* base, const TopkView& d,
                                    const float* merged,
                                    const int64_t* chunks, int n_models,
                                    int n_chunks, int64_t P, float* grad_w,
                                    int n_segs, hipStream_t s);
void launch_axpy_topk(float* w, const TopkView& d, int row, float alpha,
                      int64_t P, hipStream_t s);

// ---- norms ----------------------------------------------------------------
// dγ/dβ partial-panel geometry: for cols <= 1024 the partials come from
// the dx kernel itself (register accumulation, one panel row per
// (block, wave)); wider rows use the standalone column-reduction kernel.
constexpr int DTA_NORM_ROW_WAVES = 4;
inline bool dta_norm_fused_dwdb(int cols) {
  // NEGATIVE RESULT (r02, same-box A/B): folding the dγ/dβ partials into
  // the dx kernel removes the 0.9 ms/step standalone partial pass but the
  // 16·ITERS accumulator VGPRs double the dx kernel itself (75 → 195 µs
  // per call; whole step 76.9 vs 75.2 ms). Register pressure beats the
  // saved read on this streaming kernel. Opt-in via DTA_NORM_FDW=1.
  static const bool en = [] {
    const char* e = ::getenv("DTA_NORM_FDW");
    return e && e[0] == '1';
  }();
  return en && cols <= 1024;
}
inline int dta_norm_bwd_grid(int64_t rows) {
  int64_t want = (rows + DTA_NORM_ROW_WAVES - 1) / DTA_NORM_ROW_WAVES;
  return int(want < 4096 ? (want > 0 ? want : 1) : 4096);
}
inline int dta_norm_bwd_stripes(int64_t rows, int cols) {
  // fused path: one panel row per BLOCK (waves LDS-combined in-kernel)
  return dta_norm_fused_dwdb(cols) ? dta_norm_bwd_grid(rows)
                                   : dta_colred_stripes(rows, cols);
}
// Row-width limits of the register-resident kernels: the forward is
// instantiated up to 16 iterations of 64 lanes x 8 columns, the backward
// up to 8 (a 16-iteration backward would hold 3*16*8 fp32 per lane).
constexpr int DTA_NORM_FWD_MAX_COLS = 8192;
constexpr int DTA_NORM_BWD_MAX_COLS = 4096;
// One argument struct per direction, filled once in the bindings.
// rms: RMSNorm instead of LayerNorm; b, mean, db and pdb are then null.
// res/sum_out: optional fused residual (sum = bf16(x+res) feeds both the
// statistics and the ongoing stream); ds: optional additive gradient on
// the sum stream folded into dx.
// drop: counter-RNG dropout fused onto the incoming residual branch
// (thr16 == 0 disables; requires res). Backward emits the branch
// gradient dres = dx ⊙ mask/(1-p) when enabled.
struct NormFwdArgs {
  const bf16_t *x, *res;
  bf16_t* sum_out;
  const bf16_t *w, *b;
  bf16_t* y;
  float *mean, *rstd;
  int64_t rows;
  int cols;  // % 8 == 0, <= DTA_NORM_FWD_MAX_COLS
  float eps;
  DropParams drop;
  bool rms;
};
// pdw/pdb: [stripes, cols] fp32 workspaces (dta_norm_bwd_stripes rows) of
// the two-phase dγ/dβ column reduction; launch_colred_finish folds them
// into dw/db (fp32 [cols], stored) or, where dw_dst/db_dst is non-null,
// accumulates into that bf16 destination instead. Both repeat bit for bit
// (the opt-in DTA_NORM_FDW panel is itself built with LDS atomics).
struct NormBwdArgs {
  const bf16_t *dy, *ds, *x, *w;
  const float *mean, *rstd;
  bf16_t *dx, *dres;
  float *dw, *db, *pdw, *pdb;
  bf16_t *dw_dst, *db_dst;
  int stripes;
  int64_t rows;
  int cols;  // % 8 == 0, <= DTA_NORM_BWD_MAX_COLS
  DropParams drop;
  bool rms;
};
void launch_norm_fwd(const NormFwdArgs& a, hipStream_t s);
void launch_norm_bwd(const NormBwdArgs& a, hipStream_t s);

// ---- fused cross entropy --------------------------------------------------
void launch_ce_fwd(const bf16_t* logits, const int64_t* targets,
                   int64_t rows, int64_t vocab, int64_t ignore_index,
                   float* lse, float* loss_sum, int* count, hipStream_t s);
// v0: vocab-tile offset for tiled dlogits; nt=false keeps the tile in
// cache for the immediately following head GEMMs
void launch_ce_bwd(const bf16_t* logits, const int64_t* targets,
                   const float* lse, float scale, const float* scale_p,
                   int64_t ignore_index, int64_t v0, bool nt,
                   bf16_t* dlogits, int64_t rows, int64_t vocab,
                   hipStream_t s);
// Training: ce_fwd, then ce_bwd with scale *inv_count, row by row in one
// kernel, IN PLACE (logits becomes dlogits). A block's second sweep reads
// its row back from cache, so at most max_blocks rows are in flight.
void launch_ce_fwd_bwd(bf16_t* logits, const int64_t* targets, int64_t rows,
                       int64_t vocab, int64_t ignore_index,
                       const float* inv_count, float* lse, float* loss_sum,
                       int* count, int max_blocks, hipStream_t s);
// The same with the row held in LDS between the sweeps, one block per CU.
// False, and nothing launched, when a row (2 * vocab bytes) does not fit
// lds_limit, the LDS a block may have: the caller takes the variant above.
bool launch_ce_fwd_bwd_lds(bf16_t* logits, const int64_t* targets,
                           int64_t rows, int64_t vocab, int64_t ignore_index,
                           const float* inv_count, float* lse,
                           float* loss_sum, int* count, int n_cu,
                           int64_t lds_limit, hipStream_t s);
// Rows ce_fwd_bwd keeps in flight: half the 256 MiB Infinity Cache's worth,
// at least one per CU (wider rows then spill to HBM, still correct) and at
// most the 4096 blocks the other CE kernels launch.
inline int dta_ce_fwd_bwd_blocks(int64_t vocab, int n_cu) {
  const int64_t fit = (int64_t(128) << 20) / (2 * (vocab > 0 ? vocab : 1));
  const int64_t lo = n_cu > 0 ? n_cu : 1;
  return int(fit < lo ? lo : (fit > 4096 ? 4096 : fit));
}
// pipelined head-GEMM+CE: per-tile online-softmax update + finalize
void launch_ce_chunk(const bf16_t* chunk, int64_t ld, int64_t rows,
                     int64_t cols, const int64_t* targets, int64_t v0,
                     float* tlogit, float* m_run, float* s_run,
                     hipStream_t s);
void launch_ce_finalize(const int64_t* targets, const float* m_run,
                        const float* s_run, const float* tlogit,
                        int64_t rows, int64_t ignore_index, float* lse,
                        float* loss_sum, int* count, hipStream_t s);

// ---- fused LM-head loss (forward only, no logits in memory) ----------------
// MFMA head GEMM x[T,K] @ w[V,K]^T whose accumulator tiles are folded into
// an online log-sum-exp in-register (head_loss.hip). K % 64 == 0, rows
// 16 B aligned, T >= 1. grid = (ceil(T/tile), nsplit), 1 <= nsplit <= vocab
// tiles; ws_m/ws_s: [nsplit, T] fp32 partials, folded in fixed order into
// m_run/s_run (exp2 units, the launch_ce_finalize inputs); tlogit [T] must
// be zeroed (only rows with an in-range target are written).
constexpr int DTA_HEAD_LOSS_TILE = 128;
// automatic vocab split: a few blocks per CU (2 are resident at 64 KB LDS),
// every split owning at least one vocab tile
inline int dta_head_loss_nsplit(int64_t T, int64_t V, int cus) {
  const int64_t rb = (T + DTA_HEAD_LOSS_TILE - 1) / DTA_HEAD_LOSS_TILE;
  const int64_t nt = (V + DTA_HEAD_LOSS_TILE - 1) / DTA_HEAD_LOSS_TILE;
  int64_t ns = (4 * int64_t(cus) + rb - 1) / (rb > 0 ? rb : 1);
  if (ns > nt) ns = nt;
  if (ns > 65535) ns = 65535;  // gridDim.y
  return int(ns < 1 ? 1 : ns);
}
void launch_head_loss(const bf16_t* x, const bf16_t* w,
                      const int64_t* targets, int64_t T, int64_t V, int K,
                      int nsplit, float* ws_m, float* ws_s, float* tlogit,
                      float* m_run, float* s_run, hipStream_t s);

// ---- weight-gradient GEMM with the bias sum folded in (wgrad.hip) ----------
// dw[out,in] = bf16(float(dw) + dy[T,out]^T x[T,in]), split over T. dy and x
// are row-major with row strides ld_dy/ld_x (elements, % 8 == 0, >= the
// width) and 16 B aligned bases; out % DTA_WGRAD_BM == 0, in % DTA_WGRAD_BN
// == 0, T >= 1 arbitrary (a ragged last K-step is zero-padded). slab:
// [nsplit, out, in] fp32, every element written (no zero-fill). bpart
// non-null ([nsplit, out] fp32) also sums dy over t: db = bf16(float(db) +
// sum) where db is non-null, else bout [out] fp32 is stored. dw/db are bf16
// views of any (2 B) alignment. Results repeat bit for bit.
constexpr int DTA_WGRAD_BM = 256;  // out per tile
constexpr int DTA_WGRAD_BN = 128;  // in per tile
constexpr int DTA_WGRAD_BK = 32;   // rows of t per K-step
// split count: two resident blocks per CU (512 threads, 54 KB LDS each),
// every slice owning at least one K-step
inline int dta_wgrad_nsplit(int64_t T, int64_t out, int64_t in, int cus) {
  const int64_t tiles = (out / DTA_WGRAD_BM) * (in / DTA_WGRAD_BN);
  const int64_t ksteps = (T + DTA_WGRAD_BK - 1) / DTA_WGRAD_BK;
  int64_t ns = 2 * int64_t(cus) / (tiles > 0 ? tiles : 1);
  if (ns > ksteps) ns = ksteps;
  return int(ns < 1 ? 1 : ns);
}
struct WgradArgs {
  const bf16_t *dy, *x;
  int64_t ld_dy, ld_x, T;
  int out, in, nsplit;
  float *slab, *bpart;
  bf16_t *dw, *db;
  float* bout;
};
void launch_wgrad(const WgradArgs& a, hipStream_t s);

// ---- embedding ------------------------------------------------------------
// pos_p: device position offset for wpe (graph-replayable decode).
// doc_start: optional int32 [n_tok] (packed sequences, the attention q_lo):
// the wpe row of token t becomes (t % seq_len) - doc_start[t], with
// doc_start clamped to [0, t % seq_len].
void launch_embedding_fwd(const int64_t* ids, const bf16_t* wte,
                          const bf16_t* wpe, bf16_t* out, int64_t n_tok,
                          int seq_len, int dim, bool has_wpe,
                          const int* pos_p, const int* doc_start,
                          hipStream_t s);
// dwpe under restarting positions: out[p, :] = sum of dy[b, s, :] over the
// tokens with s - doc_start[b, s] == p, for p < seq (out: fp32 [seq * dim],
// stored). A document starts where clamp(doc_start[b, s], 0, s) == s and
// runs to the next start: doc_start must be a document layout (every value
// is the index of such a column), which is more than the q_lo contract; for
// any other tensor this is not the gradient of launch_embedding_fwd. part: [dta_doc_dwpe_stripes(B, seq, dim),
// seq * dim] fp32; dim % 8 == 0. Reads dy once, no atomics, repeats bit
// for bit.
inline int dta_doc_dwpe_stripes(int64_t B, int seq, int dim) {
  return dta_colred_stripes(B, seq * dim);
}
void launch_embedding_dwpe_doc(const bf16_t* dy, const int* doc_start,
                               float* part, float* out, int64_t B, int seq,
                               int dim, int stripes, hipStream_t s);
// KV-cache append at device position *pos_p + device int increment
void launch_kv_append(const bf16_t* kn, const bf16_t* vn, int64_t knb,
                      bf16_t* kc, bf16_t* vc, const int* pos_p, int B,
                      int Hk, int D, int64_t cb, int64_t ch, hipStream_t s);
void launch_i32_inc(int* p, hipStream_t s);
void launch_embedding_bwd(const bf16_t* dy, const int64_t* ids,
                          float* dwte_f32, float* dwpe_f32, int64_t n_tok,
                          int seq_len, int dim, bool has_wpe, hipStream_t s);
void launch_f32_to_bf16(const float* x, bf16_t* y, int64_t n, hipStream_t s);

// ---- serving gemv ---------------------------------------------------------
// y[M,N] = x[M,K] @ W[N,K]^T (+ bias), M <= 16 weight-streaming decode
void launch_gemv(const bf16_t* x, const bf16_t* w, const bf16_t* bias,
                 bf16_t* y, int M, int64_t N, int K, hipStream_t s);

// ---- rope -----------------------------------------------------------------
// pos_p: device position offset for graph-replayable decode
void launch_rope(const bf16_t* x, const float* cos_t, const float* sin_t,
                 bf16_t* y, int64_t bh, int seq, int hd, bool backward,
                 const int* pos_p, hipStream_t s);

// ---- attention ------------------------------------------------------------
// Strided geometry: every tensor is addressed as (batch, head, seq) strides
// over contiguous head_dim rows, whatever its memory order; kv tensors have
// H/grp heads (GQA). lse/delta are [B*H, S] fp32 contiguous.
struct AttnStride { int64_t batch, head, seq; };
struct AttnGeom {
  int B, H, grp, seq, hd;
  float scale;
  AttnStride q, k, v, o;   // forward operands and output
  AttnStride dout, dq;     // backward: incoming and query gradient
  AttnStride dkv;          // dk and dv of the direct-store path (grp == 1)
  // padding mask (reference attention_mask, right-padded batches:
  // training_manager.py:380-385): key j of batch row b is valid iff
  // j < kvlen[b]. null = no mask (all keys valid).
  const int* kvlen = nullptr;
  // attention-probability dropout (transformers GPT-2 attn_pdrop)
  DropParams drop;
  // document mask (packed sequences), int32 [B, seq] each, null = none:
  // key k is visible to query q iff q_lo[b,q] <= k on top of the rules
  // above. Contract: 0 <= q_lo[b,q] <= q, non-decreasing in q. k_hi[b,k] =
  // #{q : q_lo[b,q] <= k}, one past the last query that sees key k (the
  // backward's loop bound; required there whenever q_lo is set). The
  // kernels clamp what they read to [0, q] and [0, seq]: a tensor that
  // breaks the contract gives wrong numbers, never an out-of-bounds access.
  const int* q_lo = nullptr;
  const int* k_hi = nullptr;
};
void launch_attn_fwd(const bf16_t* q, const bf16_t* k, const bf16_t* v,
                     bf16_t* o, float* lse, const AttnGeom& geo,
                     hipStream_t s);
// also computes delta[q] = rowsum(dO * O) for the dkv kernel
void launch_attn_bwd_dq(const bf16_t* dout, const bf16_t* q, const bf16_t* k,
                        const bf16_t* v, const bf16_t* o, const float* lse,
                        float* delta, bf16_t* dq, const AttnGeom& geo,
                        hipStream_t s);
// grp > 1: fp32 atomics into zeroed contiguous [B,Hk,S,D] dk32/dv32;
// grp == 1: bf16 stores into dk/dv with the dkv strides
void launch_attn_bwd_dkv(const bf16_t* dout, const bf16_t* q,
                         const bf16_t* k, const bf16_t* v, const float* lse,
                         const float* delta, float* dk32, float* dv32,
                         bf16_t* dk, bf16_t* dv, const AttnGeom& geo,
                         hipStream_t s);
// Shapes the single-tile fused backward takes: the whole head is one
// 64-row tile, no GQA fold, and a head dim whose panels fit LDS (128 does
// not: 90 KB). Everything else runs dq then dkv.
inline bool dta_attn_bwd_fused_shape(const AttnGeom& geo) {
  return geo.seq <= 64 && geo.grp == 1 && (geo.hd == 32 || geo.hd == 64);
}
// DTA_ATTN_BWD_FUSED=0 keeps eligible shapes on the two-kernel path too.
inline bool dta_attn_bwd_fused_default() {
  static const bool en = [] {
    const char* e = ::getenv("DTA_ATTN_BWD_FUSED");
    return !(e && e[0] == '0');
  }();
  return en;
}
// dq + dk/dv of one (b, h) in one block; needs dta_attn_bwd_fused_shape.
// delta stays in LDS. dk/dv are stored with the dkv strides.
void launch_attn_bwd_fused(const bf16_t* dout, const bf16_t* q,
                           const bf16_t* k, const bf16_t* v, const bf16_t* o,
                           const float* lse, bf16_t* dq, bf16_t* dk,
                           bf16_t* dv, const AttnGeom& geo, hipStream_t s);

// len_p: device cache-length counter (effective kvlen = *len_p + 1) for
// hipGraph-replayable decode; null = host kvlen scalar
void launch_attn_decode(const bf16_t* q, const bf16_t* kc, const bf16_t* vc,
                        bf16_t* o, int B, int H, int grp, int kvlen,
                        const int* len_p, int hd, int64_t cb, int64_t ch,
                        float scale, hipStream_t s);

// ---- mfma layout self-test ------------------------------------------------
// D[32,32] = A[32,16] x B[16,32] and D[16,16] = A[16,32] x B[32,16]
void launch_mfma_probe_32(const bf16_t* A, const bf16_t* B, float* D,
                          hipStream_t s);
void launch_mfma_probe_16(const bf16_t* A, const bf16_t* B, float* D,
                          hipStream_t s);
