// Fused causal flash attention, forward + backward, MFMA
// (mfma_f32_16x16x32_bf16) with online softmax — the CDNA4 replacement for
// the reference's transformers attention (SURVEY.md §2.2 op table; miner
// seq 64, validator seq 512).
//
// Structure:
//   * grid = (ceil(S/64), B*H), block = 4 waves = 64 rows of one (b,h):
//     query rows in fwd/dq, key rows in dkv; each wave owns 16 of them and
//     keeps their fragments and accumulators in registers.
//   * The other operand is walked in 32-row tiles that all 256 threads
//     stage into LDS together, once per iteration, between two
//     __syncthreads (previous reads done / tile visible):
//       fwd: K row-major, V transposed
//       dq:  K row-major + transposed, V row-major
//       dkv: Q and dO, each row-major + transposed
//     Row-major panels (pitch D+8) feed A-fragments of the score MFMAs,
//     transposed [D][LDS_RP] panels feed B-fragments of the accumulating
//     MFMAs as single 16 B LDS reads.
//   * seq <= 64 without GQA (the training shape): attn_bwd_fused_k does dq
//     and dkv in one block from resident 64-row panels, so the operands
//     leave HBM once; same arithmetic, bit-identical results. Measured
//     0.249 ms against 0.126 + 0.183 ms (profiles/r04_fused_backward.md).
//   * Barrier-uniform loops: the trip count depends on blockIdx only, and
//     a wave with nothing to do in an iteration `continue`s AFTER the
//     second barrier. Nothing returns or breaks before a __syncthreads.
//   * STRIDE-AWARE addressing: q/k/v/o are consumed as [B,H,S,D] *views*
//     of the projection output [B,S,H*D] (and dq/dk/dv written the same
//     way) so the model layer does zero transpose/contiguous copies.
//   * GQA native: kv head = h / group; no repeat_interleave materialization.
//     Backward dK/dV: attn_bwd_dkv_gqa_k walks the head group inside one
//     block per KV head (no atomics, bf16 stores, bit-repeatable) for the
//     shapes of dta_attn_bwd_gqa_wins; attn_bwd_dkv_k<., ATOMIC> folds the
//     heads with fp32 atomics everywhere else.
//   * Serving decode has two routes: attn_decode_k (one block per query
//     head, fp32 FMAs) and attn_decode_split_k + attn_decode_combine_k (one
//     block per KV head and cache split, the head group on MFMA); see the
//     comments at the kernels and ops.decode_split_plan. The split route
//     has an int8-cache sibling, attn_decode_split_q8_k (codes + per-row
//     scales, written by kv_append_q8_k in embedding.hip).
//   * Sq > 1 new queries on a filled cache (chunked prefill, a second turn,
//     verifying drafted tokens): attn_extend_k, one block per 64 (position,
//     head-in-group) rows of a KV head, optional KV splits merged by
//     attn_decode_combine_k; see the comment at the kernel.
//   * swapped QK^T: mfma(A=K_tile, B=Q^T) puts a query's scores in lanes
//     sharing (lane&15) so the softmax row-reduce is two shfl_xor ops;
//     exp via the single-instruction exp2 path.
//   * Document mask (packed sequences, DOC instantiations): geo.q_lo adds
//     the lower bound q_lo[b,q] <= k to the rule. Tile skipping stays
//     block-uniform: fwd/dq start the key walk at the 32-tile holding q_lo
//     of the block's first row (the smallest, q_lo is non-decreasing), dkv
//     ends the query walk at k_hi of the block's last live key. A skipped
//     tile is one whose probabilities are all exactly 0, so skipping
//     changes no bit. The unmasked instantiations are the code they were.
//   * One copy each of the mask rule (attn_visible), the dropout draw of a
//     32-key tile (attn_drop_hashes/attn_drop_apply) and the accumulator
//     walk (for_acc_rows); the host gold mirrors them in ops/droprng.py.
//
// Fragment maps (verified on-device by mfma_selftest, tests/test_ops_gpu.py):
//   mfma_f32_16x16x32_bf16: A[i][k]: i=lane&15, k=8*(lane>>4)+j (j=0..7)
//                           B[k][n]: n=lane&15, k=8*(lane>>4)+j
//                           C/D[i][j]: col=lane&15, row=4*(lane>>4)+reg
#include "dta_common.h"
#include "dta_kernels.h"

#include <type_traits>

namespace {

// ---- per-block context ------------------------------------------------------
// What the three training kernels derive the same way from the geometry and
// the block/thread ids. Which 64-row tile the block owns is the kernel's.
struct AttnCtx {
  int tid, lane, wid, g;            // g = lane >> 4: MFMA lane group
  int b, h, hk;
  int64_t bhid;                     // b * H + h: row of lse/delta, RNG head
  const ushort *q, *k, *v, *dout;   // (b, h | hk) base pointers
  float sc2;                        // scale folded into the exp2 argument
  int kvl;                          // keys >= kvl are padding (block-uniform)
  const int *q_lo, *k_hi;           // document mask rows of b, or null
  uint32_t thr;                     // dropout threshold, 0 = off
  uint64_t drop_s2;                 // per-head dropout seed
};

// The fields that follow the query head: a block of the GQA dK/dV kernel
// walks every head of its group and re-derives them at each head step.
// dout may be null (forward); its strides are then 0.
DEV void attn_ctx_set_head(AttnCtx& c, const AttnGeom& geo, const ushort* q,
                           const ushort* dout, int h) {
  c.h = h;
  c.bhid = int64_t(c.b) * geo.H + h;
  c.q = q + c.b * geo.q.batch + h * geo.q.head;
  c.dout = dout + c.b * geo.dout.batch + h * geo.dout.head;
  c.drop_s2 = 0;
  if (c.thr)
    c.drop_s2 = rng_head_seed(rng_site_seed(geo.drop.rng, geo.drop.site),
                              uint64_t(c.bhid));
}

// Context of batch row b and query head h (kv head h / grp).
DEV AttnCtx attn_ctx_at(const AttnGeom& geo, const ushort* q, const ushort* k,
                        const ushort* v, const ushort* dout, int b, int h) {
  AttnCtx c;
  c.tid = threadIdx.x;
  c.lane = c.tid & 63;
  c.wid = c.tid >> 6;
  c.g = c.lane >> 4;
  c.b = b;
  c.hk = h / geo.grp;
  c.k = k + c.b * geo.k.batch + c.hk * geo.k.head;
  c.v = v + c.b * geo.v.batch + c.hk * geo.v.head;
  c.sc2 = geo.scale * LOG2E;
  c.kvl = geo.kvlen ? min(geo.seq, geo.kvlen[c.b]) : geo.seq;
  c.q_lo = geo.q_lo ? geo.q_lo + int64_t(c.b) * geo.seq : nullptr;
  c.k_hi = geo.k_hi ? geo.k_hi + int64_t(c.b) * geo.seq : nullptr;
  c.thr = geo.drop.thr16;
  attn_ctx_set_head(c, geo, q, dout, h);
  return c;
}

// blockIdx.y = b * H + h: one block per query head
DEV AttnCtx attn_ctx(const AttnGeom& geo, const ushort* q, const ushort* k,
                     const ushort* v, const ushort* dout) {
  return attn_ctx_at(geo, q, k, v, dout, int(blockIdx.y) / geo.H,
                     int(blockIdx.y) % geo.H);
}

// Rows past seq are loaded from the last row instead: garbage, but in
// bounds, and safe everywhere because the matching score/probability lanes
// are masked to 0.
DEV int clamp_row(int row, int seq) { return row < seq ? row : seq - 1; }

// key k is visible to query q: causal, not padding of this batch row, and
// (DOC) not before lo = q_lo[b,q], the start of q's document
template <bool DOC>
DEV bool attn_visible(int q, int k, int kvl, int lo) {
  return (!DOC || lo <= k) && k <= q && k < kvl;
}
// The document-mask operands as the kernels read them: row index clamped
// into the table, value clamped to the contract's range, so no input can
// move a loop bound or a mask outside [0, seq].
DEV int doc_lo(const AttnCtx& c, int q, int seq) {
  q = clamp_row(q, seq);
  return min(max(c.q_lo[q], 0), q);
}
DEV int doc_hi(const AttnCtx& c, int k, int seq) {
  return min(max(c.k_hi[clamp_row(max(k, 0), seq)], 0), seq);
}


// ---- dropout of a 32-key score tile (fwd, dq) -------------------------------
// A lane holds keys kv0 + 4g + r and kv0 + 16 + 4g + r (r = 0..3) of query
// qrow: one hash covers the 4 consecutive keys of each half (k & 3 == r).
struct DropHashes { uint64_t h0, h1; };
DEV DropHashes attn_drop_hashes(const AttnCtx& c, int qrow, int kv0) {
  const uint64_t hq = rng_attn_row(c.drop_s2, uint32_t(qrow));
  return {rng_attn_row_hash(hq, uint32_t((kv0 + 4 * c.g) >> 2)),
          rng_attn_row_hash(hq, uint32_t((kv0 + 16 + 4 * c.g) >> 2))};
}
// keep-or-zero of the element in hash slot r (k & 3), unbiased rescale
DEV float attn_drop_keep(float x, uint64_t h, int r, const DropParams& d) {
  return rng_keep(h, r, d.thr16) ? x * d.inv_keep : 0.f;
}

// ---- fragments and LDS tile staging ----------------------------------------
// B-fragments (k-major columns) gathered straight from global memory cost 8
// scalar 2 B loads each, every one touching its own 64 B line (~32x wasted
// HBM traffic — measured 204 us on the dkv kernel), and loading tiles per
// wave re-read ~590 MB/step from L2/HBM at the flagship shape. So the 4
// waves stage each 32-row tile once, cooperatively.
constexpr int LDS_RP = 40;  // 32 rows + 8 pad (multiple of 8: aligned reads)
// Row-major pitch: D+8 (2-way max bank conflict on 16-row A reads).
template <int DTILES> constexpr int LDS_RM_PITCH = 16 * DTILES + 8;
template <int DTILES> constexpr int LDS_RM_SIZE = 32 * LDS_RM_PITCH<DTILES>;
template <int DTILES> constexpr int LDS_T_SIZE = 16 * DTILES * LDS_RP;

DEV bf16x8 load_frag_row(const ushort* base, int64_t row_stride, int row,
                         int col0) {
  return as_bf16x8(*reinterpret_cast<const s16x8*>(
      base + int64_t(row) * row_stride + col0));
}
DEV bf16x8 load_frag_col_lds(const ushort* lds_t, int row0, int col) {
  return as_bf16x8(
      *reinterpret_cast<const s16x8*>(lds_t + col * LDS_RP + row0));
}
template <int DTILES>
DEV bf16x8 load_frag_rm(const ushort* lds_rm, int row_rel, int c0) {
  return as_bf16x8(*reinterpret_cast<const s16x8*>(
      lds_rm + row_rel * LDS_RM_PITCH<DTILES> + c0));
}

// Stage rows row0..row0+31 of a [seq, D] operand into LDS, row-major or
// TRANSPOSEd, one clamped 16 B global load per chunk.
template <int DTILES, bool TRANSPOSE>
DEV void stage_tile(ushort* lds, const ushort* src, int64_t rstride,
                    int row0, int seq, int tid) {
  constexpr int CPR = 2 * DTILES;       // 16B chunks per row (D/8)
  for (int i = tid; i < 32 * CPR; i += 256) {
    const int r = i / CPR, c8 = (i % CPR) * 8;
    const s16x8 v = *reinterpret_cast<const s16x8*>(
        src + int64_t(clamp_row(row0 + r, seq)) * rstride + c8);
    if constexpr (TRANSPOSE) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        lds[(c8 + j) * LDS_RP + r] = ushort(v[j]);
    } else {
      *reinterpret_cast<s16x8*>(lds + r * LDS_RM_PITCH<DTILES> + c8) = v;
    }
  }
}

DEV bf16x8 pack_bf16x8(const float* f) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    union { ushort s; __bf16 b; } c;
    c.s = f2bf(f[j]);
    o[j] = c.b;
  }
  return o;
}

// Redistribute a 32-key score tile from C layout (q=lane&15,
// key=16*ks+4*(lane>>4)+r in p0/p1) into the A-fragment layout
// (q=lane&15, k=8*(lane>>4)+j) — two shfl rounds per j.
DEV bf16x8 scores_to_afrag(const f32x4& p0, const f32x4& p1, int lane) {
  const int g = lane >> 4;
  float pa[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int kt = 8 * g + j;
    const int src = (lane & 15) + 16 * ((kt >> 2) & 3);
    const float va = __shfl(p0[j & 3], src);
    const float vb = __shfl(p1[j & 3], src);
    pa[j] = (kt < 16) ? va : vb;
  }
  return pack_bf16x8(pa);
}

// ---- accumulator epilogue ---------------------------------------------------
// Walk a wave's [16, D] accumulator in C layout: f(t, r, row, col) for
// every element whose row (row0 + 4g + r) is below seq.
template <int DTILES, class F>
DEV void for_acc_rows(int row0, int seq, int lane, F f) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * (lane >> 4) + r;
    if (row >= seq) continue;
#pragma unroll
    for (int t = 0; t < DTILES; ++t) f(t, r, row, 16 * t + (lane & 15));
  }
}
// dst[row, col] = bf16(acc * fac[r]) for o and dq; dst is their (b, h) base
template <int DTILES>
DEV void store_acc_tile(ushort* dst, int64_t rstride, int row0, int seq,
                        int lane, const f32x4* acc, f32x4 fac) {
  for_acc_rows<DTILES>(row0, seq, lane, [&](int t, int r, int row, int col) {
    dst[int64_t(row) * rstride + col] = f2bf(acc[t][r] * fac[r]);
  });
}

// ---------------- forward ----------------
// K (row-major) and V (transposed) tiles are staged once per block per
// 32-key iteration.
template <int DTILES, bool DOC>  // D = 16*DTILES
__global__ void attn_fwd_k(const ushort* __restrict__ q,
                           const ushort* __restrict__ k,
                           const ushort* __restrict__ v,
                           ushort* __restrict__ o, float* __restrict__ lse,
                           AttnGeom geo) {
  const AttnCtx c = attn_ctx(geo, q, k, v, nullptr);
  const int lane = c.lane, g = c.g, seq = geo.seq, kvl = c.kvl;
  const int q0 = blockIdx.x * 64 + c.wid * 16;
  const bool live = q0 < seq;
  const int qrow = q0 + (lane & 15);

  bf16x8 qb_[DTILES / 2];
#pragma unroll
  for (int sl = 0; sl < DTILES / 2; ++sl)
    qb_[sl] = load_frag_row(c.q, geo.q.seq, clamp_row(qrow, seq),
                            32 * sl + 8 * g);

  f32x4 acc[DTILES];
#pragma unroll
  for (int t = 0; t < DTILES; ++t) acc[t] = f32x4{0, 0, 0, 0};
  float m_run = -INFINITY, l_run = 0.f;  // in exp2 units

  __shared__ ushort k_rm[LDS_RM_SIZE<DTILES>];
  __shared__ ushort v_t[LDS_T_SIZE<DTILES>];
  // loop + mask bounds honor the pad length (kvl == seq when unmasked)
  const int blk_kv_end =
      min(min(seq, int(blockIdx.x) * 64 + 64), (kvl + 31) & ~31);  // uniform
  const int my_kv_end = live ? min(seq, q0 + 16) : 0;
  // DOC: no row of the block sees a key before q_lo of its first row
  const int lo_q = DOC ? doc_lo(c, qrow, seq) : 0;
  const int blk_kv_begin =
      DOC ? (doc_lo(c, int(blockIdx.x) * 64, seq) & ~31) : 0;  // uniform
  for (int kv0 = blk_kv_begin; kv0 < blk_kv_end; kv0 += 32) {
    __syncthreads();   // previous iteration's LDS reads complete
    stage_tile<DTILES, false>(k_rm, c.k, geo.k.seq, kv0, seq, c.tid);
    stage_tile<DTILES, true>(v_t, c.v, geo.v.seq, kv0, seq, c.tid);
    __syncthreads();
    if (kv0 >= my_kv_end) continue;   // after barriers: uniform safety
    f32x4 p0 = {0, 0, 0, 0}, p1 = {0, 0, 0, 0};
#pragma unroll
    for (int sl = 0; sl < DTILES / 2; ++sl) {
      const int c0 = 32 * sl + 8 * g;
      bf16x8 ka = load_frag_rm<DTILES>(k_rm, lane & 15, c0);
      p0 = mfma_bf16(ka, qb_[sl], p0);
      bf16x8 kb2 = load_frag_rm<DTILES>(k_rm, 16 + (lane & 15), c0);
      p1 = mfma_bf16(kb2, qb_[sl], p1);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k0a = kv0 + 4 * g + r, k1a = k0a + 16;
      p0[r] = attn_visible<DOC>(qrow, k0a, kvl, lo_q) ? p0[r] * c.sc2
                                                      : -INFINITY;
      p1[r] = attn_visible<DOC>(qrow, k1a, kvl, lo_q) ? p1[r] * c.sc2
                                                      : -INFINITY;
      mx = fmaxf(mx, fmaxf(p0[r], p1[r]));
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);
    const float alpha =
        (m_run == -INFINITY) ? 0.f : __builtin_exp2f(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p0[r] = (p0[r] == -INFINITY) ? 0.f : __builtin_exp2f(p0[r] - m_new);
      p1[r] = (p1[r] == -INFINITY) ? 0.f : __builtin_exp2f(p1[r] - m_new);
      psum += p0[r] + p1[r];
    }
    psum += __shfl_xor(psum, 16);
    psum += __shfl_xor(psum, 32);
    l_run = l_run * alpha + psum;
    m_run = m_new;

    if (c.thr) {
      // dropout on the PV accumulation only: l keeps the undropped sum,
      // so O = dropout(P) V with P the true softmax
      const DropHashes dh = attn_drop_hashes(c, qrow, kv0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p0[r] = attn_drop_keep(p0[r], dh.h0, r, geo.drop);
        p1[r] = attn_drop_keep(p1[r], dh.h1, r, geo.drop);
      }
    }
    bf16x8 pa = scores_to_afrag(p0, p1, lane);
    float a_r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a_r[r] = __shfl(alpha, 4 * g + r);
#pragma unroll
    for (int t = 0; t < DTILES; ++t) {
      acc[t][0] *= a_r[0]; acc[t][1] *= a_r[1];
      acc[t][2] *= a_r[2]; acc[t][3] *= a_r[3];
      bf16x8 vb = load_frag_col_lds(v_t, 8 * g, 16 * t + (lane & 15));
      acc[t] = mfma_bf16(pa, vb, acc[t]);
    }
  }

  if (!live) return;
  // epilogue: O /= l; lse stored in NATURAL-log units = (m + log2 l)*ln2
  if (lane < 16 && qrow < seq)
    lse[c.bhid * seq + qrow] = (m_run + __builtin_log2f(l_run)) * LN2;
  f32x4 inv;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float lr = __shfl(l_run, 4 * g + r);
    inv[r] = lr > 0.f ? 1.0f / lr : 0.f;
  }
  store_acc_tile<DTILES>(o + c.b * geo.o.batch + c.h * geo.o.head, geo.o.seq,
                         q0, seq, lane, acc, inv);
}

// ---------------- backward dQ ----------------
// K (row-major + transposed) and V (row-major) staged once per block per
// 32-key iteration.
// Also COMPUTES delta[q] = rowsum(dO[q]*O[q]) from its own rows (it loads
// dO anyway; O rows are one extra coalesced read) and publishes it for the
// dkv kernel — the standalone delta kernel is gone.
template <int DTILES, bool DOC>
__global__ void attn_bwd_dq_k(const ushort* __restrict__ dout,
                              const ushort* __restrict__ q,
                              const ushort* __restrict__ k,
                              const ushort* __restrict__ v,
                              const ushort* __restrict__ o,
                              const float* __restrict__ lse,
                              float* __restrict__ delta,
                              ushort* __restrict__ dq, AttnGeom geo) {
  const AttnCtx c = attn_ctx(geo, q, k, v, dout);
  const int lane = c.lane, g = c.g, seq = geo.seq, kvl = c.kvl;
  const int q0 = blockIdx.x * 64 + c.wid * 16;
  const bool live = q0 < seq;
  const int qrow = q0 + (lane & 15);
  const int qr_ld = clamp_row(qrow, seq);
  const ushort* op = o + c.b * geo.o.batch + c.h * geo.o.head;

  bf16x8 qb_[DTILES / 2], dob[DTILES / 2];
  float dpart = 0.f;
#pragma unroll
  for (int sl = 0; sl < DTILES / 2; ++sl) {
    const int c0 = 32 * sl + 8 * g;
    qb_[sl] = load_frag_row(c.q, geo.q.seq, qr_ld, c0);
    dob[sl] = load_frag_row(c.dout, geo.dout.seq, qr_ld, c0);
    bf16x8 orow = load_frag_row(op, geo.o.seq, qr_ld, c0);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      dpart = fmaf(float(dob[sl][j]), float(orow[j]), dpart);
  }
  // delta[qrow]: each of the 4 lane-groups holds 16 of the 64 columns of
  // row (lane&15); fold across groups
  dpart += __shfl_xor(dpart, 16);
  dpart += __shfl_xor(dpart, 32);
  const float dlt_q = dpart;
  if (lane < 16 && qrow < seq) delta[c.bhid * seq + qrow] = dlt_q;
  const float lse_q = lse[c.bhid * seq + qr_ld] * LOG2E;  // exp2 units

  f32x4 acc[DTILES];
#pragma unroll
  for (int t = 0; t < DTILES; ++t) acc[t] = f32x4{0, 0, 0, 0};

  __shared__ ushort k_rm[LDS_RM_SIZE<DTILES>];
  __shared__ ushort v_rm[LDS_RM_SIZE<DTILES>];
  __shared__ ushort k_t[LDS_T_SIZE<DTILES>];
  const int blk_kv_end =
      min(min(seq, int(blockIdx.x) * 64 + 64), (kvl + 31) & ~31);  // uniform
  const int my_kv_end = live ? min(seq, q0 + 16) : 0;
  const int lo_q = DOC ? doc_lo(c, qrow, seq) : 0;
  const int blk_kv_begin =
      DOC ? (doc_lo(c, int(blockIdx.x) * 64, seq) & ~31) : 0;  // uniform
  for (int kv0 = blk_kv_begin; kv0 < blk_kv_end; kv0 += 32) {
    __syncthreads();
    stage_tile<DTILES, false>(k_rm, c.k, geo.k.seq, kv0, seq, c.tid);
    stage_tile<DTILES, false>(v_rm, c.v, geo.v.seq, kv0, seq, c.tid);
    stage_tile<DTILES, true>(k_t, c.k, geo.k.seq, kv0, seq, c.tid);
    __syncthreads();
    if (kv0 >= my_kv_end) continue;
    f32x4 s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
    f32x4 dp0 = {0, 0, 0, 0}, dp1 = {0, 0, 0, 0};
#pragma unroll
    for (int sl = 0; sl < DTILES / 2; ++sl) {
      const int c0 = 32 * sl + 8 * g;
      bf16x8 ka = load_frag_rm<DTILES>(k_rm, lane & 15, c0);
      bf16x8 kb2 = load_frag_rm<DTILES>(k_rm, 16 + (lane & 15), c0);
      bf16x8 va = load_frag_rm<DTILES>(v_rm, lane & 15, c0);
      bf16x8 vb2 = load_frag_rm<DTILES>(v_rm, 16 + (lane & 15), c0);
      s0 = mfma_bf16(ka, qb_[sl], s0);
      s1 = mfma_bf16(kb2, qb_[sl], s1);
      dp0 = mfma_bf16(va, dob[sl], dp0);
      dp1 = mfma_bf16(vb2, dob[sl], dp1);
    }
    // dS = P ⊙ (M/(1-p) ⊙ (dO Vᵀ) − delta): the dropout mask gates the
    // dO·V term only; delta = rowsum(dO ⊙ O) already absorbs the mask
    if (c.thr) {
      const DropHashes dh = attn_drop_hashes(c, qrow, kv0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        dp0[r] = attn_drop_keep(dp0[r], dh.h0, r, geo.drop);
        dp1[r] = attn_drop_keep(dp1[r], dh.h1, r, geo.drop);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k0a = kv0 + 4 * g + r, k1a = k0a + 16;
      const float P0 = attn_visible<DOC>(qrow, k0a, kvl, lo_q)
                           ? __builtin_exp2f(s0[r] * c.sc2 - lse_q) : 0.f;
      const float P1 = attn_visible<DOC>(qrow, k1a, kvl, lo_q)
                           ? __builtin_exp2f(s1[r] * c.sc2 - lse_q) : 0.f;
      s0[r] = P0 * (dp0[r] - dlt_q);
      s1[r] = P1 * (dp1[r] - dlt_q);
    }
    bf16x8 dsa = scores_to_afrag(s0, s1, lane);
#pragma unroll
    for (int t = 0; t < DTILES; ++t) {
      bf16x8 kcb = load_frag_col_lds(k_t, 8 * g, 16 * t + (lane & 15));
      acc[t] = mfma_bf16(dsa, kcb, acc[t]);
    }
  }
  if (!live) return;
  store_acc_tile<DTILES>(dq + c.b * geo.dq.batch + c.h * geo.dq.head,
                         geo.dq.seq, q0, seq, lane, acc,
                         f32x4{geo.scale, geo.scale, geo.scale, geo.scale});
}

// ---------------- backward dK/dV ----------------
// One 32-query tile (rows q0..q0+31 of head c.h, staged in the four LDS
// panels) against the wave's 16 key rows: scores, probabilities from lse,
// dS from delta, dropout, and the two accumulations. krow: the lane's key.
template <int DTILES, bool DOC>
DEV void dkv_tile(const AttnCtx& c, const AttnGeom& geo, const ushort* q_rm,
                  const ushort* d_rm, const ushort* q_t, const ushort* d_t,
                  int q0, int krow, const bf16x8* kb_, const bf16x8* vbf,
                  const float* __restrict__ lse,
                  const float* __restrict__ delta, f32x4* acck, f32x4* accv) {
  const int lane = c.lane, g = c.g, seq = geo.seq, kvl = c.kvl;
  f32x4 s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
  f32x4 dp0 = {0, 0, 0, 0}, dp1 = {0, 0, 0, 0};
#pragma unroll
  for (int sl = 0; sl < DTILES / 2; ++sl) {
    const int c0 = 32 * sl + 8 * g;
    bf16x8 qa = load_frag_rm<DTILES>(q_rm, lane & 15, c0);
    bf16x8 qa1 = load_frag_rm<DTILES>(q_rm, 16 + (lane & 15), c0);
    s0 = mfma_bf16(qa, kb_[sl], s0);
    s1 = mfma_bf16(qa1, kb_[sl], s1);
    bf16x8 doa = load_frag_rm<DTILES>(d_rm, lane & 15, c0);
    bf16x8 doa1 = load_frag_rm<DTILES>(d_rm, 16 + (lane & 15), c0);
    dp0 = mfma_bf16(doa, vbf[sl], dp0);
    dp1 = mfma_bf16(doa1, vbf[sl], dp1);
  }
  f32x4 p0, p1, ds0, ds1;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    // roles swapped: this lane's key krow against the tile's queries
    const int qa0 = q0 + 4 * g + r, qa1 = qa0 + 16;
    const bool v0 = qa0 < seq &&
        attn_visible<DOC>(qa0, krow, kvl, DOC ? doc_lo(c, qa0, seq) : 0);
    const bool v1 = qa1 < seq &&
        attn_visible<DOC>(qa1, krow, kvl, DOC ? doc_lo(c, qa1, seq) : 0);
    const float l0 = lse[c.bhid * seq + (v0 ? qa0 : 0)] * LOG2E;
    const float l1 = lse[c.bhid * seq + (v1 ? qa1 : 0)] * LOG2E;
    p0[r] = v0 ? __builtin_exp2f(s0[r] * c.sc2 - l0) : 0.f;
    p1[r] = v1 ? __builtin_exp2f(s1[r] * c.sc2 - l1) : 0.f;
    const float d0 = delta[c.bhid * seq + ((qa0 < seq) ? qa0 : 0)];
    const float d1 = delta[c.bhid * seq + ((qa1 < seq) ? qa1 : 0)];
    if (c.thr) {
      // element (q, k=krow): slice krow&3 of hash(q, krow>>2) — the
      // transposed view of the SAME per-(b,h,q,k) draw the fwd/dq
      // kernels take; dV uses the dropped P, dK the dropout-gated dS
      const uint64_t hk0 =
          rng_attn_hash(c.drop_s2, uint32_t(qa0), uint32_t(krow) >> 2);
      const uint64_t hk1 =
          rng_attn_hash(c.drop_s2, uint32_t(qa1), uint32_t(krow) >> 2);
      const float m0 =
          rng_keep(hk0, krow & 3, c.thr) ? geo.drop.inv_keep : 0.f;
      const float m1 =
          rng_keep(hk1, krow & 3, c.thr) ? geo.drop.inv_keep : 0.f;
      // dS = A ⊙ (M/(1-p)·dp − delta); dV gets the dropped P = A·M/(1-p)
      ds0[r] = p0[r] * (m0 * dp0[r] - d0);
      ds1[r] = p1[r] * (m1 * dp1[r] - d1);
      p0[r] *= m0;
      p1[r] *= m1;
    } else {
      ds0[r] = p0[r] * (dp0[r] - d0);
      ds1[r] = p1[r] * (dp1[r] - d1);
    }
  }
  bf16x8 pa = scores_to_afrag(p0, p1, lane);
  bf16x8 dsa = scores_to_afrag(ds0, ds1, lane);
#pragma unroll
  for (int t = 0; t < DTILES; ++t) {
    bf16x8 dob2 = load_frag_col_lds(d_t, 8 * g, 16 * t + (lane & 15));
    accv[t] = mfma_bf16(pa, dob2, accv[t]);
    bf16x8 qcb = load_frag_col_lds(q_t, 8 * g, 16 * t + (lane & 15));
    acck[t] = mfma_bf16(dsa, qcb, acck[t]);
  }
}

// Q/dO tiles staged once per block per 32-query iteration (row-major for
// the score mfmas, transposed for the accumulation B-fragments). With GQA
// (grp>1) off the one-pass route each kv head is walked once per ATTACHED
// q head (blockIdx.y covers B*H) and results are accumulated with fp32
// atomics into dk/dv.
// Early waves see a few below-diagonal query tiles (probabilities masked
// to 0) — the price of a uniform, barrier-safe loop.
template <int DTILES, bool ATOMIC, bool DOC>
__global__ void attn_bwd_dkv_k(const ushort* __restrict__ dout,
                               const ushort* __restrict__ q,
                               const ushort* __restrict__ k,
                               const ushort* __restrict__ v,
                               const float* __restrict__ lse,
                               const float* __restrict__ delta,
                               float* __restrict__ dk32,
                               float* __restrict__ dv32,
                               ushort* __restrict__ dk,
                               ushort* __restrict__ dv, AttnGeom geo) {
  const AttnCtx c = attn_ctx(geo, q, k, v, dout);
  const int lane = c.lane, g = c.g, seq = geo.seq, kvl = c.kvl;
  const int kv0 = blockIdx.x * 64 + c.wid * 16;
  const bool live = kv0 < seq;
  const int krow = kv0 + (lane & 15);

  bf16x8 kb_[DTILES / 2], vbf[DTILES / 2];
#pragma unroll
  for (int sl = 0; sl < DTILES / 2; ++sl) {
    kb_[sl] = load_frag_row(c.k, geo.k.seq, clamp_row(krow, seq),
                            32 * sl + 8 * g);
    vbf[sl] = load_frag_row(c.v, geo.v.seq, clamp_row(krow, seq),
                            32 * sl + 8 * g);
  }

  f32x4 acck[DTILES], accv[DTILES];
#pragma unroll
  for (int t = 0; t < DTILES; ++t) {
    acck[t] = f32x4{0, 0, 0, 0};
    accv[t] = f32x4{0, 0, 0, 0};
  }

  __shared__ ushort q_rm[LDS_RM_SIZE<DTILES>];
  __shared__ ushort d_rm[LDS_RM_SIZE<DTILES>];
  __shared__ ushort q_t[LDS_T_SIZE<DTILES>];
  __shared__ ushort d_t[LDS_T_SIZE<DTILES>];
  // a block whose 64 key rows are all padding has zero dk/dv: skip the
  // whole walk (uniform) and fall through to the zero-initialized stores
  const int q_start =
      (int(blockIdx.x) * 64 >= kvl) ? seq : int(blockIdx.x) * 64;
  // DOC: no query from k_hi of the block's last live key on sees any key of
  // the block (k_hi is non-decreasing); uniform, rounded up to the tile
  const int q_end =
      DOC ? min(seq, (doc_hi(c, min(int(blockIdx.x) * 64 + 64, kvl) - 1, seq)
                      + 31) & ~31)
          : seq;
  for (int q0 = q_start; q0 < q_end; q0 += 32) {
    __syncthreads();
    stage_tile<DTILES, false>(q_rm, c.q, geo.q.seq, q0, seq, c.tid);
    stage_tile<DTILES, false>(d_rm, c.dout, geo.dout.seq, q0, seq, c.tid);
    stage_tile<DTILES, true>(q_t, c.q, geo.q.seq, q0, seq, c.tid);
    stage_tile<DTILES, true>(d_t, c.dout, geo.dout.seq, q0, seq, c.tid);
    __syncthreads();
    if (!live || q0 + 31 < kv0) continue;   // fully below the diagonal
    dkv_tile<DTILES, DOC>(c, geo, q_rm, d_rm, q_t, d_t, q0, krow, kb_, vbf,
                          lse, delta, acck, accv);
  }
  if (!live) return;
  // One walk for both outputs: storing dk and dv in two passes costs the
  // head-dim-128 instantiation 16 more bytes of spill.
  for_acc_rows<DTILES>(kv0, seq, lane, [&](int t, int r, int row, int col) {
    if (ATOMIC) {
      // fp32 accumulation across the grp q-heads sharing this kv head,
      // into contiguous [B,Hk,S,D]
      const int64_t off =
          ((int64_t(c.b) * (geo.H / geo.grp) + c.hk) * seq + row) *
              (16 * DTILES) + col;
      atomicAdd(dk32 + off, acck[t][r] * geo.scale);
      atomicAdd(dv32 + off, accv[t][r]);
    } else {
      ushort* dkp = dk + c.b * geo.dkv.batch + c.hk * geo.dkv.head;
      ushort* dvp = dv + c.b * geo.dkv.batch + c.hk * geo.dkv.head;
      dkp[int64_t(row) * geo.dkv.seq + col] = f2bf(acck[t][r] * geo.scale);
      dvp[int64_t(row) * geo.dkv.seq + col] = f2bf(accv[t][r]);
    }
  });
}

// ---------------- backward dK/dV, GQA: the head group in one block ---------
// grid = (ceil(S/64), B*Hk): one block owns 64 key rows of one KV head and
// walks the grp query heads attached to it, heads ascending and inside a
// head the 32-query tiles ascending, through dkv_tile into ONE acck/accv
// register set. dk/dv are therefore a pure function of the inputs with a
// fixed summation order: no fp32 buffer, no atomics, no workspace, equal
// bits on every run. K/V fragments are loaded once per block; the head
// fields of the context (Q/dO base, lse/delta row, dropout head seed) are
// re-derived at every head step, the per-batch-row ones (kvl, document
// mask) stay. Key rows that are padding or unseen keep zero accumulators.
//
// Staging (what differs from attn_bwd_dkv_k, which fetches every Q and dO
// tile twice and transposes with 2 B LDS stores between two barriers):
//   * a thread owns a ROW PAIR x 16 B chunk of Q or dO: two 16 B global
//     loads into registers, once per tile. From those registers it writes
//     the row-major panel (two 16 B LDS stores) and the transposed panel
//     (eight 4 B stores: rows 2p, 2p+1 of one column are one LDS word).
//     Lanes 0..15 of a wave hold the 16 row pairs of one chunk, so a
//     transposed store is 4-way bank conflicted where a chunk-major lane
//     order would be 16-way.
//   * the loads of tile n+1 (which may belong to the next head) are issued
//     before the MFMAs of tile n and land during them.
//   * two LDS buffers: tile n+2 overwrites the buffer of tile n only after
//     the barrier of tile n+1, which every wave reaches after its reads of
//     tile n. One barrier per tile. One buffer between two barriers (same
//     register prefetch) measured 0.4885 against 0.4824 ms at B8 H32 Hk8
//     S512 D128 and 0.3713 against 0.3528 ms at B8 H14 Hk2 S512 D64, and
//     was dropped (profiles/r13_gqa_dkv.md).
// Epilogue: after the walk the LDS is free; each wave rounds its [16, D]
// dk and dv tiles to bf16 into it once and stores them as 16 B rows.
//
// Budget per block (256 threads), D = 16*DTILES, one buffer =
// 2 * 32*(D+8)*2 B row-major + 2 * D*40*2 B transposed:
//   D   LDS (2 buffers)   acc  K/V frags  prefetch   = held across the loop
//   32      20.0 KB        16      4         4 VGPR
//   64      38.0 KB        32      8         4
//  128      74.0 KB        64     16        16
// so two blocks per CU fit at D = 128 (160 KB LDS, 512 VGPR per SIMD lane).
template <int DTILES>
struct GqaStage {
  static constexpr int CPR = 2 * DTILES;       // 16 B chunks per row
  static constexpr int PER_OP = 16 * CPR;      // (row pair, chunk) per operand
  static constexpr int ITEMS = (2 * PER_OP + 255) / 256;   // per thread
  static constexpr int BUF = 2 * LDS_RM_SIZE<DTILES> + 2 * LDS_T_SIZE<DTILES>;
  s16x8 lo[ITEMS], hi[ITEMS];                  // rows 2p and 2p+1

  // item i of the tile: operand (0 Q, 1 dO), row pair, first column
  static DEV bool item(int tid, int it, int& op, int& rp, int& c8) {
    const int i = tid + 256 * it;
    op = i / PER_OP;
    rp = i & 15;
    c8 = ((i % PER_OP) >> 4) * 8;
    return i < 2 * PER_OP;
  }
  // rows q0..q0+31 of head bases qh/doh, clamped like stage_tile
  DEV void load(const ushort* qh, int64_t qs, const ushort* doh, int64_t ds,
                int q0, int seq, int tid) {
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      int op, rp, c8;
      if (!item(tid, it, op, rp, c8)) continue;
      const ushort* src = op ? doh : qh;
      const int64_t rs = op ? ds : qs;
      lo[it] = *reinterpret_cast<const s16x8*>(
          src + int64_t(clamp_row(q0 + 2 * rp, seq)) * rs + c8);
      hi[it] = *reinterpret_cast<const s16x8*>(
          src + int64_t(clamp_row(q0 + 2 * rp + 1, seq)) * rs + c8);
    }
  }
  // buf: Q row-major | dO row-major | Q transposed | dO transposed
  DEV void store(ushort* buf, int tid) const {
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      int op, rp, c8;
      if (!item(tid, it, op, rp, c8)) continue;
      ushort* rm = buf + op * LDS_RM_SIZE<DTILES> +
                   2 * rp * LDS_RM_PITCH<DTILES> + c8;
      *reinterpret_cast<s16x8*>(rm) = lo[it];
      *reinterpret_cast<s16x8*>(rm + LDS_RM_PITCH<DTILES>) = hi[it];
      ushort* t = buf + 2 * LDS_RM_SIZE<DTILES> + op * LDS_T_SIZE<DTILES> +
                  c8 * LDS_RP + 2 * rp;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        *reinterpret_cast<uint32_t*>(t + j * LDS_RP) =
            uint32_t(ushort(lo[it][j])) | uint32_t(ushort(hi[it][j])) << 16;
    }
  }
};

// The fp32 scale of the epilogue stays a scalar multiply: the packed
// two-lane fp32 forms are switched off for this kernel.
template <int DTILES, bool DOC>
__global__ __launch_bounds__(256)
__attribute__((target("no-packed-fp32-ops")))
void attn_bwd_dkv_gqa_k(const ushort* __restrict__ dout,
                        const ushort* __restrict__ q,
                        const ushort* __restrict__ k,
                        const ushort* __restrict__ v,
                        const float* __restrict__ lse,
                        const float* __restrict__ delta,
                        ushort* __restrict__ dk, ushort* __restrict__ dv,
                        AttnGeom geo) {
  using Stage = GqaStage<DTILES>;
  constexpr int PITCH = LDS_RM_PITCH<DTILES>;
  static_assert(4 * 2 * 16 * PITCH <= 2 * Stage::BUF, "epilogue tiles fit");
  const int n_hk = geo.H / geo.grp;
  const int b = int(blockIdx.y) / n_hk, hk = int(blockIdx.y) % n_hk;
  AttnCtx c = attn_ctx_at(geo, q, k, v, dout, b, hk * geo.grp);
  const int lane = c.lane, g = c.g, seq = geo.seq, kvl = c.kvl;
  const int kv0 = blockIdx.x * 64 + c.wid * 16;
  const bool live = kv0 < seq;
  const int krow = kv0 + (lane & 15);

  bf16x8 kb_[DTILES / 2], vbf[DTILES / 2];
#pragma unroll
  for (int sl = 0; sl < DTILES / 2; ++sl) {
    kb_[sl] = load_frag_row(c.k, geo.k.seq, clamp_row(krow, seq),
                            32 * sl + 8 * g);
    vbf[sl] = load_frag_row(c.v, geo.v.seq, clamp_row(krow, seq),
                            32 * sl + 8 * g);
  }
  f32x4 acck[DTILES], accv[DTILES];
#pragma unroll
  for (int t = 0; t < DTILES; ++t) {
    acck[t] = f32x4{0, 0, 0, 0};
    accv[t] = f32x4{0, 0, 0, 0};
  }

  __shared__ __attribute__((aligned(16))) ushort lds[2 * Stage::BUF];
  // the query walk of one head, as in attn_bwd_dkv_k (all block-uniform):
  // nothing for a block of padding keys; DOC ends it at k_hi of the
  // block's last live key
  const int q_start =
      (int(blockIdx.x) * 64 >= kvl) ? seq : int(blockIdx.x) * 64;
  const int q_end =
      DOC ? min(seq, (doc_hi(c, min(int(blockIdx.x) * 64 + 64, kvl) - 1, seq)
                      + 31) & ~31)
          : seq;
  const int n_q = q_end > q_start ? (q_end - q_start + 31) / 32 : 0;
  const int total = geo.grp * n_q;          // tiles: heads x query tiles

  Stage st;
  if (total) st.load(c.q, geo.q.seq, c.dout, geo.dout.seq, q_start, seq, c.tid);
  int ld_h = c.h, ld_q0 = q_start;          // the tile held in st
  int q0 = q_start;                         // the tile computed
  for (int n = 0; n < total; ++n) {
    ushort* buf = lds + (n & 1) * Stage::BUF;
    st.store(buf, c.tid);
    ld_q0 += 32;
    if (ld_q0 >= q_end) { ld_q0 = q_start; ++ld_h; }
    if (n + 1 < total)
      st.load(q + b * geo.q.batch + ld_h * geo.q.head, geo.q.seq,
              dout + b * geo.dout.batch + ld_h * geo.dout.head, geo.dout.seq,
              ld_q0, seq, c.tid);
    __syncthreads();
    if (n && q0 == q_start) attn_ctx_set_head(c, geo, q, dout, c.h + 1);
    if (live && q0 + 31 >= kv0)             // not fully below the diagonal
      dkv_tile<DTILES, DOC>(c, geo, buf, buf + LDS_RM_SIZE<DTILES>,
                            buf + 2 * LDS_RM_SIZE<DTILES>,
                            buf + 2 * LDS_RM_SIZE<DTILES> + LDS_T_SIZE<DTILES>,
                            q0, krow, kb_, vbf, lse, delta, acck, accv);
    q0 += 32;
    if (q0 >= q_end) q0 = q_start;
  }

  // epilogue: dk | dv tile of the wave, bf16, through LDS
  __syncthreads();                          // every read of the walk is done
  ushort* tile = lds + c.wid * 2 * 16 * PITCH;
  if (live)
    for_acc_rows<DTILES>(0, 16, lane, [&](int t, int r, int row, int col) {
      tile[row * PITCH + col] = f2bf(acck[t][r] * geo.scale);
      tile[(16 + row) * PITCH + col] = f2bf(accv[t][r]);
    });
  __syncthreads();
  if (!live) return;
  ushort* dkp = dk + b * geo.dkv.batch + hk * geo.dkv.head;
  ushort* dvp = dv + b * geo.dkv.batch + hk * geo.dkv.head;
#pragma unroll
  for (int i = lane; i < 16 * Stage::CPR; i += 64) {
    const int row = i / Stage::CPR, c8 = (i % Stage::CPR) * 8;
    if (kv0 + row >= seq) continue;
    const int64_t off = int64_t(kv0 + row) * geo.dkv.seq + c8;
    *reinterpret_cast<s16x8*>(dkp + off) =
        *reinterpret_cast<const s16x8*>(tile + row * PITCH + c8);
    *reinterpret_cast<s16x8*>(dvp + off) =
        *reinterpret_cast<const s16x8*>(tile + (16 + row) * PITCH + c8);
  }
}

// ---------------- backward, whole head in one tile ----------------
// seq <= 64 and grp == 1 (the miner's training shape): the dq block and the
// dkv block of a (b, h) load the same four 64-row tiles, so one block does
// both and Q, K, V, dO and O leave HBM once. Both score walks are kept
// (S/P/dS recomputed q-major, then k-major), reading the resident panels
// where the two kernels above read staged tiles and global rows, so every
// element goes through the same arithmetic in the same order and dq/dk/dv
// are bit-identical to the two-kernel path. delta and lse live in LDS; the
// delta global buffer is not needed.
// LDS: the four operands row-major as two 32-row tiles each, as
// stage_tile lays them out. The transposed panels are made from those
// (LDS to LDS) and share one pool with the K/V row-major panels, which the
// dkv phase reads from registers only:
//   dq phase:  pool = K rm | V rm | K t      dkv phase: pool = Q t | dO t
// 47.6 KB at D = 64: three blocks per CU. D = 128 would need 90 KB (one
// block per CU) and is left on the two-kernel path.
// No wave returns before the last __syncthreads.
template <int DTILES>
DEV bf16x8 load_frag_head(const ushort* rm2, int row, int c0) {
  return load_frag_rm<DTILES>(rm2 + (row >> 5) * LDS_RM_SIZE<DTILES>,
                              row & 31, c0);
}

template <int DTILES, bool DOC>
__global__ void attn_bwd_fused_k(const ushort* __restrict__ dout,
                                 const ushort* __restrict__ q,
                                 const ushort* __restrict__ k,
                                 const ushort* __restrict__ v,
                                 const ushort* __restrict__ o,
                                 const float* __restrict__ lse,
                                 ushort* __restrict__ dq,
                                 ushort* __restrict__ dk,
                                 ushort* __restrict__ dv, AttnGeom geo) {
  constexpr int RM = LDS_RM_SIZE<DTILES>, TP = LDS_T_SIZE<DTILES>;
  constexpr int PITCH = LDS_RM_PITCH<DTILES>;
  static_assert(4 * TP <= 4 * RM + 2 * TP, "Q t | dO t must fit the pool");
  const AttnCtx c = attn_ctx(geo, q, k, v, dout);
  const int lane = c.lane, g = c.g, seq = geo.seq, kvl = c.kvl;
  const int r0 = c.wid * 16;           // this wave's query rows, then key rows
  const bool live = r0 < seq;
  const int row = r0 + (lane & 15);    // qrow in the dq phase, krow in dkv

  __shared__ __attribute__((aligned(16))) ushort q_rm[2 * RM];
  __shared__ __attribute__((aligned(16))) ushort d_rm[2 * RM];
  __shared__ __attribute__((aligned(16))) ushort pool[4 * RM + 2 * TP];
  __shared__ float lse_s[64], dlt_s[64];
  // DOC: the head's 64 clamped q_lo values, read per (query, key) pair in
  // both phases; never referenced (and so not allocated) without DOC
  __shared__ int lo_s[64];
  ushort* k_rm = pool;
  ushort* v_rm = pool + 2 * RM;
  ushort* k_t = pool + 4 * RM;
  ushort* q_t = pool;
  ushort* d_t = pool + 2 * TP;

  // O rows feed delta only: straight to registers, issued before staging
  const ushort* op = o + c.b * geo.o.batch + c.h * geo.o.head;
  bf16x8 orow[DTILES / 2];
#pragma unroll
  for (int sl = 0; sl < DTILES / 2; ++sl)
    orow[sl] = load_frag_row(op, geo.o.seq, clamp_row(row, seq),
                             32 * sl + 8 * g);
  if (c.tid < 64) lse_s[c.tid] = lse[c.bhid * seq + clamp_row(c.tid, seq)];
  if constexpr (DOC)
    if (c.tid < 64) lo_s[c.tid] = doc_lo(c, c.tid, seq);
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) {
    stage_tile<DTILES, false>(q_rm + t2 * RM, c.q, geo.q.seq, 32 * t2, seq,
                              c.tid);
    stage_tile<DTILES, false>(d_rm + t2 * RM, c.dout, geo.dout.seq, 32 * t2,
                              seq, c.tid);
    stage_tile<DTILES, false>(k_rm + t2 * RM, c.k, geo.k.seq, 32 * t2, seq,
                              c.tid);
    stage_tile<DTILES, false>(v_rm + t2 * RM, c.v, geo.v.seq, 32 * t2, seq,
                              c.tid);
  }
  __syncthreads();
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2)
    stage_tile<DTILES, true>(k_t + t2 * TP, k_rm + t2 * RM, PITCH, 0, 32,
                             c.tid);

  // ---- dq phase: attn_bwd_dq_k for query rows r0..r0+15 ----
  {
    const int qrow = row;
    bf16x8 qb_[DTILES / 2], dob[DTILES / 2];
    float dpart = 0.f;
#pragma unroll
    for (int sl = 0; sl < DTILES / 2; ++sl) {
      const int c0 = 32 * sl + 8 * g;
      qb_[sl] = load_frag_head<DTILES>(q_rm, qrow, c0);
      dob[sl] = load_frag_head<DTILES>(d_rm, qrow, c0);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        dpart = fmaf(float(dob[sl][j]), float(orow[sl][j]), dpart);
    }
    dpart += __shfl_xor(dpart, 16);
    dpart += __shfl_xor(dpart, 32);
    const float dlt_q = dpart;
    if (lane < 16 && qrow < seq) dlt_s[qrow] = dlt_q;
    const float lse_q = lse_s[qrow] * LOG2E;  // exp2 units
    const int lo_q = DOC ? lo_s[qrow] : 0;
    __syncthreads();   // K t (and delta, for the dkv phase) visible

    f32x4 acc[DTILES];
#pragma unroll
    for (int t = 0; t < DTILES; ++t) acc[t] = f32x4{0, 0, 0, 0};
    const int blk_kv_end = min(seq, (kvl + 31) & ~31);  // uniform
    const int my_kv_end = live ? min(seq, r0 + 16) : 0;
    for (int kv0 = 0; kv0 < blk_kv_end; kv0 += 32) {
      if (kv0 >= my_kv_end) continue;
      const ushort* k_rm_t = k_rm + (kv0 >> 5) * RM;
      const ushort* v_rm_t = v_rm + (kv0 >> 5) * RM;
      const ushort* k_t_t = k_t + (kv0 >> 5) * TP;
      f32x4 s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
      f32x4 dp0 = {0, 0, 0, 0}, dp1 = {0, 0, 0, 0};
#pragma unroll
      for (int sl = 0; sl < DTILES / 2; ++sl) {
        const int c0 = 32 * sl + 8 * g;
        bf16x8 ka = load_frag_rm<DTILES>(k_rm_t, lane & 15, c0);
        bf16x8 kb2 = load_frag_rm<DTILES>(k_rm_t, 16 + (lane & 15), c0);
        bf16x8 va = load_frag_rm<DTILES>(v_rm_t, lane & 15, c0);
        bf16x8 vb2 = load_frag_rm<DTILES>(v_rm_t, 16 + (lane & 15), c0);
        s0 = mfma_bf16(ka, qb_[sl], s0);
        s1 = mfma_bf16(kb2, qb_[sl], s1);
        dp0 = mfma_bf16(va, dob[sl], dp0);
        dp1 = mfma_bf16(vb2, dob[sl], dp1);
      }
      if (c.thr) {
        const DropHashes dh = attn_drop_hashes(c, qrow, kv0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          dp0[r] = attn_drop_keep(dp0[r], dh.h0, r, geo.drop);
          dp1[r] = attn_drop_keep(dp1[r], dh.h1, r, geo.drop);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k0a = kv0 + 4 * g + r, k1a = k0a + 16;
        const float P0 = attn_visible<DOC>(qrow, k0a, kvl, lo_q)
                             ? __builtin_exp2f(s0[r] * c.sc2 - lse_q) : 0.f;
        const float P1 = attn_visible<DOC>(qrow, k1a, kvl, lo_q)
                             ? __builtin_exp2f(s1[r] * c.sc2 - lse_q) : 0.f;
        s0[r] = P0 * (dp0[r] - dlt_q);
        s1[r] = P1 * (dp1[r] - dlt_q);
      }
      bf16x8 dsa = scores_to_afrag(s0, s1, lane);
#pragma unroll
      for (int t = 0; t < DTILES; ++t) {
        bf16x8 kcb = load_frag_col_lds(k_t_t, 8 * g, 16 * t + (lane & 15));
        acc[t] = mfma_bf16(dsa, kcb, acc[t]);
      }
    }
    if (live)
      store_acc_tile<DTILES>(dq + c.b * geo.dq.batch + c.h * geo.dq.head,
                             geo.dq.seq, r0, seq, lane, acc,
                             f32x4{geo.scale, geo.scale, geo.scale,
                                   geo.scale});
  }

  // ---- dkv phase: attn_bwd_dkv_k<.., false> for key rows r0..r0+15 ----
  const int krow = row;
  bf16x8 kb_[DTILES / 2], vbf[DTILES / 2];
#pragma unroll
  for (int sl = 0; sl < DTILES / 2; ++sl) {
    kb_[sl] = load_frag_head<DTILES>(k_rm, krow, 32 * sl + 8 * g);
    vbf[sl] = load_frag_head<DTILES>(v_rm, krow, 32 * sl + 8 * g);
  }
  __syncthreads();   // every wave is done with K rm | V rm | K t
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) {
    stage_tile<DTILES, true>(q_t + t2 * TP, q_rm + t2 * RM, PITCH, 0, 32,
                             c.tid);
    stage_tile<DTILES, true>(d_t + t2 * TP, d_rm + t2 * RM, PITCH, 0, 32,
                             c.tid);
  }
  __syncthreads();

  f32x4 acck[DTILES], accv[DTILES];
#pragma unroll
  for (int t = 0; t < DTILES; ++t) {
    acck[t] = f32x4{0, 0, 0, 0};
    accv[t] = f32x4{0, 0, 0, 0};
  }
  // all 64 key rows padding: zero dk/dv, skip the walk (uniform)
  const int q_start = (0 >= kvl) ? seq : 0;
  for (int q0 = q_start; q0 < seq; q0 += 32) {
    if (!live || q0 + 31 < r0) continue;   // fully below the diagonal
    const ushort* q_rm_t = q_rm + (q0 >> 5) * RM;
    const ushort* d_rm_t = d_rm + (q0 >> 5) * RM;
    f32x4 s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
    f32x4 dp0 = {0, 0, 0, 0}, dp1 = {0, 0, 0, 0};
#pragma unroll
    for (int sl = 0; sl < DTILES / 2; ++sl) {
      const int c0 = 32 * sl + 8 * g;
      bf16x8 qa = load_frag_rm<DTILES>(q_rm_t, lane & 15, c0);
      bf16x8 qa1 = load_frag_rm<DTILES>(q_rm_t, 16 + (lane & 15), c0);
      s0 = mfma_bf16(qa, kb_[sl], s0);
      s1 = mfma_bf16(qa1, kb_[sl], s1);
      bf16x8 doa = load_frag_rm<DTILES>(d_rm_t, lane & 15, c0);
      bf16x8 doa1 = load_frag_rm<DTILES>(d_rm_t, 16 + (lane & 15), c0);
      dp0 = mfma_bf16(doa, vbf[sl], dp0);
      dp1 = mfma_bf16(doa1, vbf[sl], dp1);
    }
    f32x4 p0, p1, ds0, ds1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qa0 = q0 + 4 * g + r, qa1 = qa0 + 16;
      const bool v0 = qa0 < seq &&
          attn_visible<DOC>(qa0, krow, kvl, DOC ? lo_s[qa0] : 0);
      const bool v1 = qa1 < seq &&
          attn_visible<DOC>(qa1, krow, kvl, DOC ? lo_s[qa1] : 0);
      const float l0 = lse_s[v0 ? qa0 : 0] * LOG2E;
      const float l1 = lse_s[v1 ? qa1 : 0] * LOG2E;
      p0[r] = v0 ? __builtin_exp2f(s0[r] * c.sc2 - l0) : 0.f;
      p1[r] = v1 ? __builtin_exp2f(s1[r] * c.sc2 - l1) : 0.f;
      const float d0 = dlt_s[(qa0 < seq) ? qa0 : 0];
      const float d1 = dlt_s[(qa1 < seq) ? qa1 : 0];
      if (c.thr) {
        const uint64_t hk0 =
            rng_attn_hash(c.drop_s2, uint32_t(qa0), uint32_t(krow) >> 2);
        const uint64_t hk1 =
            rng_attn_hash(c.drop_s2, uint32_t(qa1), uint32_t(krow) >> 2);
        const float m0 =
            rng_keep(hk0, krow & 3, c.thr) ? geo.drop.inv_keep : 0.f;
        const float m1 =
            rng_keep(hk1, krow & 3, c.thr) ? geo.drop.inv_keep : 0.f;
        ds0[r] = p0[r] * (m0 * dp0[r] - d0);
        ds1[r] = p1[r] * (m1 * dp1[r] - d1);
        p0[r] *= m0;
        p1[r] *= m1;
      } else {
        ds0[r] = p0[r] * (dp0[r] - d0);
        ds1[r] = p1[r] * (dp1[r] - d1);
      }
    }
    bf16x8 pa = scores_to_afrag(p0, p1, lane);
    bf16x8 dsa = scores_to_afrag(ds0, ds1, lane);
    const ushort* d_t_t = d_t + (q0 >> 5) * TP;
    const ushort* q_t_t = q_t + (q0 >> 5) * TP;
#pragma unroll
    for (int t = 0; t < DTILES; ++t) {
      bf16x8 dob2 = load_frag_col_lds(d_t_t, 8 * g, 16 * t + (lane & 15));
      accv[t] = mfma_bf16(pa, dob2, accv[t]);
      bf16x8 qcb = load_frag_col_lds(q_t_t, 8 * g, 16 * t + (lane & 15));
      acck[t] = mfma_bf16(dsa, qcb, acck[t]);
    }
  }
  if (!live) return;
  ushort* dkp = dk + c.b * geo.dkv.batch + c.h * geo.dkv.head;
  ushort* dvp = dv + c.b * geo.dkv.batch + c.h * geo.dkv.head;
  for_acc_rows<DTILES>(r0, seq, lane, [&](int t, int r, int rw, int col) {
    dkp[int64_t(rw) * geo.dkv.seq + col] = f2bf(acck[t][r] * geo.scale);
    dvp[int64_t(rw) * geo.dkv.seq + col] = f2bf(accv[t][r]);
  });
}

// ---------------- decode (KV-cache serving path) ----------------
// One new query per (b,h) against a cached K/V of length kvlen (no mask:
// every cached key is attended). ONE BLOCK per (b,h): the 4 waves split
// the cache into interleaved 64-key chunks (4x the scan parallelism of
// the round-1 wave-per-head layout, which left batch-1 GPT-2/Llama with
// 8 workgroups on 256 CUs and measured 2 ms/token in the llama decode),
// each wave online-softmaxing its subset; a flash-decoding LDS combine
// (m*, rescaled l and acc) merges the four partials. Phase 2 unrolls
// the V-row walk 2-deep to keep two row loads in flight.
template <int DTILES>  // D = 16*DTILES; CPL = D/64 columns per lane
__global__ void attn_decode_k(const ushort* __restrict__ q,   // [B,H,D]
                              const ushort* __restrict__ kc,  // [B,Hk,L,D]
                              const ushort* __restrict__ vc,
                              ushort* __restrict__ o,         // [B,H,D]
                              int B, int H, int grp, int kvlen,
                              const int* __restrict__ len_p,  // device pos
                              int64_t cb, int64_t ch,  // cache strides
                              float scale) {
  constexpr int D = 16 * DTILES;
  constexpr int CPL = D / 64;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int bh = blockIdx.x;
  if (bh >= B * H) return;
  // hipGraph-replayable serving: the valid cache length comes from a
  // device counter (the append wrote row *len_p, so attend *len_p + 1)
  if (len_p) kvlen = *len_p + 1;
  const int b = bh / H, h = bh % H;
  const int hk = h / grp;
  const ushort* qp = q + (int64_t(b) * H + h) * D;
  const ushort* kp = kc + b * cb + hk * ch;
  const ushort* vp = vc + b * cb + hk * ch;
  const float sc2 = scale * LOG2E;

  // full query register-resident (bf16 pairs -> fp32 on use)
  float qr[D];
#pragma unroll
  for (int i = 0; i < D; i += 8) {
    s16x8 vq = *reinterpret_cast<const s16x8*>(qp + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) qr[i + j] = bf2f(ushort(vq[j]));
  }

  __shared__ float p_all[4][64];
  __shared__ float comb_m[4], comb_l[4];
  __shared__ float comb_acc[4][D];
  float* p = p_all[wid];
  float m_run = -INFINITY, l_run = 0.f;
  float acc[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) acc[c] = 0.f;

  // wave wid owns interleaved chunks s0 = (wid + 4i) * 64
  for (int s0 = wid * 64; s0 < kvlen; s0 += 4 * 64) {
    // phase 1: this lane's key
    const int srow = s0 + lane;
    float sc = -INFINITY;
    if (srow < kvlen) {
      const ushort* kr = kp + int64_t(srow) * D;
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < D; i += 8) {
        s16x8 vk = *reinterpret_cast<const s16x8*>(kr + i);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          dot = fmaf(qr[i + j], bf2f(ushort(vk[j])), dot);
      }
      sc = dot * sc2;
    }
    float mx = sc;
#pragma unroll
    for (int off = 32; off; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    const float m_new = fmaxf(m_run, mx);
    const float pj = (sc == -INFINITY) ? 0.f : __builtin_exp2f(sc - m_new);
    float ps = pj;
#pragma unroll
    for (int off = 32; off; off >>= 1) ps += __shfl_xor(ps, off);
    const float alpha =
        (m_run == -INFINITY) ? 0.f : __builtin_exp2f(m_run - m_new);
    l_run = l_run * alpha + ps;
    m_run = m_new;
    p[lane] = pj;
    __threadfence_block();   // wave-local LDS visibility
    // phase 2: lane owns CPL output columns; 2-deep V-row pipeline
    const int n = min(64, kvlen - s0);
#pragma unroll
    for (int c = 0; c < CPL; ++c) acc[c] *= alpha;
    int s_ = 0;
    for (; s_ + 2 <= n; s_ += 2) {
      const ushort* vr0 = vp + int64_t(s0 + s_) * D;
      const ushort* vr1 = vr0 + D;
      float va0[CPL], va1[CPL];
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        va0[c] = bf2f(vr0[64 * c + lane]);
        va1[c] = bf2f(vr1[64 * c + lane]);
      }
      const float p0 = p[s_], p1 = p[s_ + 1];
#pragma unroll
      for (int c = 0; c < CPL; ++c)
        acc[c] = fmaf(p1, va1[c], fmaf(p0, va0[c], acc[c]));
    }
    if (s_ < n) {
      const ushort* vr = vp + int64_t(s0 + s_) * D;
      const float ps_ = p[s_];
#pragma unroll
      for (int c = 0; c < CPL; ++c)
        acc[c] = fmaf(ps_, bf2f(vr[64 * c + lane]), acc[c]);
    }
    __threadfence_block();   // p reads done before next chunk overwrites
  }
  // flash-decoding combine of the 4 wave-partials via LDS
  if (lane == 0) {
    comb_m[wid] = m_run;
    comb_l[wid] = l_run;
  }
#pragma unroll
  for (int c = 0; c < CPL; ++c) comb_acc[wid][64 * c + lane] = acc[c];
  __syncthreads();
  if (wid == 0) {
    float mg = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) mg = fmaxf(mg, comb_m[w]);
    float lg = 0.f;
    float r[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      r[w] = (comb_m[w] == -INFINITY) ? 0.f
                                      : __builtin_exp2f(comb_m[w] - mg);
      lg += comb_l[w] * r[w];
    }
    const float inv = lg > 0.f ? 1.0f / lg : 0.f;
    ushort* op = o + (int64_t(b) * H + h) * D;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        s = fmaf(comb_acc[w][64 * c + lane], r[w], s);
      op[64 * c + lane] = f2bf(s * inv);
    }
  }
}

// ---------------- decode, split-KV route (long-context GQA serving) --------
// One block per (KV split, KV head, batch row): the grp <= 16 query heads of
// a KV head are the 16 columns of one MFMA tile, so K and V leave HBM once
// per KV head, and a long cache is cut into nsplit independent blocks whose
// fp32 partials (m, l, acc) attn_decode_combine_k merges in index order.
//   * The 4 waves take the split's 32-key tiles interleaved and never meet
//     in the loop: each has a V tile of its own in LDS, ordered by
//     wave-scope fences only (a wave's LDS operations execute in order).
//   * Scores, swapped as in attn_fwd_k: mfma(A = K tile, B = Q^T). Q^T is
//     D/32 B-fragments held for the whole block (column n = head hk*grp + n,
//     zero for n >= grp). K goes from global memory straight into the
//     A-fragments: lane (n, g) loads 16 B of key row n at column 32*step +
//     8g, every element is used by exactly one lane.
//   * P.V without moving P: the score tiles p0, p1 in C layout (key 4g + r
//     and 16 + 4g + r of query n) ARE a B-fragment of the 32-deep MFMA once
//     contraction slot 8g + j is read as key 16*(j >> 2) + 4g + (j & 3).
//     The A-fragment (V^T: row d, same key order) is two 8 B reads of the
//     transposed [D][DEC_VP] tile. The product is O^T: acc[t][r] is column
//     d = 16t + 4g + r of query n, so alpha, l and 1/l are per lane, and a
//     lane stores 4 consecutive columns.
//   * Loads run one tile ahead in registers: K(i+1) is issued after the
//     score MFMAs of tile i, V(i+1) after V(i) went to LDS. Rows are clamped
//     into the split, so the look-ahead past the last tile re-reads its last
//     row instead of branching (a branch made the compiler drain the loads).
// Rounding points: P is rounded to bf16 before P.V, l sums the unrounded
// fp32 p (as attn_fwd_k), partials are fp32, o is rounded once.
constexpr int DEC_VP = 36;   // V^T tile pitch: 32 keys + 4 (18 dwords: the 4
                             // lane groups of a staging write hit 4 bank sets)

// 16 B of cache row `row` (clamped below `end`) at column c0
DEV s16x8 dec_load(const ushort* base, int row, int end, int D, int c0) {
  return *reinterpret_cast<const s16x8*>(
      base + int64_t(row < end ? row : end - 1) * D + c0);
}

// K A-fragments of the 32-key tile at kv0: rows kv0 + n and kv0 + 16 + n
template <int DTILES>
DEV void dec_load_k(s16x8 (&ka)[DTILES / 2], s16x8 (&kb)[DTILES / 2],
                    const ushort* kp, int kv0, int end, int lane) {
  const int n = lane & 15, g = lane >> 4;
#pragma unroll
  for (int sl = 0; sl < DTILES / 2; ++sl) {
    ka[sl] = dec_load(kp, kv0 + n, end, 16 * DTILES, 32 * sl + 8 * g);
    kb[sl] = dec_load(kp, kv0 + 16 + n, end, 16 * DTILES, 32 * sl + 8 * g);
  }
}
// V tile at kv0: vr[it] is row n + 16*(it & 1), 16 B chunk g + 4*(it >> 1)
template <int DTILES>
DEV void dec_load_v(s16x8 (&vr)[DTILES], const ushort* vp, int kv0, int end,
                    int lane) {
  const int n = lane & 15, g = lane >> 4;
#pragma unroll
  for (int it = 0; it < DTILES; ++it)
    vr[it] = dec_load(vp, kv0 + n + 16 * (it & 1), end, 16 * DTILES,
                      8 * (g + 4 * (it >> 1)));
}

// A split with no valid key: o = 0 when it is the only split, else m = -inf
// (attn_decode_combine_k skips the row). bh0: b * H + first head of the group.
template <int D>
DEV void dec_split_empty(ushort* o, float* ws, int64_t bh0, int grp, int split,
                         int nsplit, int tid) {
  if (tid >= grp) return;
  if (nsplit == 1) {
    for (int c = 0; c < D; ++c) o[(bh0 + tid) * D + c] = 0;
  } else {
    float* row = ws + ((bh0 + tid) * nsplit + split) * dta_decode_split_row(D);
    *reinterpret_cast<f32x4*>(row + D) = f32x4{-INFINITY, 0.f, 0.f, 0.f};
  }
}

// Tail of a split block: the 4 wave partials (m, l of query n = lane & 15,
// acc[t][r] = column 16t + 4g + r) merged in wave order through LDS, then o
// (nsplit == 1) or the split's workspace row. smem: >= DEC_COMB(D) floats.
constexpr int DEC_COMB(int D) { return 128 + 4 * 16 * D; }  // m, l [4][16], acc
template <int DTILES>
DEV void dec_split_merge(char* smem, const f32x4 (&acc)[DTILES], float m_run,
                         float l_run, ushort* o, float* ws, int64_t bh0,
                         int grp, int split, int nsplit) {
  constexpr int D = 16 * DTILES;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  // merge of the 4 wave partials, 16 columns wide; the V tiles are dead
  __syncthreads();
  float* cm = reinterpret_cast<float*>(smem);   // [4][16]
  float* cl = cm + 64;                          // [4][16]
  float* ca = cl + 64;                          // [4][16][D]
  if (g == 0) {
    cm[wid * 16 + n] = m_run;
    cl[wid * 16 + n] = l_run;
  }
#pragma unroll
  for (int t = 0; t < DTILES; ++t)
    *reinterpret_cast<f32x4*>(ca + (wid * 16 + n) * D + 16 * t + 4 * g) =
        acc[t];
  __syncthreads();
  for (int u = tid; u < 4 * D; u += 256) {   // (head, 4 columns) units
    const int hn = u / (D / 4), d4 = (u % (D / 4)) * 4;
    if (hn >= grp) continue;
    float mg = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) mg = fmaxf(mg, cm[w * 16 + hn]);
    float lg = 0.f;
    f32x4 s = {0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float mw = cm[w * 16 + hn];
      const float r = (mw == -INFINITY) ? 0.f : __builtin_exp2f(mw - mg);
      lg += cl[w * 16 + hn] * r;
      const f32x4 a =
          *reinterpret_cast<const f32x4*>(ca + (w * 16 + hn) * D + d4);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = fmaf(a[e], r, s[e]);
    }
    const int64_t bh = bh0 + hn;
    if (nsplit == 1) {
      const float inv = lg > 0.f ? 1.0f / lg : 0.f;
      s16x4 ob;
#pragma unroll
      for (int e = 0; e < 4; ++e) ob[e] = short(f2bf(s[e] * inv));
      *reinterpret_cast<s16x4*>(o + bh * D + d4) = ob;
    } else {
      float* row = ws + (bh * nsplit + split) * dta_decode_split_row(D);
      *reinterpret_cast<f32x4*>(row + d4) = s;
      if (d4 == 0) *reinterpret_cast<f32x4*>(row + D) = f32x4{mg, lg, 0.f, 0.f};
    }
  }
}

template <int DTILES>  // D = 16*DTILES
__global__ __launch_bounds__(256)
__attribute__((target("no-packed-fp32-ops")))
void attn_decode_split_k(const ushort* __restrict__ q,   // [B,H,D]
                         const ushort* __restrict__ kc,  // [B,Hk,Lmax,D]
                         const ushort* __restrict__ vc,
                         ushort* __restrict__ o,         // [B,H,D]
                         float* __restrict__ ws,  // [B,H,nsplit,D+4]
                         int H, int grp, int Lmax, int kvlen,
                         const int* __restrict__ len_p, int64_t cb, int64_t ch,
                         int chunk, float scale) {
  constexpr int D = 16 * DTILES;
  constexpr int KS = DTILES / 2;            // 32-column steps of a K row
  constexpr int VT = D * DEC_VP;            // ushorts of one wave's V^T tile
  constexpr int COMB = DEC_COMB(D);         // floats of the merge
  constexpr int SMEM = 4 * VT * 2 > COMB * 4 ? 4 * VT * 2 : COMB * 4;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int split = blockIdx.x, nsplit = gridDim.x;
  const int hk = blockIdx.y, b = blockIdx.z;
  if (len_p) kvlen = *len_p + 1;
  kvlen = min(kvlen, Lmax);
  const int start = split * chunk;
  const int end = min(kvlen, start + chunk);
  const int h0 = hk * grp;

  if (start >= end) {   // block-uniform: nothing of this split is valid yet
    dec_split_empty<D>(o, ws, int64_t(b) * H + h0, grp, split, nsplit, tid);
    return;
  }

  const ushort* kp = kc + b * cb + hk * ch;
  const ushort* vp = vc + b * cb + hk * ch;
  const float sc2 = scale * LOG2E;

  // Q^T B-fragments: lane (n, g) holds q[head h0 + n][32*sl + 8g .. + 7]
  bf16x8 qb[KS];
  {
    const ushort* qp = q + (int64_t(b) * H + h0 + min(n, grp - 1)) * D;
#pragma unroll
    for (int sl = 0; sl < KS; ++sl) {
      s16x8 v = *reinterpret_cast<const s16x8*>(qp + 32 * sl + 8 * g);
      if (n >= grp) v = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
      qb[sl] = as_bf16x8(v);
    }
  }

  f32x4 acc[DTILES];
#pragma unroll
  for (int t = 0; t < DTILES; ++t) acc[t] = f32x4{0, 0, 0, 0};
  float m_run = -INFINITY, l_run = 0.f;   // of query n, in exp2 units

  ushort* vt = reinterpret_cast<ushort*>(smem) + wid * VT;
  s16x8 ka[KS], kb[KS];   // key rows kv0 + n and kv0 + 16 + n
  s16x8 vr[DTILES];
  // wave wid owns tiles wid, wid + 4, ... of the split (wave-uniform loop)
  int kv0 = start + 32 * wid;
  dec_load_k<DTILES>(ka, kb, kp, kv0, end, lane);   // clamped: in bounds
  // K before V here as in the loop: the wait for K at the loop top is
  // counted against the entry that has more loads issued after K
  __builtin_amdgcn_sched_barrier(0);
  dec_load_v<DTILES>(vr, vp, kv0, end, lane);
  for (; kv0 < end; kv0 += 128) {
    f32x4 p0 = {0, 0, 0, 0}, p1 = {0, 0, 0, 0};
#pragma unroll
    for (int sl = 0; sl < KS; ++sl) {
      p0 = mfma_bf16(as_bf16x8(ka[sl]), qb[sl], p0);
      p1 = mfma_bf16(as_bf16x8(kb[sl]), qb[sl], p1);
    }
    // clamped: in bounds even past the last tile
    dec_load_k<DTILES>(ka, kb, kp, kv0 + 128, end, lane);

    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k0a = kv0 + 4 * g + r;
      p0[r] = k0a < end ? p0[r] * sc2 : -INFINITY;
      p1[r] = k0a + 16 < end ? p1[r] * sc2 : -INFINITY;
      mx = fmaxf(mx, fmaxf(p0[r], p1[r]));
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);   // finite: key kv0 is valid
    const float alpha =
        (m_run == -INFINITY) ? 0.f : __builtin_exp2f(m_run - m_new);
    float pf[8];
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pf[r] = (p0[r] == -INFINITY) ? 0.f : __builtin_exp2f(p0[r] - m_new);
      pf[4 + r] = (p1[r] == -INFINITY) ? 0.f : __builtin_exp2f(p1[r] - m_new);
      psum += pf[r] + pf[4 + r];
    }
    psum += __shfl_xor(psum, 16);
    psum += __shfl_xor(psum, 32);
    l_run = l_run * alpha + psum;
    m_run = m_new;
    // slot 8g + j of the contraction = key 16*(j >> 2) + 4g + (j & 3)
    const bf16x8 pb = pack_bf16x8(pf);

    // V(i) registers -> transposed tile; the previous tile's reads are done
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < DTILES; ++it) {
      const int row = n + 16 * (it & 1), c8 = 8 * (g + 4 * (it >> 1));
#pragma unroll
      for (int j = 0; j < 8; ++j)
        vt[(c8 + j) * DEC_VP + row] = ushort(vr[it][j]);
    }
    dec_load_v<DTILES>(vr, vp, kv0 + 128, end, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < DTILES; ++t) {
      const ushort* vrow = vt + (16 * t + n) * DEC_VP + 4 * g;
      const s16x4 lo = *reinterpret_cast<const s16x4*>(vrow);
      const s16x4 hi = *reinterpret_cast<const s16x4*>(vrow + 16);
      const bf16x8 va =
          as_bf16x8(__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      acc[t] *= alpha;
      acc[t] = mfma_bf16(va, pb, acc[t]);
    }
  }

  dec_split_merge<DTILES>(smem, acc, m_run, l_run, o, ws,
                          int64_t(b) * H + h0, grp, split, nsplit);
}

// ---------------- decode, split-KV route on an int8 KV cache ---------------
// The int8 sibling of attn_decode_split_k (format: docs/serving.md): caches
// are int8 codes [B,Hk,Lmax,D] with one fp32 scale per (token, KV head) row in
// [B,Hk,Lp], value = float(code) * scale. Same decomposition (one block per
// split, KV head and batch row, 4 waves on interleaved 32-key tiles, the head
// group as the 16 MFMA columns), the same wave merge and workspace rows, so
// attn_decode_combine_k finishes it. The cache bytes per key drop from 4 D to
// 2 D + 8. How the codes move is this kernel's own:
//   * No code is ever multiplied by its scale. A code is an integer of
//     |q| <= 127, exact in bf16, so the MFMAs run on the converted codes and
//     the per-key scales are applied where a key is a C-layout row (K) or the
//     contraction index (V).
//   * K: lane (n, g) loads 16 B = 16 codes of key row n at column 64 s + 16 g
//     (D/64 loads per row: half the bf16 kernel's). Codes 8 j .. 8 j + 7 are
//     the A-fragment of MFMA (s, j), as in w8_gemv.hip: contraction slot
//     8 g + e of that MFMA stands for column 64 s + 16 g + 8 j + e, and the
//     Q^T B-fragments qb[s][j] are loaded once per block in that order. The
//     raw score of key 4 g + r (p0) and 16 + 4 g + r (p1) is multiplied by
//     k_scale[key] * scale * log2e before the mask and the max; the lane
//     loads its 2 x 4 K scales as two 16 B vectors.
//   * V: lane (kq, c) = (lane >> 3, lane & 7) loads D/8 bytes of the 4 key
//     rows 4 kq .. 4 kq + 3 at column c D/8, transposes each 4 x 4 byte block
//     in registers (v_perm_b32) and writes dwords of 4 keys x 1 column into
//     the wave's transposed CODE tile [D][DQ8_VP bytes]. The codes convert
//     to bf16 on the FRAGMENT READ (two 4 B LDS reads -> one A-fragment),
//     not on the staging write: a lane converts 32 D / 64 codes either way
//     (every tile element belongs to one lane on both sides), but a byte
//     tile halves the LDS footprint and the LDS read traffic, and the
//     staging writes stay whole dwords.
//   * The per-key V scale is folded into P: pb = bf16(p * v_scale[key]) with
//     the key the contraction index of P.V, so acc needs no rescale beyond
//     alpha. l sums the unscaled, unrounded fp32 p.
//   * Loads run one tile ahead in registers (K codes and the 4 scale vectors
//     after the score MFMAs, V codes after the staging write). Rows are
//     clamped into the split and the scale vectors to the split's last tile,
//     so nothing branches around a load; every branch is block- or
//     wave-uniform. Masked keys select 0 / -inf, never multiply, so the
//     scales past kvlen may hold anything.
//   * Scale padding: a scale vector load covers keys 32 i + 4 g .. + 3 of a
//     tile that holds at least one valid key, i.e. indices below
//     ceil32(Lmax). Hence Lp >= dta_kv_q8_scale_len(Lmax) = Lmax rounded up
//     to a multiple of 32, and Lp % 4 == 0 keeps every row 16 B aligned.
// Rounding points: p * v_scale is rounded to bf16 once; scores, p, l, alpha,
// the accumulators and all partials are fp32; o is rounded once.
typedef __attribute__((ext_vector_type(4))) int i32x4;
template <int N> using i32xN = int __attribute__((ext_vector_type(N)));
constexpr int DQ8_VP = 36;   // bytes per V^T code row: 32 keys + 4 (9 dwords)

template <int DTILES>
DEV void dq8_load_k(i32x4 (&ka)[DTILES / 4], i32x4 (&kb)[DTILES / 4],
                    const char* kp, int kv0, int end, int lane) {
  constexpr int D = 16 * DTILES;
  const int n = lane & 15, g = lane >> 4;
  const int ra = min(kv0 + n, end - 1), rb = min(kv0 + 16 + n, end - 1);
#pragma unroll
  for (int s = 0; s < DTILES / 4; ++s) {
    ka[s] = *reinterpret_cast<const i32x4*>(kp + int64_t(ra) * D + 64 * s +
                                            16 * g);
    kb[s] = *reinterpret_cast<const i32x4*>(kp + int64_t(rb) * D + 64 * s +
                                            16 * g);
  }
}
// sc[0], sc[1]: K scales of keys 4g + r and 16 + 4g + r of the tile at kv0;
// sc[2], sc[3]: the V scales. Past the split: its last tile again.
DEV void dq8_load_scales(f32x4 (&sc)[4], const float* ksp, const float* vsp,
                         int kv0, int end, int g) {
  const int tb = (kv0 < end ? kv0 : ((end - 1) & ~31)) + 4 * g;
  sc[0] = *reinterpret_cast<const f32x4*>(ksp + tb);
  sc[1] = *reinterpret_cast<const f32x4*>(ksp + tb + 16);
  sc[2] = *reinterpret_cast<const f32x4*>(vsp + tb);
  sc[3] = *reinterpret_cast<const f32x4*>(vsp + tb + 16);
}
// vr[i]: D/8 bytes of key row kv0 + 4 kq + i at column c D/8
template <int DTILES>
DEV void dq8_load_v(i32xN<DTILES / 2> (&vr)[4], const char* vp, int kv0,
                    int end, int lane) {
  constexpr int D = 16 * DTILES;
  const int kq = lane >> 3, c = lane & 7;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    vr[i] = *reinterpret_cast<const i32xN<DTILES / 2>*>(
        vp + int64_t(min(kv0 + 4 * kq + i, end - 1)) * D + c * (D / 8));
}

template <int DTILES>  // D = 16*DTILES
__global__ __launch_bounds__(256)
__attribute__((target("no-packed-fp32-ops")))
void attn_decode_split_q8_k(const ushort* __restrict__ q,   // [B,H,D]
                            const char* __restrict__ kc,    // [B,Hk,Lmax,D]
                            const char* __restrict__ vc,
                            const float* __restrict__ ksc,  // [B,Hk,Lp]
                            const float* __restrict__ vsc,
                            ushort* __restrict__ o,         // [B,H,D]
                            float* __restrict__ ws,  // [B,H,nsplit,D+4]
                            int H, int grp, int Lmax, int Lp, int kvlen,
                            const int* __restrict__ len_p, int chunk,
                            float scale) {
  constexpr int D = 16 * DTILES;
  constexpr int KS = DTILES / 4;            // 64-column steps of a K row
  constexpr int VW = DTILES / 2;            // dwords of a lane's V row piece
  constexpr int VT = D * DQ8_VP;            // bytes of one wave's V^T tile
  constexpr int COMB = DEC_COMB(D);         // floats of the merge
  constexpr int SMEM = 4 * VT > COMB * 4 ? 4 * VT : COMB * 4;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int split = blockIdx.x, nsplit = gridDim.x;
  const int hk = blockIdx.y, Hk = gridDim.y, b = blockIdx.z;
  if (len_p) kvlen = *len_p + 1;
  kvlen = min(kvlen, Lmax);
  const int start = split * chunk;
  const int end = min(kvlen, start + chunk);
  const int h0 = hk * grp;

  if (start >= end) {   // block-uniform: nothing of this split is valid yet
    dec_split_empty<D>(o, ws, int64_t(b) * H + h0, grp, split, nsplit, tid);
    return;
  }

  const int64_t bhk = int64_t(b) * Hk + hk;
  const char* kp = kc + bhk * Lmax * D;
  const char* vp = vc + bhk * Lmax * D;
  const float* ksp = ksc + bhk * Lp;
  const float* vsp = vsc + bhk * Lp;
  const float sc2 = scale * LOG2E;

  // Q^T B-fragments: qb[s][j] of lane (n, g) = q[h0 + n][64s + 16g + 8j ..]
  bf16x8 qb[KS][2];
  {
    const ushort* qp = q + (int64_t(b) * H + h0 + min(n, grp - 1)) * D;
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        s16x8 v =
            *reinterpret_cast<const s16x8*>(qp + 64 * s + 16 * g + 8 * j);
        if (n >= grp) v = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
        qb[s][j] = as_bf16x8(v);
      }
  }

  f32x4 acc[DTILES];
#pragma unroll
  for (int t = 0; t < DTILES; ++t) acc[t] = f32x4{0, 0, 0, 0};
  float m_run = -INFINITY, l_run = 0.f;   // of query n, in exp2 units

  char* vt = smem + wid * VT;
  const int kq = lane >> 3, vcol = (lane & 7) * (D / 8);
  i32x4 ka[KS], kb[KS];     // codes of key rows kv0 + n and kv0 + 16 + n
  f32x4 sc[4];              // K and V scales of the lane's 8 keys
  i32xN<VW> vr[4];
  // wave wid owns tiles wid, wid + 4, ... of the split (wave-uniform loop)
  int kv0 = start + 32 * wid;
  dq8_load_k<DTILES>(ka, kb, kp, kv0, end, lane);   // clamped: in bounds
  dq8_load_scales(sc, ksp, vsp, kv0, end, g);
  __builtin_amdgcn_sched_barrier(0);   // K before V, as in the loop
  dq8_load_v<DTILES>(vr, vp, kv0, end, lane);
  for (; kv0 < end; kv0 += 128) {
    f32x4 p0 = {0, 0, 0, 0}, p1 = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        p0 = mfma_bf16(codes_to_bf16(ka[s][2 * j], ka[s][2 * j + 1]),
                       qb[s][j], p0);
        p1 = mfma_bf16(codes_to_bf16(kb[s][2 * j], kb[s][2 * j + 1]),
                       qb[s][j], p1);
      }
    const f32x4 ksa = sc[0], ksb = sc[1], vsa = sc[2], vsb = sc[3];
    // clamped: in bounds even past the last tile
    dq8_load_k<DTILES>(ka, kb, kp, kv0 + 128, end, lane);
    dq8_load_scales(sc, ksp, vsp, kv0 + 128, end, g);

    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k0a = kv0 + 4 * g + r;
      p0[r] = k0a < end ? p0[r] * (ksa[r] * sc2) : -INFINITY;
      p1[r] = k0a + 16 < end ? p1[r] * (ksb[r] * sc2) : -INFINITY;
      mx = fmaxf(mx, fmaxf(p0[r], p1[r]));
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);   // finite: key kv0 is valid
    const float alpha =
        (m_run == -INFINITY) ? 0.f : __builtin_exp2f(m_run - m_new);
    float pv[8];
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool v0 = p0[r] != -INFINITY, v1 = p1[r] != -INFINITY;
      const float e0 = v0 ? __builtin_exp2f(p0[r] - m_new) : 0.f;
      const float e1 = v1 ? __builtin_exp2f(p1[r] - m_new) : 0.f;
      psum += e0 + e1;
      pv[r] = v0 ? e0 * vsa[r] : 0.f;
      pv[4 + r] = v1 ? e1 * vsb[r] : 0.f;
    }
    psum += __shfl_xor(psum, 16);
    psum += __shfl_xor(psum, 32);
    l_run = l_run * alpha + psum;
    m_run = m_new;
    // slot 8g + j of the contraction = key 16*(j >> 2) + 4g + (j & 3)
    const bf16x8 pb = pack_bf16x8(pv);

    // V(i) codes -> transposed tile; the previous tile's reads are done
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int w = 0; w < VW; ++w) {
      // 4 keys x 4 columns of bytes -> 4 columns x 4 keys (key 0 lowest)
      const int a0 = __builtin_amdgcn_perm(vr[1][w], vr[0][w], 0x05010400);
      const int a1 = __builtin_amdgcn_perm(vr[1][w], vr[0][w], 0x07030602);
      const int b0 = __builtin_amdgcn_perm(vr[3][w], vr[2][w], 0x05010400);
      const int b1 = __builtin_amdgcn_perm(vr[3][w], vr[2][w], 0x07030602);
      char* dst = vt + (vcol + 4 * w) * DQ8_VP + 4 * kq;
      *reinterpret_cast<int*>(dst) =
          __builtin_amdgcn_perm(b0, a0, 0x05040100);
      *reinterpret_cast<int*>(dst + DQ8_VP) =
          __builtin_amdgcn_perm(b0, a0, 0x07060302);
      *reinterpret_cast<int*>(dst + 2 * DQ8_VP) =
          __builtin_amdgcn_perm(b1, a1, 0x05040100);
      *reinterpret_cast<int*>(dst + 3 * DQ8_VP) =
          __builtin_amdgcn_perm(b1, a1, 0x07060302);
    }
    dq8_load_v<DTILES>(vr, vp, kv0 + 128, end, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < DTILES; ++t) {
      const char* vrow = vt + (16 * t + n) * DQ8_VP + 4 * g;
      const bf16x8 va =
          codes_to_bf16(*reinterpret_cast<const int*>(vrow),
                        *reinterpret_cast<const int*>(vrow + 16));
      acc[t] *= alpha;
      acc[t] = mfma_bf16(va, pb, acc[t]);
    }
  }

  dec_split_merge<DTILES>(smem, acc, m_run, l_run, o, ws,
                          int64_t(b) * H + h0, grp, split, nsplit);
}

// One wave per (b, h): m* over the splits, then l and acc rescaled and summed
// in split order, o rounded once. A fixed order: the result repeats bit for
// bit. An empty split (m = -inf) has no acc row and is skipped.
template <int DTILES>
__global__ __launch_bounds__(256)
__attribute__((target("no-packed-fp32-ops")))
void attn_decode_combine_k(const float* __restrict__ ws,
                           ushort* __restrict__ o, int BH, int nsplit) {
  constexpr int D = 16 * DTILES;
  constexpr int CPL = D / 64;
  const int lane = threadIdx.x & 63;
  const int bh = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (bh >= BH) return;
  const int64_t rs = dta_decode_split_row(D);
  const float* base = ws + int64_t(bh) * nsplit * rs;
  float mg = -INFINITY;
  for (int s = 0; s < nsplit; ++s) mg = fmaxf(mg, base[s * rs + D]);
  float lg = 0.f;
  float acc[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) acc[c] = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float* row = base + s * rs;
    const float ms = row[D];
    if (ms == -INFINITY) continue;   // wave-uniform
    const float r = __builtin_exp2f(ms - mg);
    lg += row[D + 1] * r;
#pragma unroll
    for (int c = 0; c < CPL; ++c)
      acc[c] = fmaf(row[64 * c + lane], r, acc[c]);
  }
  const float inv = lg > 0.f ? 1.0f / lg : 0.f;
#pragma unroll
  for (int c = 0; c < CPL; ++c)
    o[int64_t(bh) * D + 64 * c + lane] = f2bf(acc[c] * inv);
}

// ---------------- extend: Sq new queries on a filled KV cache --------------
// Chunked prefill, a second turn, verifying drafted tokens: Sq >= 1 queries
// per head at absolute positions P .. P + Sq - 1 attend P cached keys plus
// themselves (query i sees key j iff j <= P + i; the new rows are already
// appended). Neither attn_fwd_k (queries and keys share one index range) nor
// the decode kernels (one query) serve this.
//   * Rows are (position, head-in-group) pairs of ONE KV head, position-major:
//     r = i * grp + hn, Sq * grp rows. A block is 4 waves x 16 = 64 consecutive
//     r of (kv head, batch row); grid = (ceil(Sq grp / 64) * nsplit, Hk, B).
//     The 64 rows lie within ceil(64 / grp) + 1 positions, so the four waves
//     share one key walk and each K/V tile reaches LDS once per block for the
//     whole head group: K/V traffic per KV head is 1 / grp of one attn_fwd_k
//     pass per query head. A block boundary may fall inside a position's head
//     group (grp 7: 64 rows = 9 positions + 1 head); nothing relies on it not
//     doing so, position and head are derived per row. Rows >= Sq * grp are
//     padding: they load row Sq * grp - 1 again and are never stored.
//   * Scores swapped as in attn_fwd_k: mfma(A = K tile, B = Q^T), Q^T held
//     as D/32 B-fragments for the whole block, softmax reduce = two shfl_xor.
//     P.V without moving P, as in attn_decode_split_k: the score tiles in C
//     layout are the B-fragment, the A-fragment is V^T read as two 8 B LDS
//     loads, the product is O^T (acc[t][r] = column 16t + 4g + r of query
//     n), so alpha, l, 1/l are per lane and a lane stores 4 columns at once.
//   * LDS per block: K row-major 32 x (D + 8) and V^T D x LDS_RP bf16, one
//     pair: 8.5 + 10 KB at D = 128, 4.5 + 5 KB at D = 64.
//   * Loads run a tile ahead through registers (D/64 x 16 B of K and of V per
//     thread): tile t + 1 is requested right after tile t became visible in
//     LDS and lands during the MFMAs of tile t. Rows are clamped below P + Sq,
//     so the look-ahead past the last tile re-reads the last row instead of
//     branching (see attn_decode_split_k).
//   * The walk of a block: keys [split start, min(split end, P + last
//     position of the block + 1)), block-uniform. A tile whose last key is
//     <= P + first position of the block is visible to every row: those run
//     in the first loop with no compare. Only the tiles crossing the band of
//     the block's positions (<= 3 for grp >= 1: 64 rows span <= 65 keys) take
//     the per-row compare `key <= P + i`, which is the whole mask: it implies
//     key < P + Sq, and splits start and end on tile boundaries.
//   * nsplit > 1 (few rows, long prefix): split s owns keys [s chunk,
//     (s + 1) chunk), chunk a multiple of 32; the block writes fp32 (acc, m, l)
//     per (row, split) in the dta_decode_split_row format and
//     attn_decode_combine_k merges B * Sq * H rows in split order. A row that
//     sees no key of its split keeps m = -inf, l = 0, acc = 0 (alpha and p
//     are guarded, no exp2 of inf - inf) and the combine skips it.
// Rounding points: P is rounded to bf16 before P.V with the running max
// after the current tile, l sums the unrounded fp32 p, partials are fp32, o
// is rounded once.
template <int DTILES>
DEV void ext_load_tile(s16x8 (&kr)[DTILES / 4], s16x8 (&vr)[DTILES / 4],
                       const ushort* kp, const ushort* vp, int kv0, int kvl,
                       int tid) {
  constexpr int CPR = 2 * DTILES;       // 16B chunks per row (D/8)
#pragma unroll
  for (int c = 0; c < DTILES / 4; ++c) {
    const int i = tid + 256 * c;
    const int64_t off =
        int64_t(clamp_row(kv0 + i / CPR, kvl)) * (16 * DTILES) + (i % CPR) * 8;
    kr[c] = *reinterpret_cast<const s16x8*>(kp + off);
    vr[c] = *reinterpret_cast<const s16x8*>(vp + off);
  }
}
// the LDS layouts of stage_tile: K row-major, V transposed
template <int DTILES>
DEV void ext_store_tile(ushort* k_rm, ushort* v_t,
                        const s16x8 (&kr)[DTILES / 4],
                        const s16x8 (&vr)[DTILES / 4], int tid) {
  constexpr int CPR = 2 * DTILES;
#pragma unroll
  for (int c = 0; c < DTILES / 4; ++c) {
    const int i = tid + 256 * c;
    const int r = i / CPR, c8 = (i % CPR) * 8;
    *reinterpret_cast<s16x8*>(k_rm + r * LDS_RM_PITCH<DTILES> + c8) = kr[c];
#pragma unroll
    for (int j = 0; j < 8; ++j) v_t[(c8 + j) * LDS_RP + r] = ushort(vr[c][j]);
  }
}

template <int DTILES>  // D = 16*DTILES
__global__ __launch_bounds__(256)
void attn_extend_k(const ushort* __restrict__ q,    // [B,H,Sq,D] view
                   const ushort* __restrict__ kc,   // [B,Hk,Lmax,D]
                   const ushort* __restrict__ vc,
                   ushort* __restrict__ o,          // [B,Sq,H,D]
                   float* __restrict__ ws,  // [B,Sq,H,nsplit,D+4]
                   ExtGeom geo) {
  constexpr int D = 16 * DTILES;
  constexpr int KS = DTILES / 2;            // 32-column steps of a K row
  __shared__ __attribute__((aligned(16))) ushort k_rm[LDS_RM_SIZE<DTILES>];
  __shared__ __attribute__((aligned(16))) ushort v_t[LDS_T_SIZE<DTILES>];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int blk = int(blockIdx.x) / geo.nsplit;
  const int split = int(blockIdx.x) % geo.nsplit;
  const int hk = blockIdx.y, b = blockIdx.z;
  const int grp = geo.grp, P = geo.P;
  const int R = geo.Sq * grp;               // rows of this KV head
  const int kvl = P + geo.Sq;               // valid cache rows

  // this lane's query row (column n of the wave's Q^T), clamped into R
  const int r0 = blk * 64 + wid * 16;
  const int row = r0 + n;
  const int rc = min(row, R - 1);
  const int qi = rc / grp;                  // position within the Sq
  const int h = hk * grp + (rc - qi * grp);
  const int qlim = P + qi;                  // last key this row sees

  bf16x8 qb[KS];
  {
    const ushort* qp = q + b * geo.q_batch + h * geo.q_head + qi * geo.q_seq;
#pragma unroll
    for (int sl = 0; sl < KS; ++sl)
      qb[sl] = load_frag_row(qp, 0, 0, 32 * sl + 8 * g);
  }
  const ushort* kp = kc + b * geo.c_batch + hk * geo.c_head;
  const ushort* vp = vc + b * geo.c_batch + hk * geo.c_head;
  const float sc2 = geo.scale * LOG2E;

  // block-uniform walk bounds (blk * 64 < R by the grid)
  const int i_first = (blk * 64) / grp;
  const int i_last = min(blk * 64 + 63, R - 1) / grp;
  const int start = split * geo.chunk;
  const int end = min(start + geo.chunk, P + i_last + 1);   // may be <= start
  const int full_end =
      start + 32 * max(0, (min(end, P + i_first + 1) - start) / 32);
  // wave-uniform: nothing at or past this key is visible to the wave's rows
  const int wave_end = r0 < R ? P + min(r0 + 15, R - 1) / grp + 1 : 0;

  f32x4 acc[DTILES];
#pragma unroll
  for (int t = 0; t < DTILES; ++t) acc[t] = f32x4{0, 0, 0, 0};
  float m_run = -INFINITY, l_run = 0.f;   // of query n, in exp2 units

  s16x8 kr[DTILES / 4], vr[DTILES / 4];
  ext_load_tile<DTILES>(kr, vr, kp, vp, start, kvl, tid);   // clamped
  auto tile = [&](int kv0, auto masked) {
    __syncthreads();   // previous tile's LDS reads complete
    ext_store_tile<DTILES>(k_rm, v_t, kr, vr, tid);
    __syncthreads();
    // clamped: in bounds even past the last tile
    ext_load_tile<DTILES>(kr, vr, kp, vp, kv0 + 32, kvl, tid);
    if (kv0 >= wave_end) return;   // after the barriers
    f32x4 p0 = {0, 0, 0, 0}, p1 = {0, 0, 0, 0};
#pragma unroll
    for (int sl = 0; sl < KS; ++sl) {
      const int c0 = 32 * sl + 8 * g;
      p0 = mfma_bf16(load_frag_rm<DTILES>(k_rm, n, c0), qb[sl], p0);
      p1 = mfma_bf16(load_frag_rm<DTILES>(k_rm, 16 + n, c0), qb[sl], p1);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p0[r] *= sc2;
      p1[r] *= sc2;
      if constexpr (decltype(masked)::value) {
        const int k0a = kv0 + 4 * g + r;
        if (k0a > qlim) p0[r] = -INFINITY;
        if (k0a + 16 > qlim) p1[r] = -INFINITY;
      }
      mx = fmaxf(mx, fmaxf(p0[r], p1[r]));
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);   // -inf: the row saw no key yet
    const float alpha =
        (m_run == -INFINITY) ? 0.f : __builtin_exp2f(m_run - m_new);
    float pf[8];
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pf[r] = __builtin_exp2f(p0[r] - m_new);
      pf[4 + r] = __builtin_exp2f(p1[r] - m_new);
      if constexpr (decltype(masked)::value) {   // m_new may be -inf too
        if (p0[r] == -INFINITY) pf[r] = 0.f;
        if (p1[r] == -INFINITY) pf[4 + r] = 0.f;
      }
      psum += pf[r] + pf[4 + r];
    }
    psum += __shfl_xor(psum, 16);
    psum += __shfl_xor(psum, 32);
    l_run = l_run * alpha + psum;
    m_run = m_new;
    // slot 8g + j of the contraction = key 16*(j >> 2) + 4g + (j & 3)
    const bf16x8 pb = pack_bf16x8(pf);
#pragma unroll
    for (int t = 0; t < DTILES; ++t) {
      const ushort* vrow = v_t + (16 * t + n) * LDS_RP + 4 * g;
      const s16x4 lo = *reinterpret_cast<const s16x4*>(vrow);
      const s16x4 hi = *reinterpret_cast<const s16x4*>(vrow + 16);
      const bf16x8 va =
          as_bf16x8(__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      acc[t] *= alpha;
      acc[t] = mfma_bf16(va, pb, acc[t]);
    }
  };
  int kv0 = start;
  for (; kv0 < full_end; kv0 += 32) tile(kv0, std::false_type{});
  for (; kv0 < end; kv0 += 32) tile(kv0, std::true_type{});

  if (row >= R) return;   // padding rows; no barrier follows
  const int64_t orow = (int64_t(b) * geo.Sq + qi) * geo.H + h;
  if (geo.nsplit == 1) {
    const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
    ushort* op = o + orow * D + 4 * g;
#pragma unroll
    for (int t = 0; t < DTILES; ++t) {
      s16x4 ob;
#pragma unroll
      for (int e = 0; e < 4; ++e) ob[e] = short(f2bf(acc[t][e] * inv));
      *reinterpret_cast<s16x4*>(op + 16 * t) = ob;
    }
  } else {
    float* wrow = ws + (orow * geo.nsplit + split) * dta_decode_split_row(D);
#pragma unroll
    for (int t = 0; t < DTILES; ++t)
      *reinterpret_cast<f32x4*>(wrow + 16 * t + 4 * g) = acc[t];
    if (g == 0)
      *reinterpret_cast<f32x4*>(wrow + D) = f32x4{m_run, l_run, 0.f, 0.f};
  }
}

// ---------------- mfma layout probes ----------------
__global__ void mfma_probe16_k(const ushort* A, const ushort* B, float* D) {
  const int lane = threadIdx.x & 63;
  bf16x8 a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    union { ushort s; __bf16 v; } ca, cb;
    ca.s = A[(lane & 15) * 32 + 8 * (lane >> 4) + j];
    cb.s = B[(8 * (lane >> 4) + j) * 16 + (lane & 15)];
    a[j] = ca.v;
    b[j] = cb.v;
  }
  f32x4 c = {0, 0, 0, 0};
  c = mfma_bf16(a, b, c);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    D[(4 * (lane >> 4) + r) * 16 + (lane & 15)] = c[r];
}

__global__ void mfma_probe32_k(const ushort* A, const ushort* B, float* D) {
  const int lane = threadIdx.x & 63;
  bf16x8 a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    union { ushort s; __bf16 v; } ca, cb;
    ca.s = A[(lane & 31) * 16 + 8 * (lane >> 5) + j];
    cb.s = B[(8 * (lane >> 5) + j) * 32 + (lane & 31)];
    a[j] = ca.v;
    b[j] = cb.v;
  }
  f32x16 c = {};
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    D[row * 32 + (lane & 31)] = c[r];
  }
}

// ---- head-dim dispatch ------------------------------------------------------
// f(std::integral_constant<int, DTILES>) for hd = 16 * DTILES. The bindings
// reject other head dims before any launch. HD32: whether the kernel family
// is instantiated for head dim 32 (decode is not).
template <bool HD32 = true, class F>
void for_head_dim(int hd, F f) {
  if (hd == 64) f(std::integral_constant<int, 4>{});
  else if (hd == 128) f(std::integral_constant<int, 8>{});
  else if constexpr (HD32)
    if (hd == 32) f(std::integral_constant<int, 2>{});
}

// f(std::bool_constant<DOC>): the document-mask instantiation iff q_lo is set
template <class F>
void for_doc_mask(const AttnGeom& geo, F f) {
  if (geo.q_lo) f(std::true_type{});
  else f(std::false_type{});
}

dim3 attn_grid(const AttnGeom& geo) {
  return dim3((geo.seq + 63) / 64, int64_t(geo.B) * geo.H);
}

}  // namespace

void launch_attn_fwd(const bf16_t* q, const bf16_t* k, const bf16_t* v,
                     bf16_t* o, float* lse, const AttnGeom& geo,
                     hipStream_t s) {
  for_head_dim(geo.hd, [&](auto dt) {
    for_doc_mask(geo, [&](auto doc) {
      attn_fwd_k<dt(), doc()><<<attn_grid(geo), 256, 0, s>>>(q, k, v, o, lse,
                                                             geo);
    });
  });
}

void launch_attn_bwd_dq(const bf16_t* dout, const bf16_t* q, const bf16_t* k,
                        const bf16_t* v, const bf16_t* o, const float* lse,
                        float* delta, bf16_t* dq, const AttnGeom& geo,
                        hipStream_t s) {
  for_head_dim(geo.hd, [&](auto dt) {
    for_doc_mask(geo, [&](auto doc) {
      attn_bwd_dq_k<dt(), doc()><<<attn_grid(geo), 256, 0, s>>>(
          dout, q, k, v, o, lse, delta, dq, geo);
    });
  });
}

void launch_attn_bwd_dkv(const bf16_t* dout, const bf16_t* q,
                         const bf16_t* k, const bf16_t* v, const float* lse,
                         const float* delta, float* dk32, float* dv32,
                         bf16_t* dk, bf16_t* dv, const AttnGeom& geo,
                         hipStream_t s) {
  for_head_dim(geo.hd, [&](auto dt) {
    // GQA folds heads via fp32 atomics; grp==1 stores bf16 directly
    for_doc_mask(geo, [&](auto doc) {
      auto kern = geo.grp > 1 ? attn_bwd_dkv_k<dt(), true, doc()>
                              : attn_bwd_dkv_k<dt(), false, doc()>;
      kern<<<attn_grid(geo), 256, 0, s>>>(dout, q, k, v, lse, delta, dk32,
                                          dv32, dk, dv, geo);
    });
  });
}

void launch_attn_bwd_dkv_gqa(const bf16_t* dout, const bf16_t* q,
                             const bf16_t* k, const bf16_t* v,
                             const float* lse, const float* delta,
                             bf16_t* dk, bf16_t* dv, const AttnGeom& geo,
                             hipStream_t s) {
  // dta_attn_bwd_gqa_shape(geo) holds; one block per (key tile, b, kv head)
  const dim3 grid((geo.seq + 63) / 64, int64_t(geo.B) * (geo.H / geo.grp));
  for_head_dim(geo.hd, [&](auto dt) {
    for_doc_mask(geo, [&](auto doc) {
      attn_bwd_dkv_gqa_k<dt(), doc()><<<grid, 256, 0, s>>>(
          dout, q, k, v, lse, delta, dk, dv, geo);
    });
  });
}

void launch_attn_bwd_fused(const bf16_t* dout, const bf16_t* q,
                           const bf16_t* k, const bf16_t* v, const bf16_t* o,
                           const float* lse, bf16_t* dq, bf16_t* dk,
                           bf16_t* dv, const AttnGeom& geo, hipStream_t s) {
  // dta_attn_bwd_fused_shape(geo) holds: one 64-row tile, hd 32 or 64
  const dim3 grid(1, int64_t(geo.B) * geo.H);
  for_doc_mask(geo, [&](auto doc) {
    if (geo.hd == 64)
      attn_bwd_fused_k<4, doc()><<<grid, 256, 0, s>>>(dout, q, k, v, o, lse,
                                                      dq, dk, dv, geo);
    else
      attn_bwd_fused_k<2, doc()><<<grid, 256, 0, s>>>(dout, q, k, v, o, lse,
                                                      dq, dk, dv, geo);
  });
}

void launch_mfma_probe_16(const bf16_t* A, const bf16_t* B, float* D,
                          hipStream_t s) {
  mfma_probe16_k<<<1, 64, 0, s>>>(A, B, D);
}
void launch_mfma_probe_32(const bf16_t* A, const bf16_t* B, float* D,
                          hipStream_t s) {
  mfma_probe32_k<<<1, 64, 0, s>>>(A, B, D);
}

void launch_attn_decode(const bf16_t* q, const bf16_t* kc, const bf16_t* vc,
                        bf16_t* o, int B, int H, int grp, int kvlen,
                        const int* len_p, int hd, int64_t cb, int64_t ch,
                        float scale, hipStream_t s) {
  // block per (b, h); 4 waves split the cache
  for_head_dim<false>(hd, [&](auto dt) {
    attn_decode_k<dt()><<<B * H, 256, 0, s>>>(q, kc, vc, o, B, H, grp, kvlen,
                                              len_p, cb, ch, scale);
  });
}

void launch_attn_decode_split(const bf16_t* q, const bf16_t* kc,
                              const bf16_t* vc, bf16_t* o, float* ws, int B,
                              int H, int grp, int Lmax, int kvlen,
                              const int* len_p, int hd, int64_t cb, int64_t ch,
                              float scale, int nsplit, hipStream_t s) {
  const dim3 grid(nsplit, H / grp, B);
  const int chunk = dta_decode_split_chunk(Lmax, nsplit);
  for_head_dim<false>(hd, [&](auto dt) {
    attn_decode_split_k<dt()><<<grid, 256, 0, s>>>(
        q, kc, vc, o, ws, H, grp, Lmax, kvlen, len_p, cb, ch, chunk, scale);
    if (nsplit > 1)
      attn_decode_combine_k<dt()><<<(B * H + 3) / 4, 256, 0, s>>>(ws, o, B * H,
                                                                  nsplit);
  });
}

void launch_attn_extend(const bf16_t* q, const bf16_t* kc, const bf16_t* vc,
                        bf16_t* o, float* ws, ExtGeom geo, hipStream_t s) {
  const int rows = geo.Sq * geo.grp;
  const dim3 grid(((rows + 63) / 64) * geo.nsplit, geo.H / geo.grp, geo.B);
  geo.chunk = dta_extend_chunk(geo.P + geo.Sq, geo.nsplit);
  const int BH = geo.B * geo.Sq * geo.H;
  for_head_dim<false>(geo.hd, [&](auto dt) {
    attn_extend_k<dt()><<<grid, 256, 0, s>>>(q, kc, vc, o, ws, geo);
    if (geo.nsplit > 1)
      attn_decode_combine_k<dt()><<<(BH + 3) / 4, 256, 0, s>>>(ws, o, BH,
                                                               geo.nsplit);
  });
}

void launch_attn_decode_split_q8(const bf16_t* q, const signed char* kc,
                                 const signed char* vc, const float* k_scale,
                                 const float* v_scale, bf16_t* o, float* ws,
                                 int B, int H, int grp, int Lmax, int Lp,
                                 int kvlen, const int* len_p, int hd,
                                 float scale, int nsplit, hipStream_t s) {
  const dim3 grid(nsplit, H / grp, B);
  const int chunk = dta_decode_split_chunk(Lmax, nsplit);
  for_head_dim<false>(hd, [&](auto dt) {
    attn_decode_split_q8_k<dt()><<<grid, 256, 0, s>>>(
        q, reinterpret_cast<const char*>(kc),
        reinterpret_cast<const char*>(vc), k_scale, v_scale, o, ws, H, grp,
        Lmax, Lp, kvlen, len_p, chunk, scale);
    if (nsplit > 1)
      attn_decode_combine_k<dt()><<<(B * H + 3) / 4, 256, 0, s>>>(ws, o, B * H,
                                                                  nsplit);
  });
}
