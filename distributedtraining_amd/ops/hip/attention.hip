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

// dout may be null (forward); its strides are then 0.
DEV AttnCtx attn_ctx(const AttnGeom& geo, const ushort* q, const ushort* k,
                     const ushort* v, const ushort* dout) {
  AttnCtx c;
  c.tid = threadIdx.x;
  c.lane = c.tid & 63;
  c.wid = c.tid >> 6;
  c.g = c.lane >> 4;
  c.bhid = blockIdx.y;
  c.b = int(c.bhid) / geo.H;
  c.h = int(c.bhid) % geo.H;
  c.hk = c.h / geo.grp;
  c.q = q + c.b * geo.q.batch + c.h * geo.q.head;
  c.k = k + c.b * geo.k.batch + c.hk * geo.k.head;
  c.v = v + c.b * geo.v.batch + c.hk * geo.v.head;
  c.dout = dout + c.b * geo.dout.batch + c.h * geo.dout.head;
  c.sc2 = geo.scale * LOG2E;
  c.kvl = geo.kvlen ? min(geo.seq, geo.kvlen[c.b]) : geo.seq;
  c.q_lo = geo.q_lo ? geo.q_lo + int64_t(c.b) * geo.seq : nullptr;
  c.k_hi = geo.k_hi ? geo.k_hi + int64_t(c.b) * geo.seq : nullptr;
  c.thr = geo.drop.thr16;
  c.drop_s2 = 0;
  if (c.thr)
    c.drop_s2 = rng_head_seed(rng_site_seed(geo.drop.rng, geo.drop.site),
                              uint64_t(c.bhid));
  return c;
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
// Q/dO tiles staged once per block per 32-query iteration (row-major for
// the score mfmas, transposed for the accumulation B-fragments). With GQA
// (grp>1) each kv head is walked once per ATTACHED q head (blockIdx.y
// covers B*H) and results are accumulated with fp32 atomics into dk/dv.
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
