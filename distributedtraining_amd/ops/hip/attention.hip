// Fused causal flash attention, forward + backward, MFMA
// (mfma_f32_16x16x32_bf16) with online softmax — the CDNA4 replacement for
// the reference's transformers attention (SURVEY.md §2.2 op table; miner
// seq 64, validator seq 512).
//
// Structure (v2):
//   * one 64-lane wave owns a 16-row Q tile; blocks of 4 independent waves
//     (no __syncthreads in the loop), grid = (ceil(S/64), B*H).
//   * STRIDE-AWARE addressing: q/k/v/o are consumed as [B,H,S,D] *views*
//     of the projection output [B,S,H*D] (and dq/dk/dv written the same
//     way) so the model layer does zero transpose/contiguous copies.
//   * GQA native: kv head = h / group; no repeat_interleave materialization.
//   * row fragments stream from global (K/V fit in L2 at these seq
//     lengths); k-major B-fragments are NOT gathered from global (8 scalar
//     2B loads each, ~32x line waste) — row frags are scatter-stored
//     transposed into wave-private LDS and re-read as 16B vectors.
//   * swapped QK^T: mfma(A=K_tile, B=Q^T) puts a query's scores in lanes
//     sharing (lane&15) so the softmax row-reduce is two shfl_xor ops;
//     exp via the single-instruction exp2 path.
//
// Fragment maps (verified on-device by mfma_selftest, tests/test_ops_gpu.py):
//   mfma_f32_16x16x32_bf16: A[i][k]: i=lane&15, k=8*(lane>>4)+j (j=0..7)
//                           B[k][n]: n=lane&15, k=8*(lane>>4)+j
//                           C/D[i][j]: col=lane&15, row=4*(lane>>4)+reg
#include "dta_common.h"
#include "dta_kernels.h"

namespace {

DEV f32x4 mfma_bf16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

DEV bf16x8 load_frag_row(const ushort* base, int64_t row_stride, int row,
                         int col0) {
  const s16x8 v =
      *reinterpret_cast<const s16x8*>(base + int64_t(row) * row_stride + col0);
  union { s16x8 s; bf16x8 b; } u;
  u.s = v;
  return u.b;
}

// ---- LDS tile staging ------------------------------------------------------
// B-fragments (k-major columns) gathered straight from global memory cost 8
// scalar 2 B loads each, every one touching its own 64 B line (~32x wasted
// HBM traffic — measured 204 us on the dkv kernel). Tiles are staged
// block-cooperatively (the 4 waves share one (b,h)'s K/V or Q/dO) as
// row-major panels for A-fragments and transposed [cols][LDS_RP] panels
// for B-fragments (single 16 B LDS reads). Rows beyond seq hold clamped
// garbage — safe everywhere because the matching score/probability lanes
// are already masked to 0 upstream.
constexpr int LDS_RP = 40;  // 32 rows + 8 pad (multiple of 8: aligned reads)

DEV bf16x8 load_frag_col_lds(const ushort* lds_t, int row0, int col) {
  const s16x8 v =
      *reinterpret_cast<const s16x8*>(lds_t + col * LDS_RP + row0);
  union { s16x8 s; bf16x8 b; } u;
  u.s = v;
  return u.b;
}

// ---- block-cooperative tile staging ---------------------------------------
// The 4 waves of a block share one (b,h)'s K/V (fwd, dq) or Q/dO (dkv)
// tiles; loading them per wave re-read ~590 MB/step from L2/HBM at the
// flagship shape. All 256 threads cooperatively stage the 32-row tile
// once per iteration (row-major for A-fragments, transposed for
// B-fragments); rows past seq are clamped (masked upstream).
// Row-major pitch: D+8 (2-way max bank conflict on 16-row A reads).
template <int DTILES>
DEV void stage_tile_rm(ushort* lds_rm, const ushort* src, int64_t rstride,
                       int row0, int seq, int tid) {
  constexpr int CPR = 2 * DTILES;       // 16B chunks per row (D/8)
  constexpr int RP = 16 * DTILES + 8;
  for (int i = tid; i < 32 * CPR; i += 256) {
    const int r = i / CPR, c8 = (i % CPR) * 8;
    const int rr = row0 + r;
    const s16x8 v = *reinterpret_cast<const s16x8*>(
        src + int64_t(rr < seq ? rr : seq - 1) * rstride + c8);
    *reinterpret_cast<s16x8*>(lds_rm + r * RP + c8) = v;
  }
}

template <int DTILES>
DEV void stage_tile_T2(ushort* lds_t, const ushort* src, int64_t rstride,
                       int row0, int seq, int tid) {
  constexpr int CPR = 2 * DTILES;
  for (int i = tid; i < 32 * CPR; i += 256) {
    const int r = i / CPR, c8 = (i % CPR) * 8;
    const int rr = row0 + r;
    const s16x8 v = *reinterpret_cast<const s16x8*>(
        src + int64_t(rr < seq ? rr : seq - 1) * rstride + c8);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      lds_t[(c8 + j) * LDS_RP + r] = ushort(v[j]);
  }
}

template <int DTILES>
DEV bf16x8 load_frag_rm(const ushort* lds_rm, int row_rel, int c0) {
  constexpr int RP = 16 * DTILES + 8;
  const s16x8 v =
      *reinterpret_cast<const s16x8*>(lds_rm + row_rel * RP + c0);
  union { s16x8 s; bf16x8 b; } u;
  u.s = v;
  return u.b;
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

// ---------------- forward ----------------
// Block = 4 waves = 64 q rows of one (b,h); K/V tiles staged ONCE per
// block per 32-key iteration (cooperative, barrier-synchronized — every
// thread reaches both __syncthreads regardless of seq masking).
template <int DTILES>  // D = 16*DTILES
__global__ void attn_fwd_k(const ushort* __restrict__ q,
                           const ushort* __restrict__ k,
                           const ushort* __restrict__ v,
                           ushort* __restrict__ o, float* __restrict__ lse,
                           AttnGeom geo) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int64_t bhid = blockIdx.y;
  const int b = int(bhid) / geo.H, h = int(bhid) % geo.H;
  const int hk = h / geo.grp;
  const int seq = geo.seq;
  const int q0 = blockIdx.x * 64 + wid * 16;
  const bool live = q0 < seq;
  const ushort* qp = q + b * geo.qb + h * geo.qh;
  const ushort* kp = k + b * geo.kb + hk * geo.kh;
  const ushort* vp = v + b * geo.vb + hk * geo.vh;
  const float sc2 = geo.scale * LOG2E;  // fold scale into the exp2 argument
  // padded batches: keys >= kvl are masked for every query (block-uniform)
  const int kvl = geo.kvlen ? min(seq, geo.kvlen[b]) : seq;
  const uint32_t thr = geo.drop.thr16;
  uint64_t drop_s2 = 0;
  if (thr)
    drop_s2 = rng_head_seed(rng_site_seed(geo.drop.rng, geo.drop.site),
                            uint64_t(bhid));

  bf16x8 qb_[DTILES / 2];
  const int qrow = q0 + (lane & 15);
  const int qr_ld = qrow < seq ? qrow : seq - 1;
#pragma unroll
  for (int sl = 0; sl < DTILES / 2; ++sl)
    qb_[sl] = load_frag_row(qp, geo.qs, qr_ld, 32 * sl + 8 * (lane >> 4));

  f32x4 acc[DTILES];
#pragma unroll
  for (int t = 0; t < DTILES; ++t) acc[t] = f32x4{0, 0, 0, 0};
  float m_run = -INFINITY, l_run = 0.f;  // in exp2 units

  __shared__ ushort k_rm[32 * (16 * DTILES + 8)];
  __shared__ ushort v_t[16 * DTILES * LDS_RP];
  const int g = lane >> 4;
  // loop + mask bounds honor the pad length (kvl == seq when unmasked)
  const int blk_kv_end =
      min(min(seq, int(blockIdx.x) * 64 + 64), (kvl + 31) & ~31);  // uniform
  const int my_kv_end = live ? min(seq, q0 + 16) : 0;
  for (int kv0 = 0; kv0 < blk_kv_end; kv0 += 32) {
    __syncthreads();   // previous iteration's LDS reads complete
    stage_tile_rm<DTILES>(k_rm, kp, geo.ks, kv0, seq, tid);
    stage_tile_T2<DTILES>(v_t, vp, geo.vs, kv0, seq, tid);
    __syncthreads();
    if (kv0 >= my_kv_end) continue;   // after barriers: uniform safety
    f32x4 p0 = {0, 0, 0, 0}, p1 = {0, 0, 0, 0};
#pragma unroll
    for (int sl = 0; sl < DTILES / 2; ++sl) {
      const int c0 = 32 * sl + 8 * (lane >> 4);
      bf16x8 ka = load_frag_rm<DTILES>(k_rm, lane & 15, c0);
      p0 = mfma_bf16(ka, qb_[sl], p0);
      bf16x8 kb2 = load_frag_rm<DTILES>(k_rm, 16 + (lane & 15), c0);
      p1 = mfma_bf16(kb2, qb_[sl], p1);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k0a = kv0 + 4 * g + r, k1a = k0a + 16;
      p0[r] = (k0a <= qrow && k0a < kvl) ? p0[r] * sc2 : -INFINITY;
      p1[r] = (k1a <= qrow && k1a < kvl) ? p1[r] * sc2 : -INFINITY;
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

    if (thr) {
      // dropout on the PV accumulation only: l keeps the undropped sum,
      // so O = dropout(P) V with P the true softmax. One hash covers the
      // 4 consecutive keys this lane holds per half (k & 3 == r).
      const uint64_t hq = rng_attn_row(drop_s2, uint32_t(qrow));
      const uint64_t h0 =
          rng_attn_row_hash(hq, uint32_t((kv0 + 4 * g) >> 2));
      const uint64_t h1 =
          rng_attn_row_hash(hq, uint32_t((kv0 + 16 + 4 * g) >> 2));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p0[r] = rng_keep(h0, r, thr) ? p0[r] * geo.drop.inv_keep : 0.f;
        p1[r] = rng_keep(h1, r, thr) ? p1[r] * geo.drop.inv_keep : 0.f;
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
    lse[bhid * seq + qrow] = (m_run + __builtin_log2f(l_run)) * LN2;
  float inv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float lr = __shfl(l_run, 4 * g + r);
    inv[r] = lr > 0.f ? 1.0f / lr : 0.f;
  }
  ushort* op = o + b * geo.ob + h * geo.oh;
#pragma unroll
  for (int t = 0; t < DTILES; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = q0 + 4 * g + r;
      if (orow < seq)
        op[int64_t(orow) * geo.os_ + 16 * t + (lane & 15)] =
            f2bf(acc[t][r] * inv[r]);
    }
}

// ---------------- backward dQ ----------------
// Same cooperative structure as forward: K (row-major + transposed) and V
// (row-major) staged once per block per 32-key iteration.
// Also COMPUTES delta[q] = rowsum(dO[q]*O[q]) from its own rows (it loads
// dO anyway; O rows are one extra coalesced read) and publishes it for the
// dkv kernel — the standalone delta kernel is gone.
template <int DTILES>
__global__ void attn_bwd_dq_k(const ushort* __restrict__ dout,
                              const ushort* __restrict__ q,
                              const ushort* __restrict__ k,
                              const ushort* __restrict__ v,
                              const ushort* __restrict__ o,
                              int64_t ob2, int64_t oh2, int64_t os2,
                              const float* __restrict__ lse,
                              float* __restrict__ delta,
                              ushort* __restrict__ dq, AttnGeom geo) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int64_t bhid = blockIdx.y;
  const int b = int(bhid) / geo.H, h = int(bhid) % geo.H;
  const int hk = h / geo.grp;
  const int seq = geo.seq;
  const int q0 = blockIdx.x * 64 + wid * 16;
  const bool live = q0 < seq;
  const ushort* qp = q + b * geo.qb + h * geo.qh;
  const ushort* kp = k + b * geo.kb + hk * geo.kh;
  const ushort* vp = v + b * geo.vb + hk * geo.vh;
  const ushort* dop = dout + b * geo.db_ + h * geo.dh;
  const ushort* op2 = o + b * ob2 + h * oh2;
  const int kvl = geo.kvlen ? min(seq, geo.kvlen[b]) : seq;
  const uint32_t thr = geo.drop.thr16;
  uint64_t drop_s2 = 0;
  if (thr)
    drop_s2 = rng_head_seed(rng_site_seed(geo.drop.rng, geo.drop.site),
                            uint64_t(bhid));

  const int qrow = q0 + (lane & 15);
  const int qr_ld = qrow < seq ? qrow : seq - 1;
  bf16x8 qb_[DTILES / 2], dob[DTILES / 2];
  float dpart = 0.f;
#pragma unroll
  for (int sl = 0; sl < DTILES / 2; ++sl) {
    const int c0 = 32 * sl + 8 * (lane >> 4);
    qb_[sl] = load_frag_row(qp, geo.qs, qr_ld, c0);
    dob[sl] = load_frag_row(dop, geo.ds, qr_ld, c0);
    bf16x8 orow = load_frag_row(op2, os2, qr_ld, c0);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      dpart = fmaf(float(dob[sl][j]), float(orow[j]), dpart);
  }
  // delta[qrow]: each of the 4 lane-groups holds 16 of the 64 columns of
  // row (lane&15); fold across groups
  dpart += __shfl_xor(dpart, 16);
  dpart += __shfl_xor(dpart, 32);
  const float dlt_q = dpart;
  if (lane < 16 && qrow < seq) delta[bhid * seq + qrow] = dlt_q;
  const float lse_q = lse[bhid * seq + qr_ld] * LOG2E;  // exp2 units
  const float sc2 = geo.scale * LOG2E;

  f32x4 acc[DTILES];
#pragma unroll
  for (int t = 0; t < DTILES; ++t) acc[t] = f32x4{0, 0, 0, 0};

  __shared__ ushort k_rm[32 * (16 * DTILES + 8)];
  __shared__ ushort v_rm[32 * (16 * DTILES + 8)];
  __shared__ ushort k_t[16 * DTILES * LDS_RP];
  const int g = lane >> 4;
  const int blk_kv_end =
      min(min(seq, int(blockIdx.x) * 64 + 64), (kvl + 31) & ~31);  // uniform
  const int my_kv_end = live ? min(seq, q0 + 16) : 0;
  for (int kv0 = 0; kv0 < blk_kv_end; kv0 += 32) {
    __syncthreads();
    stage_tile_rm<DTILES>(k_rm, kp, geo.ks, kv0, seq, tid);
    stage_tile_rm<DTILES>(v_rm, vp, geo.vs, kv0, seq, tid);
    stage_tile_T2<DTILES>(k_t, kp, geo.ks, kv0, seq, tid);
    __syncthreads();
    if (kv0 >= my_kv_end) continue;
    f32x4 s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
    f32x4 dp0 = {0, 0, 0, 0}, dp1 = {0, 0, 0, 0};
#pragma unroll
    for (int sl = 0; sl < DTILES / 2; ++sl) {
      const int c0 = 32 * sl + 8 * (lane >> 4);
      bf16x8 ka = load_frag_rm<DTILES>(k_rm, lane & 15, c0);
      bf16x8 kb2 = load_frag_rm<DTILES>(k_rm, 16 + (lane & 15), c0);
      bf16x8 va = load_frag_rm<DTILES>(v_rm, lane & 15, c0);
      bf16x8 vb2 = load_frag_rm<DTILES>(v_rm, 16 + (lane & 15), c0);
      s0 = mfma_bf16(ka, qb_[sl], s0);
      s1 = mfma_bf16(kb2, qb_[sl], s1);
      dp0 = mfma_bf16(va, dob[sl], dp0);
      dp1 = mfma_bf16(vb2, dob[sl], dp1);
    }
    uint64_t h0 = 0, h1 = 0;
    if (thr) {
      const uint64_t hq = rng_attn_row(drop_s2, uint32_t(qrow));
      h0 = rng_attn_row_hash(hq, uint32_t((kv0 + 4 * g) >> 2));
      h1 = rng_attn_row_hash(hq, uint32_t((kv0 + 16 + 4 * g) >> 2));
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k0a = kv0 + 4 * g + r, k1a = k0a + 16;
      const bool v0 = (k0a <= qrow && k0a < kvl);
      const bool v1 = (k1a <= qrow && k1a < kvl);
      const float P0 = v0 ? __builtin_exp2f(s0[r] * sc2 - lse_q) : 0.f;
      const float P1 = v1 ? __builtin_exp2f(s1[r] * sc2 - lse_q) : 0.f;
      // dS = P ⊙ (M/(1-p) ⊙ (dO Vᵀ) − delta): the dropout mask gates the
      // dO·V term only; delta = rowsum(dO ⊙ O) already absorbs the mask
      float g0 = dp0[r], g1 = dp1[r];
      if (thr) {
        g0 = rng_keep(h0, r, thr) ? g0 * geo.drop.inv_keep : 0.f;
        g1 = rng_keep(h1, r, thr) ? g1 * geo.drop.inv_keep : 0.f;
      }
      s0[r] = P0 * (g0 - dlt_q);
      s1[r] = P1 * (g1 - dlt_q);
    }
    bf16x8 dsa = scores_to_afrag(s0, s1, lane);
#pragma unroll
    for (int t = 0; t < DTILES; ++t) {
      bf16x8 kcb = load_frag_col_lds(k_t, 8 * g, 16 * t + (lane & 15));
      acc[t] = mfma_bf16(dsa, kcb, acc[t]);
    }
  }
  if (!live) return;
  ushort* dqp = dq + b * geo.ob + h * geo.oh;  // dq uses o-geometry strides
#pragma unroll
  for (int t = 0; t < DTILES; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = q0 + 4 * g + r;
      if (orow < seq)
        dqp[int64_t(orow) * geo.os_ + 16 * t + (lane & 15)] =
            f2bf(acc[t][r] * geo.scale);
    }
}

// ---------------- backward dK/dV ----------------
// Block = 4 waves = 64 KV rows of one (b,h); Q/dO tiles staged once per
// block per 32-query iteration (row-major for the score mfmas, transposed
// for the accumulation B-fragments). With GQA (grp>1) each kv head is
// walked once per ATTACHED q head (blockIdx.y covers B*H) and results are
// accumulated with fp32 atomics into dk/dv. Early waves see a few
// below-diagonal query tiles (probabilities masked to 0) — the price of a
// uniform, barrier-safe loop.
template <int DTILES, bool ATOMIC>
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
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int64_t bhid = blockIdx.y;
  const int b = int(bhid) / geo.H, h = int(bhid) % geo.H;
  const int hk = h / geo.grp;
  const int seq = geo.seq;
  const int kv0 = blockIdx.x * 64 + wid * 16;
  const bool live = kv0 < seq;
  const ushort* qp = q + b * geo.qb + h * geo.qh;
  const ushort* kp = k + b * geo.kb + hk * geo.kh;
  const ushort* vp = v + b * geo.vb + hk * geo.vh;
  const ushort* dop = dout + b * geo.db_ + h * geo.dh;
  const float sc2 = geo.scale * LOG2E;
  const int kvl = geo.kvlen ? min(seq, geo.kvlen[b]) : seq;
  const uint32_t thr = geo.drop.thr16;
  uint64_t drop_s2 = 0;
  if (thr)
    drop_s2 = rng_head_seed(rng_site_seed(geo.drop.rng, geo.drop.site),
                            uint64_t(bhid));

  const int krow = kv0 + (lane & 15);
  const int kr_ld = krow < seq ? krow : seq - 1;
  bf16x8 kb_[DTILES / 2], vbf[DTILES / 2];
#pragma unroll
  for (int sl = 0; sl < DTILES / 2; ++sl) {
    kb_[sl] = load_frag_row(kp, geo.ks, kr_ld, 32 * sl + 8 * (lane >> 4));
    vbf[sl] = load_frag_row(vp, geo.vs, kr_ld, 32 * sl + 8 * (lane >> 4));
  }

  f32x4 acck[DTILES], accv[DTILES];
#pragma unroll
  for (int t = 0; t < DTILES; ++t) {
    acck[t] = f32x4{0, 0, 0, 0};
    accv[t] = f32x4{0, 0, 0, 0};
  }

  __shared__ ushort q_rm[32 * (16 * DTILES + 8)];
  __shared__ ushort d_rm[32 * (16 * DTILES + 8)];
  __shared__ ushort q_t[16 * DTILES * LDS_RP];
  __shared__ ushort d_t[16 * DTILES * LDS_RP];
  const int g = lane >> 4;
  // a block whose 64 key rows are all padding has zero dk/dv: skip the
  // whole walk (uniform) and fall through to the zero-initialized stores
  const int q_start =
      (int(blockIdx.x) * 64 >= kvl) ? seq : int(blockIdx.x) * 64;
  const bool kv_ok = krow < kvl;
  for (int q0 = q_start; q0 < seq; q0 += 32) {
    __syncthreads();
    stage_tile_rm<DTILES>(q_rm, qp, geo.qs, q0, seq, tid);
    stage_tile_rm<DTILES>(d_rm, dop, geo.ds, q0, seq, tid);
    stage_tile_T2<DTILES>(q_t, qp, geo.qs, q0, seq, tid);
    stage_tile_T2<DTILES>(d_t, dop, geo.ds, q0, seq, tid);
    __syncthreads();
    if (!live || q0 + 31 < kv0) continue;   // fully below the diagonal
    f32x4 s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
    f32x4 dp0 = {0, 0, 0, 0}, dp1 = {0, 0, 0, 0};
#pragma unroll
    for (int sl = 0; sl < DTILES / 2; ++sl) {
      const int c0 = 32 * sl + 8 * (lane >> 4);
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
      const int qa0 = q0 + 4 * g + r, qa1 = qa0 + 16;
      const bool v0 = (qa0 >= krow && qa0 < seq && kv_ok);
      const bool v1 = (qa1 >= krow && qa1 < seq && kv_ok);
      const float l0 = lse[bhid * seq + (v0 ? qa0 : 0)] * LOG2E;
      const float l1 = lse[bhid * seq + (v1 ? qa1 : 0)] * LOG2E;
      p0[r] = v0 ? __builtin_exp2f(s0[r] * sc2 - l0) : 0.f;
      p1[r] = v1 ? __builtin_exp2f(s1[r] * sc2 - l1) : 0.f;
      const float d0 = delta[bhid * seq + ((qa0 < seq) ? qa0 : 0)];
      const float d1 = delta[bhid * seq + ((qa1 < seq) ? qa1 : 0)];
      if (thr) {
        // element (q, k=krow): slice krow&3 of hash(q, krow>>2) — the
        // transposed view of the SAME per-(b,h,q,k) draw the fwd/dq
        // kernels take; dV uses the dropped P, dK the dropout-gated dS
        const uint64_t hk0 =
            rng_attn_hash(drop_s2, uint32_t(qa0), uint32_t(krow) >> 2);
        const uint64_t hk1 =
            rng_attn_hash(drop_s2, uint32_t(qa1), uint32_t(krow) >> 2);
        const float m0 =
            rng_keep(hk0, krow & 3, thr) ? geo.drop.inv_keep : 0.f;
        const float m1 =
            rng_keep(hk1, krow & 3, thr) ? geo.drop.inv_keep : 0.f;
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
  constexpr int D = 16 * DTILES;
#pragma unroll
  for (int t = 0; t < DTILES; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = kv0 + 4 * g + r;
      if (orow >= seq) continue;
      const int col = 16 * t + (lane & 15);
      if (ATOMIC) {
        // fp32 accumulation across the grp q-heads sharing this kv head
        int64_t off = ((int64_t(b) * (geo.H / geo.grp) + hk) * seq + orow) * D + col;
        atomicAdd(dk32 + off, acck[t][r] * geo.scale);
        atomicAdd(dv32 + off, accv[t][r]);
      } else {
        ushort* dkp = dk + b * geo.gkb + hk * geo.gkh;
        ushort* dvp = dv + b * geo.gkb + hk * geo.gkh;
        dkp[int64_t(orow) * geo.gks + col] = f2bf(acck[t][r] * geo.scale);
        dvp[int64_t(orow) * geo.gks + col] = f2bf(accv[t][r]);
      }
    }
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
  typedef __attribute__((ext_vector_type(16))) float f32x16_t;
  bf16x8 a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    union { ushort s; __bf16 v; } ca, cb;
    ca.s = A[(lane & 31) * 16 + 8 * (lane >> 5) + j];
    cb.s = B[(8 * (lane >> 5) + j) * 32 + (lane & 31)];
    a[j] = ca.v;
    b[j] = cb.v;
  }
  f32x16_t c = {};
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    D[row * 32 + (lane & 31)] = c[r];
  }
}

}  // namespace

void launch_attn_fwd(const bf16_t* q, const bf16_t* k, const bf16_t* v,
                     bf16_t* o, float* lse, const AttnGeom& geo,
                     hipStream_t s) {
  dim3 grid((geo.seq + 63) / 64, int64_t(geo.B) * geo.H);
  const int hd = geo.hd;
  if (hd == 64) attn_fwd_k<4><<<grid, 256, 0, s>>>(q, k, v, o, lse, geo);
  else if (hd == 128) attn_fwd_k<8><<<grid, 256, 0, s>>>(q, k, v, o, lse, geo);
  else if (hd == 32) attn_fwd_k<2><<<grid, 256, 0, s>>>(q, k, v, o, lse, geo);
}

void launch_attn_bwd_dq(const bf16_t* dout, const bf16_t* q, const bf16_t* k,
                        const bf16_t* v, const bf16_t* o, int64_t ob2,
                        int64_t oh2, int64_t os2, const float* lse,
                        float* delta, bf16_t* dq, const AttnGeom& geo,
                        hipStream_t s) {
  dim3 grid((geo.seq + 63) / 64, int64_t(geo.B) * geo.H);
  const int hd = geo.hd;
  if (hd == 64) attn_bwd_dq_k<4><<<grid, 256, 0, s>>>(dout, q, k, v, o, ob2, oh2, os2, lse, delta, dq, geo);
  else if (hd == 128) attn_bwd_dq_k<8><<<grid, 256, 0, s>>>(dout, q, k, v, o, ob2, oh2, os2, lse, delta, dq, geo);
  else if (hd == 32) attn_bwd_dq_k<2><<<grid, 256, 0, s>>>(dout, q, k, v, o, ob2, oh2, os2, lse, delta, dq, geo);
}

void launch_attn_bwd_dkv(const bf16_t* dout, const bf16_t* q,
                         const bf16_t* k, const bf16_t* v, const float* lse,
                         const float* delta, float* dk32, float* dv32,
                         bf16_t* dk, bf16_t* dv, const AttnGeom& geo,
                         hipStream_t s) {
  dim3 grid((geo.seq + 63) / 64, int64_t(geo.B) * geo.H);
  const int hd = geo.hd;
  const bool at = geo.grp > 1;  // GQA folds heads via fp32 atomics;
                                // grp==1 stores bf16 directly
#define DKV(D_)                                                              \
  do {                                                                       \
    if (at)                                                                  \
      attn_bwd_dkv_k<D_, true><<<grid, 256, 0, s>>>(dout, q, k, v, lse,      \
                                                    delta, dk32, dv32, dk,   \
                                                    dv, geo);                \
    else                                                                     \
      attn_bwd_dkv_k<D_, false><<<grid, 256, 0, s>>>(dout, q, k, v, lse,     \
                                                     delta, dk32, dv32, dk,  \
                                                     dv, geo);               \
  } while (0)
  if (hd == 64) DKV(4);
  else if (hd == 128) DKV(8);
  else if (hd == 32) DKV(2);
#undef DKV
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
  const int grid = B * H;   // block per (b, h); 4 waves split the cache
  if (hd == 64)
    attn_decode_k<4><<<grid, 256, 0, s>>>(q, kc, vc, o, B, H, grp, kvlen,
                                          len_p, cb, ch, scale);
  else if (hd == 128)
    attn_decode_k<8><<<grid, 256, 0, s>>>(q, kc, vc, o, B, H, grp, kvlen,
                                          len_p, cb, ch, scale);
}
