// Fused log-softmax + cross-entropy over the vocab dimension, fwd + bwd.
// This is the dominant memory cost of GPT-2-small training (logits are
// [tokens, 50257] bf16). Replaces the reference's transformers-internal CE
// (`labels=` path, training_manager.py:380-385).
//
// fwd: one block per row, ONE online pass: per s16x8 vector take the local
//      max (cheap fmax tree), then one branch-free accumulator rescale
//      s = s*exp2(m_old−m_new) + Σ exp2(x_j−m_new) — 9 exp2 per 8 elements.
//      (A per-ELEMENT rescale branch measured 3x slower than two-pass; the
//      per-VECTOR unconditional rescale beats both: single HBM pass.)
// bwd: dlogits = scale_row * (softmax - onehot), one streaming pass.
// fwd+bwd (training, logits given up): both passes by one block per row,
//      in place. Two variants, measured at [64512, 50257] on device events
//      (profiles/r04_fused_backward.md), against 4.46 ms for the pair:
//      * second sweep from cache, 256 threads, rows in flight capped
//        (ce_fwd_bwd_k): 3.47 ms at 1335 rows in flight, half the 256 MiB
//        Infinity Cache (512 / 1024 / 2048 / 4096: 4.25 / 3.51 / 3.64 /
//        3.58 ms). Same per-thread streams as ce_fwd_k: lse and dlogits
//        bit-identical to the pair. THE DEFAULT.
//      * row held in LDS, 1024 threads, one block per CU
//        (ce_fwd_bwd_lds_k): 3.09 ms, and about 0.3 ms/step end to end.
//        Other per-thread streams, so lse moves in the last bit and a
//        quarter of the step's dumped gradients move by a bf16 ulp, far
//        outside the run-to-run band of the step (one or two elements).
//        Kept opt-in, DTA_CE_FUSED=lds, for that reason alone.
#include "dta_common.h"
#include "dta_kernels.h"

namespace {

constexpr int CE_BLOCK = 256;

// A thread's two (m, s) streams, then the block's threads, into the row's
// natural-log lse.
DEV float ce_block_lse(float m0, float s0, float m1, float s1, float* lds) {
  // merge the two streams (guard empty ones: exp2(-inf - -inf) is NaN
  // for threads whose slice starts past a small vocab)
  const float m_run = fmaxf(m0, m1);
  float s_run = 0.f;
  if (m0 != -INFINITY) s_run += s0 * __builtin_exp2f(m0 - m_run);
  if (m1 != -INFINITY) s_run += s1 * __builtin_exp2f(m1 - m_run);
  // combine the per-thread (m, s) pairs across the block
  const float M = block_max<16>(m_run, lds);
  const float s_adj = s_run * __builtin_exp2f(m_run - M);
  const float S = block_sum<16>(s_adj, lds);
  return (M + __builtin_log2f(S)) * LN2;
}

// One row's natural-log lse, by the whole block (CE_BLOCK threads).
DEV float ce_row_lse(const ushort* xr, int64_t vocab, float* lds) {
  // online pass: TWO independent per-thread (m, s) streams (the single
  // running pair is a serial rescale chain — no ILP across vectors),
  // each reading a WAVE-CONTIGUOUS 1 KiB pass (stream B one full
  // block-sweep ahead — per-thread window widening shatters wave
  // coalescing, see ce_bwd_k)
  float m0 = -INFINITY, s0 = 0.f, m1 = -INFINITY, s1 = 0.f;
  const int64_t CB = int64_t(CE_BLOCK) * 8;
  int64_t i = int64_t(threadIdx.x) * 8;
  for (; i + CB + 8 <= vocab; i += 2 * CB) {
    s16x8 va = *reinterpret_cast<const s16x8*>(xr + i);
    s16x8 vb = *reinterpret_cast<const s16x8*>(xr + i + CB);
    float fa[8], fb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      fa[j] = bf2f(ushort(va[j])) * LOG2E;
      fb[j] = bf2f(ushort(vb[j])) * LOG2E;
    }
    const float mxa = fmaxf(fmaxf(fmaxf(fa[0], fa[1]), fmaxf(fa[2], fa[3])),
                            fmaxf(fmaxf(fa[4], fa[5]), fmaxf(fa[6], fa[7])));
    const float mxb = fmaxf(fmaxf(fmaxf(fb[0], fb[1]), fmaxf(fb[2], fb[3])),
                            fmaxf(fmaxf(fb[4], fb[5]), fmaxf(fb[6], fb[7])));
    const float na = fmaxf(m0, mxa), nb = fmaxf(m1, mxb);
    float pa = 0.f, pb = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      pa += __builtin_exp2f(fa[j] - na);
      pb += __builtin_exp2f(fb[j] - nb);
    }
    s0 = s0 * __builtin_exp2f(m0 - na) + pa;
    s1 = s1 * __builtin_exp2f(m1 - nb) + pb;
    m0 = na;
    m1 = nb;
  }
  for (; i + 8 <= vocab; i += CB) {
    s16x8 va = *reinterpret_cast<const s16x8*>(xr + i);
    float fa[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) fa[j] = bf2f(ushort(va[j])) * LOG2E;
    const float mxa = fmaxf(fmaxf(fmaxf(fa[0], fa[1]), fmaxf(fa[2], fa[3])),
                            fmaxf(fmaxf(fa[4], fa[5]), fmaxf(fa[6], fa[7])));
    const float na = fmaxf(m0, mxa);
    float pa = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) pa += __builtin_exp2f(fa[j] - na);
    s0 = s0 * __builtin_exp2f(m0 - na) + pa;
    m0 = na;
  }
  if (i < vocab)
    for (; i < vocab; ++i) {
      const float f = bf2f(xr[i]) * LOG2E;
      const float m_new = fmaxf(m0, f);
      s0 = s0 * __builtin_exp2f(m0 - m_new) +
           __builtin_exp2f(f - m_new);
      m0 = m_new;
    }
  return ce_block_lse(m0, s0, m1, s1, lds);
}

__global__ void ce_fwd_k(const ushort* __restrict__ logits,
                         const int64_t* __restrict__ targets, int64_t rows,
                         int64_t vocab, int64_t ignore_index,
                         float* __restrict__ lse, float* __restrict__ loss_sum,
                         int* __restrict__ count) {
  __shared__ float lds[16];
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const ushort* xr = logits + row * vocab;
    const float l = ce_row_lse(xr, vocab, lds);  // natural-log lse
    if (threadIdx.x == 0) {
      lse[row] = l;
      const int64_t tgt = targets[row];
      if (tgt != ignore_index) {
        atomicAdd(loss_sum, l - bf2f(xr[tgt]));
        atomicAdd(count, 1);
      }
    }
    __syncthreads();
  }
}

// One row's gradient, by the whole block: dxr = sc * (softmax - onehot),
// lb the row's lse in exp2 units, tgt the onehot column. dxr may be xr
// (ce_fwd_bwd_k): every element is read and then written by one thread.
template <bool NT>
DEV void ce_row_grad(const ushort* xr, ushort* dxr, int64_t vocab,
                     int64_t tgt, float lb, float sc) {
  // two WAVE-CONTIGUOUS 1 KiB passes in flight per iteration: lane l
  // reads 16 B at 16·l — perfectly coalesced — and the second pass sits
  // one whole block-sweep (CB elements) ahead. (Widening the per-THREAD
  // window instead measured 2.3x SLOWER: 32-element windows stride the
  // wave's lanes 64 B apart and shatter coalescing.)
  const int64_t CB = int64_t(CE_BLOCK) * 8;
  int64_t i = int64_t(threadIdx.x) * 8;
  for (; i + CB + 8 <= vocab; i += 2 * CB) {
    s16x8 va = *reinterpret_cast<const s16x8*>(xr + i);
    s16x8 vb = *reinterpret_cast<const s16x8*>(xr + i + CB);
    s16x8 oa, ob;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float pa = __builtin_exp2f(bf2f(ushort(va[j])) * LOG2E - lb);
      float pb = __builtin_exp2f(bf2f(ushort(vb[j])) * LOG2E - lb);
      oa[j] = f2bf(sc * (pa - ((i + j) == tgt ? 1.f : 0.f)));
      ob[j] = f2bf(sc * (pb - ((i + CB + j) == tgt ? 1.f : 0.f)));
    }
    if (NT) {
      __builtin_nontemporal_store(oa, reinterpret_cast<s16x8*>(dxr + i));
      __builtin_nontemporal_store(ob,
                                  reinterpret_cast<s16x8*>(dxr + i + CB));
    } else {
      *reinterpret_cast<s16x8*>(dxr + i) = oa;
      *reinterpret_cast<s16x8*>(dxr + i + CB) = ob;
    }
  }
  for (; i + 8 <= vocab; i += CB) {
    s16x8 va = *reinterpret_cast<const s16x8*>(xr + i);
    s16x8 oa;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float pa = __builtin_exp2f(bf2f(ushort(va[j])) * LOG2E - lb);
      oa[j] = f2bf(sc * (pa - ((i + j) == tgt ? 1.f : 0.f)));
    }
    if (NT)
      __builtin_nontemporal_store(oa, reinterpret_cast<s16x8*>(dxr + i));
    else
      *reinterpret_cast<s16x8*>(dxr + i) = oa;
  }
  if (i < vocab)
    for (; i < vocab; ++i) {
      float p = __builtin_exp2f(bf2f(xr[i]) * LOG2E - lb);
      dxr[i] = f2bf(sc * (p - (i == tgt ? 1.f : 0.f)));
    }
}

// scale_p: optional device pointer (dloss/count computed on device so the
// whole backward is hipGraph-capturable with no host sync); if null the
// host 'scale' scalar is used. v0: vocab-tile offset (the onehot column
// is targets[row] - v0). NT: nontemporal dlogits stores — right for the
// one-shot 6.5 GB pass (keeps the logits read stream L2-resident), wrong
// for the tiled pipeline (the tile is re-read by the two head GEMMs
// immediately, so it should STAY in cache).
template <bool NT>
__global__ void ce_bwd_k(const ushort* __restrict__ logits,
                         const int64_t* __restrict__ targets,
                         const float* __restrict__ lse, float scale,
                         const float* __restrict__ scale_p,
                         int64_t ignore_index, int64_t v0,
                         ushort* __restrict__ dlogits, int64_t rows,
                         int64_t vocab) {
  const float sc_base = scale_p ? *scale_p : scale;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t tgt_raw = targets[row];
    const float sc = (tgt_raw == ignore_index) ? 0.f : sc_base;
    ce_row_grad<NT>(logits + row * vocab, dlogits + row * vocab, vocab,
                    tgt_raw - v0, lse[row] * LOG2E, sc);
  }
}

// ---- one-pass forward + backward for training ------------------------------
// The training step drops the logits, and a block that has finished a row's
// online pass holds all the row's gradient needs (lse, target, 1/count). So
// one block does ce_fwd_k's pass and then ce_bwd_k's over the same row,
// IN PLACE: logits becomes dlogits = inv_count * (softmax - onehot). Both
// sweeps are the helpers above, so lse, loss_sum and dlogits are
// bit-identical to ce_fwd + ce_bwd(scale = inv_count).
// The second sweep re-reads the row from cache, not HBM: the grid is capped
// (launch_ce_fwd_bwd) so the rows in flight, 100 KB each at V = 50257, stay
// well inside the 256 MiB Infinity Cache. The stores are nontemporal so
// they do not push unread rows out.
__global__ void ce_fwd_bwd_k(ushort* logits,
                             const int64_t* __restrict__ targets,
                             int64_t rows, int64_t vocab,
                             int64_t ignore_index,
                             const float* __restrict__ inv_count,
                             float* __restrict__ lse,
                             float* __restrict__ loss_sum,
                             int* __restrict__ count) {
  __shared__ float lds[16];
  const float sc_base = *inv_count;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    ushort* xr = logits + row * vocab;
    const float l = ce_row_lse(xr, vocab, lds);
    const int64_t tgt = targets[row];
    if (threadIdx.x == 0) {
      lse[row] = l;
      if (tgt != ignore_index) {
        atomicAdd(loss_sum, l - bf2f(xr[tgt]));
        atomicAdd(count, 1);
      }
    }
    __syncthreads();   // the target logit is read before it is overwritten
    ce_row_grad<true>(xr, xr, vocab, tgt, l * LOG2E,
                      tgt == ignore_index ? 0.f : sc_base);
  }
}

// The same, with the row held in LDS between the two sweeps: a guaranteed
// single read, but one 1024-thread block per CU (the row is 100,514 B at
// V = 50257), so a CU has no loads in flight while it stores and no stores
// while it loads. The 1024 threads cut the row into other per-thread
// (m, s) streams than the 256 of ce_fwd_k: lse agrees to rounding, not bit
// for bit. `vocab` is only 2-byte aligned from row to row, so a row is
// split into head elements up to the first 16 B boundary, whole 16 B
// vectors, and tail elements; row_s[pad + i] holds xr[i] with pad chosen
// so the vectors are 16 B aligned in LDS too.
constexpr int CE_LDS_BLOCK = 1024;

DEV void ce_online8(s16x8 v, float& m, float& s) {
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = bf2f(ushort(v[j])) * LOG2E;
  const float mx = fmaxf(fmaxf(fmaxf(f[0], f[1]), fmaxf(f[2], f[3])),
                         fmaxf(fmaxf(f[4], f[5]), fmaxf(f[6], f[7])));
  const float n = fmaxf(m, mx);
  float p = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) p += __builtin_exp2f(f[j] - n);
  s = s * __builtin_exp2f(m - n) + p;
  m = n;
}

__global__ __launch_bounds__(CE_LDS_BLOCK) void ce_fwd_bwd_lds_k(
    ushort* logits, const int64_t* __restrict__ targets, int64_t rows,
    int64_t vocab, int64_t ignore_index, const float* __restrict__ inv_count,
    float* __restrict__ lse, float* __restrict__ loss_sum,
    int* __restrict__ count) {
  extern __shared__ __attribute__((aligned(16))) ushort row_s[];  // vocab + 8
  __shared__ float lds[16];
  const float sc_base = *inv_count;
  const int tid = threadIdx.x;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    ushort* xr = logits + row * vocab;
    const int64_t to16 =
        ((16 - (reinterpret_cast<uintptr_t>(xr) & 15)) & 15) >> 1;
    const int64_t head = to16 < vocab ? to16 : vocab;       // 0..7
    const int64_t nvec = (vocab - head) >> 3;
    const int64_t tail0 = head + 8 * nvec;                  // vocab - tail0 < 8
    ushort* rs = row_s + ((8 - head) & 7);                  // rs[i] <-> xr[i]
    s16x8* gv = reinterpret_cast<s16x8*>(xr + head);
    s16x8* sv = reinterpret_cast<s16x8*>(rs + head);
    // the head and tail elements, at most 14, one thread each
    const int64_t nsc = head + (vocab - tail0);
    const int64_t isc = tid < head ? tid : tail0 + (tid - head);

    float m0 = -INFINITY, s0 = 0.f, m1 = -INFINITY, s1 = 0.f;
    int64_t v = tid;
    for (; v + CE_LDS_BLOCK < nvec; v += 2 * CE_LDS_BLOCK) {
      const s16x8 va = gv[v], vb = gv[v + CE_LDS_BLOCK];
      sv[v] = va;
      sv[v + CE_LDS_BLOCK] = vb;
      ce_online8(va, m0, s0);
      ce_online8(vb, m1, s1);
    }
    for (; v < nvec; v += CE_LDS_BLOCK) {
      const s16x8 va = gv[v];
      sv[v] = va;
      ce_online8(va, m0, s0);
    }
    if (tid < nsc) {
      const ushort x = xr[isc];
      rs[isc] = x;
      const float f = bf2f(x) * LOG2E;
      const float n = fmaxf(m1, f);
      s1 = s1 * __builtin_exp2f(m1 - n) + __builtin_exp2f(f - n);
      m1 = n;
    }
    // its barriers also make row_s visible to the whole block
    const float l = ce_block_lse(m0, s0, m1, s1, lds);
    const int64_t tgt = targets[row];
    if (tid == 0) {
      lse[row] = l;
      if (tgt != ignore_index) {
        atomicAdd(loss_sum, l - bf2f(rs[tgt]));
        atomicAdd(count, 1);
      }
    }
    const float lb = l * LOG2E;
    const float sc = tgt == ignore_index ? 0.f : sc_base;
    for (v = tid; v < nvec; v += CE_LDS_BLOCK) {
      const s16x8 va = sv[v];
      const int64_t i0 = head + 8 * v;
      s16x8 oa;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = __builtin_exp2f(bf2f(ushort(va[j])) * LOG2E - lb);
        oa[j] = f2bf(sc * (p - ((i0 + j) == tgt ? 1.f : 0.f)));
      }
      __builtin_nontemporal_store(oa, gv + v);
    }
    if (tid < nsc) {
      const float p = __builtin_exp2f(bf2f(rs[isc]) * LOG2E - lb);
      xr[isc] = f2bf(sc * (p - (isc == tgt ? 1.f : 0.f)));
    }
    __syncthreads();   // row_s is read out before the next row lands in it
  }
}

// ---- pipelined head-GEMM + CE forward -------------------------------------
// The LM-head logits ([tokens, 50k] bf16, ~6.5 GB at the flagship shape)
// are produced tile-by-tile by the head GEMM; consuming each tile's
// online-softmax contribution IMMEDIATELY after its GEMM (while the tile
// is L2/Infinity-Cache resident) removes the full-logits HBM re-read of
// the one-shot ce_fwd. State: per-row running (m, s) in exp2 units.
// targets/v0/tlogit: the tile holding a row's target column records the
// target logit into tlogit[row] (exactly one tile matches per row), so
// finalize never re-touches the logits.
__global__ void ce_chunk_k(const ushort* __restrict__ chunk, int64_t ld,
                           int64_t rows, int64_t cols,
                           const int64_t* __restrict__ targets, int64_t v0,
                           float* __restrict__ tlogit,
                           float* __restrict__ m_run,
                           float* __restrict__ s_run) {
  __shared__ float lds[16];
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const ushort* xr = chunk + row * ld;
    float m_l = -INFINITY, s_l = 0.f;
    int64_t i = int64_t(threadIdx.x) * 8;
    const int64_t stride = int64_t(CE_BLOCK) * 8;
    for (; i + 8 <= cols; i += stride) {
      s16x8 vx = *reinterpret_cast<const s16x8*>(xr + i);
      float f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = bf2f(ushort(vx[j])) * LOG2E;
      float mx = fmaxf(fmaxf(fmaxf(f[0], f[1]), fmaxf(f[2], f[3])),
                       fmaxf(fmaxf(f[4], f[5]), fmaxf(f[6], f[7])));
      const float m_new = fmaxf(m_l, mx);
      float ps = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) ps += __builtin_exp2f(f[j] - m_new);
      s_l = s_l * __builtin_exp2f(m_l - m_new) + ps;
      m_l = m_new;
    }
    if (i < cols && i + 8 > cols)
      for (; i < cols; ++i) {
        const float f = bf2f(xr[i]) * LOG2E;
        const float m_new = fmaxf(m_l, f);
        s_l = s_l * __builtin_exp2f(m_l - m_new) +
              __builtin_exp2f(f - m_new);
        m_l = m_new;
      }
    const float M = block_max<16>(m_l, lds);
    const float S = block_sum<16>(s_l * __builtin_exp2f(m_l - M), lds);
    if (threadIdx.x == 0) {
      const float m0 = m_run[row], s0 = s_run[row];
      const float mn = fmaxf(m0, M);
      // first chunk: s0 == 0 (the -inf m0 exp2 underflows to 0 cleanly)
      s_run[row] = s0 * __builtin_exp2f(m0 - mn) +
                   S * __builtin_exp2f(M - mn);
      m_run[row] = mn;
      const int64_t tc = targets[row] - v0;
      if (tc >= 0 && tc < cols) tlogit[row] = bf2f(xr[tc]);
    }
    __syncthreads();
  }
}

// lse[t] = ln-units lse from (m, s); loss_sum/count accumulated over
// non-ignored rows using the tlogit recorded by the chunks.
__global__ void ce_finalize_k(const int64_t* __restrict__ targets,
                              const float* __restrict__ m_run,
                              const float* __restrict__ s_run,
                              const float* __restrict__ tlogit, int64_t rows,
                              int64_t ignore_index,
                              float* __restrict__ lse,
                              float* __restrict__ loss_sum,
                              int* __restrict__ count) {
  float part = 0.f;
  int c = 0;
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < rows;
       t += int64_t(gridDim.x) * blockDim.x) {
    const float l = (m_run[t] + __builtin_log2f(s_run[t])) * LN2;
    lse[t] = l;
    const int64_t tg = targets[t];
    if (tg != ignore_index) {
      part += l - tlogit[t];
      ++c;
    }
  }
  part = wave_sum(part);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(loss_sum, part);
    atomicAdd(count, c);
  }
}

}  // namespace

void launch_ce_chunk(const bf16_t* chunk, int64_t ld, int64_t rows,
                     int64_t cols, const int64_t* targets, int64_t v0,
                     float* tlogit, float* m_run, float* s_run,
                     hipStream_t s) {
  const int grid = int(rows < 4096 ? (rows > 0 ? rows : 1) : 4096);
  ce_chunk_k<<<grid, CE_BLOCK, 0, s>>>(chunk, ld, rows, cols, targets, v0,
                                       tlogit, m_run, s_run);
}

void launch_ce_finalize(const int64_t* targets, const float* m_run,
                        const float* s_run, const float* tlogit,
                        int64_t rows, int64_t ignore_index, float* lse,
                        float* loss_sum, int* count, hipStream_t s) {
  const int grid = elementwise_grid(rows, 256, 1);
  ce_finalize_k<<<grid, 256, 0, s>>>(targets, m_run, s_run, tlogit, rows,
                                     ignore_index, lse, loss_sum, count);
}

void launch_ce_fwd(const bf16_t* logits, const int64_t* targets, int64_t rows,
                   int64_t vocab, int64_t ignore_index, float* lse,
                   float* loss_sum, int* count, hipStream_t s) {
  const int grid = int(rows < 4096 ? (rows > 0 ? rows : 1) : 4096);
  ce_fwd_k<<<grid, CE_BLOCK, 0, s>>>(logits, targets, rows, vocab,
                                     ignore_index, lse, loss_sum, count);
}

void launch_ce_fwd_bwd(bf16_t* logits, const int64_t* targets, int64_t rows,
                       int64_t vocab, int64_t ignore_index,
                       const float* inv_count, float* lse, float* loss_sum,
                       int* count, int max_blocks, hipStream_t s) {
  const int64_t cap = max_blocks < 1 ? 1 : max_blocks;
  const int grid = int(rows < cap ? (rows > 0 ? rows : 1) : cap);
  ce_fwd_bwd_k<<<grid, CE_BLOCK, 0, s>>>(logits, targets, rows, vocab,
                                         ignore_index, inv_count, lse,
                                         loss_sum, count);
}

bool launch_ce_fwd_bwd_lds(bf16_t* logits, const int64_t* targets,
                           int64_t rows, int64_t vocab, int64_t ignore_index,
                           const float* inv_count, float* lse,
                           float* loss_sum, int* count, int n_cu,
                           int64_t lds_limit, hipStream_t s) {
  const int64_t bytes = (2 * (vocab + 8) + 15) & ~int64_t(15);
  if (bytes + 1024 > lds_limit) return false;   // row does not fit
  // raised once per size, outside any later stream capture of the step
  static int64_t allowed = 0;
  if (bytes > allowed) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(ce_fwd_bwd_lds_k),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            int(bytes)) != hipSuccess)
      return false;
    allowed = bytes;
  }
  const int64_t cap = n_cu > 0 ? n_cu : 1;      // one block fits per CU
  const int grid = int(rows < cap ? (rows > 0 ? rows : 1) : cap);
  ce_fwd_bwd_lds_k<<<grid, CE_LDS_BLOCK, size_t(bytes), s>>>(
      logits, targets, rows, vocab, ignore_index, inv_count, lse, loss_sum,
      count);
  return true;
}

void launch_ce_bwd(const bf16_t* logits, const int64_t* targets,
                   const float* lse, float scale, const float* scale_p,
                   int64_t ignore_index, int64_t v0, bool nt,
                   bf16_t* dlogits, int64_t rows, int64_t vocab,
                   hipStream_t s) {
  const int grid = int(rows < 4096 ? (rows > 0 ? rows : 1) : 4096);
  if (nt)
    ce_bwd_k<true><<<grid, CE_BLOCK, 0, s>>>(logits, targets, lse, scale,
                                             scale_p, ignore_index, v0,
                                             dlogits, rows, vocab);
  else
    ce_bwd_k<false><<<grid, CE_BLOCK, 0, s>>>(logits, targets, lse, scale,
                                              scale_p, ignore_index, v0,
                                              dlogits, rows, vocab);
}
