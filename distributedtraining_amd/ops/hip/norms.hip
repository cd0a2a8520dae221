// Fused LayerNorm / RMSNorm forward + backward.
//
// fwd: one 64-lane wave per row, values register-resident, bf16x8 loads
//      (Guideline 13); one HBM pass.
// bwd: split in two streaming kernels (measured: a fused version spent
//      ~95% of its time in a 2048-way atomicAdd flush of dγ/dβ):
//        * dx kernel — pure streaming, no reductions across rows;
//        * dγ/dβ kernel — column-parallel over row stripes into a partial
//          panel, folded by launch_colred_finish (elementwise.hip): no
//          atomics, each output written once.
//
// Replaces the implicit LayerNorm of the reference's GPT-2 fwd/bwd
// (transformers internals; SURVEY.md §2.2 op table).
#include "dta_common.h"
#include "dta_kernels.h"

#include <cstdio>
#include <type_traits>

namespace {

constexpr int ROW_WAVES = 4;

// ---- forward --------------------------------------------------------------
// RES: residual fusion — vals = round_bf16(x + res) (rounded BEFORE the
// statistics so the saved sum tensor reproduces them exactly in backward),
// and the sum is written out for the ongoing residual stream.
// DROP: counter-RNG dropout fused onto the INCOMING residual branch
// (transformers resid_pdrop: x = x + dropout(branch)) — elementwise
// chain over the branch's flat index, same draws as the standalone
// dropout kernel, so the host gold is ops.droprng.elem_keep_mask.
template <int ITERS, bool RMS, bool RES, bool DROP>
__global__ void norm_fwd_k(const ushort* __restrict__ x,
                           const ushort* __restrict__ res,
                           ushort* __restrict__ sum_out,
                           const ushort* __restrict__ w,
                           const ushort* __restrict__ b,
                           ushort* __restrict__ y, float* __restrict__ mean,
                           float* __restrict__ rstd, int64_t rows, int cols,
                           float eps,
                           const unsigned long long* __restrict__ rng,
                           unsigned long long site, unsigned int thr16,
                           float inv_keep) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nchunk = cols >> 3;
  const uint64_t s1d = DROP ? rng_site_seed(rng, site) : 0;
  for (int64_t row = int64_t(blockIdx.x) * ROW_WAVES + wid; row < rows;
       row += int64_t(gridDim.x) * ROW_WAVES) {
    const ushort* xr = x + row * cols;
    const ushort* rr = RES ? res + row * cols : nullptr;
    ushort* so = RES ? sum_out + row * cols : nullptr;
    float vals[ITERS][8];
    float sum = 0.f, sumsq = 0.f;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int c = lane + it * 64;
      if (c < nchunk) {
        s16x8 vx = *reinterpret_cast<const s16x8*>(xr + c * 8);
        s16x8 vr;
        if (RES) vr = *reinterpret_cast<const s16x8*>(rr + c * 8);
        uint64_t h0 = 0, h1 = 0;
        if (DROP) {
          const int64_t i0 = row * cols + int64_t(c) * 8;
          h0 = rng_elem_hash(s1d, uint64_t(i0 >> 2));
          h1 = rng_elem_hash(s1d, uint64_t((i0 >> 2) + 1));
        }
        s16x8 vs;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f = bf2f(ushort(vx[j]));
          if (RES) {
            float rf = bf2f(ushort(vr[j]));
            if (DROP) {
              const uint64_t h = (j < 4) ? h0 : h1;
              rf = rng_keep(h, j & 3, thr16) ? rf * inv_keep : 0.f;
            }
            const ushort sb = f2bf(f + rf);
            vs[j] = sb;
            f = bf2f(sb);
          }
          vals[it][j] = f;
          sum += f;
          sumsq = fmaf(f, f, sumsq);
        }
        if (RES) *reinterpret_cast<s16x8*>(so + c * 8) = vs;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) vals[it][j] = 0.f;
      }
    }
    sum = wave_sum(sum);
    sumsq = wave_sum(sumsq);
    const float inv_n = 1.0f / cols;
    float mu = RMS ? 0.f : sum * inv_n;
    float var = sumsq * inv_n - (RMS ? 0.f : mu * mu);
    float rs = rsqrtf(var + eps);
    if (lane == 0) {
      if (!RMS) mean[row] = mu;
      rstd[row] = rs;
    }
    ushort* yr = y + row * cols;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int c = lane + it * 64;
      if (c < nchunk) {
        s16x8 vw = *reinterpret_cast<const s16x8*>(w + c * 8);
        s16x8 vb;
        if (!RMS) vb = *reinterpret_cast<const s16x8*>(b + c * 8);
        s16x8 vy;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float xh = (vals[it][j] - mu) * rs;
          float o = xh * bf2f(ushort(vw[j]));
          if (!RMS) o += bf2f(ushort(vb[j]));
          vy[j] = f2bf(o);
        }
        *reinterpret_cast<s16x8*>(yr + c * 8) = vy;
      }
    }
  }
}

// ---- backward dx (streaming, no cross-row state) --------------------------
// LN:  dx = rs*(dyw - mean(dyw) - xh*mean(dyw*xh)),  dyw = dy*w
// RMS: dx = rs*(dyw - xh*mean(dyw*xh))
// DS: residual fusion — dx += ds (the gradient arriving on the sum
// stream from its downstream consumer), saving the separate add kernel.
// DROP: the forward dropped the residual branch, so its gradient is the
// total sum-gradient gated by the regenerated mask: dres = dx ⊙ M/(1-p)
// — one extra streaming write here instead of a separate dropout-bwd
// pass over dx.
// FDW: dγ/dβ partials accumulated IN-REGISTER here (each lane owns fixed
// columns across all its rows) and spilled once per (block, wave) to the
// partial panel — removing the separate dwdb_part kernel's full re-read
// of dy and x (~0.9 ms/step at the flagship shape). Register cost is
// 16·ITERS VGPRs, so the fusion is gated to cols ≤ 1024 (the GPT-2
// family); wider rows keep the two-kernel path.
template <int ITERS, bool RMS, bool DS, bool DROP, bool FDW>
__global__ void norm_bwd_dx_k(const ushort* __restrict__ dy,
                              const ushort* __restrict__ ds,
                              const ushort* __restrict__ x,
                              const ushort* __restrict__ w,
                              const float* __restrict__ mean,
                              const float* __restrict__ rstd,
                              ushort* __restrict__ dx,
                              ushort* __restrict__ dres,
                              float* __restrict__ pdw,
                              float* __restrict__ pdb, int64_t rows,
                              int cols,
                              const unsigned long long* __restrict__ rng,
                              unsigned long long site, unsigned int thr16,
                              float inv_keep) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nchunk = cols >> 3;
  const uint64_t s1d = DROP ? rng_site_seed(rng, site) : 0;
  float dwp[FDW ? ITERS : 1][8], dbp[(FDW && !RMS) ? ITERS : 1][8];
  if (FDW) {
#pragma unroll
    for (int it = 0; it < (FDW ? ITERS : 1); ++it)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        dwp[it][j] = 0.f;
        if (!RMS) dbp[it][j] = 0.f;
      }
  }
  float wv[ITERS][8];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int c = lane + it * 64;
    if (c < nchunk) {
      s16x8 vw = *reinterpret_cast<const s16x8*>(w + c * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) wv[it][j] = bf2f(ushort(vw[j]));
    }
  }
  for (int64_t row = int64_t(blockIdx.x) * ROW_WAVES + wid; row < rows;
       row += int64_t(gridDim.x) * ROW_WAVES) {
    const ushort* xr = x + row * cols;
    const ushort* dyr = dy + row * cols;
    const float mu = RMS ? 0.f : mean[row];
    const float rs = rstd[row];
    float xh[ITERS][8], dyw[ITERS][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int c = lane + it * 64;
      if (c < nchunk) {
        s16x8 vx = *reinterpret_cast<const s16x8*>(xr + c * 8);
        s16x8 vdy = *reinterpret_cast<const s16x8*>(dyr + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float xhj = (bf2f(ushort(vx[j])) - mu) * rs;
          const float dyv = bf2f(ushort(vdy[j]));
          float dywj = dyv * wv[it][j];
          xh[it][j] = xhj;
          dyw[it][j] = dywj;
          s1 += dywj;
          s2 = fmaf(dywj, xhj, s2);
          if (FDW) {
            dwp[it][j] = fmaf(dyv, xhj, dwp[it][j]);
            if (!RMS) dbp[it][j] += dyv;
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) { xh[it][j] = 0.f; dyw[it][j] = 0.f; }
      }
    }
    s1 = wave_sum(s1) / cols;
    s2 = wave_sum(s2) / cols;
    ushort* dxr = dx + row * cols;
    ushort* drr = DROP ? dres + row * cols : nullptr;
    const ushort* dsr = DS ? ds + row * cols : nullptr;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int c = lane + it * 64;
      if (c < nchunk) {
        s16x8 vds;
        if (DS) vds = *reinterpret_cast<const s16x8*>(dsr + c * 8);
        uint64_t h0 = 0, h1 = 0;
        if (DROP) {
          const int64_t i0 = row * cols + int64_t(c) * 8;
          h0 = rng_elem_hash(s1d, uint64_t(i0 >> 2));
          h1 = rng_elem_hash(s1d, uint64_t((i0 >> 2) + 1));
        }
        s16x8 o, od;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float v = RMS ? (dyw[it][j] - xh[it][j] * s2)
                        : (dyw[it][j] - s1 - xh[it][j] * s2);
          float g = rs * v;
          if (DS) g += bf2f(ushort(vds[j]));
          o[j] = f2bf(g);
          if (DROP) {
            const uint64_t h = (j < 4) ? h0 : h1;
            od[j] = rng_keep(h, j & 3, thr16) ? f2bf(g * inv_keep)
                                              : ushort(0);
          }
        }
        *reinterpret_cast<s16x8*>(dxr + c * 8) = o;
        if (DROP) *reinterpret_cast<s16x8*>(drr + c * 8) = od;
      }
    }
  }
  if (FDW) {
    // combine the 4 waves in LDS (cols <= 1024 when FDW) and spill ONE
    // panel row per block — keeps the panel small enough for the
    // stripe-parallel reduce (a per-(block,wave) panel was 4x larger
    // and measured 6.6 ms/step in dwdb_reduce)
    __shared__ float lred[FDW ? 2048 : 1];
    float* lw = lred;
    float* lb = lred + 1024;
    for (int i = threadIdx.x; i < cols; i += blockDim.x) {
      lw[i] = 0.f;
      if (!RMS) lb[i] = 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int c = lane + it * 64;
      if (c < nchunk) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          atomicAdd(&lw[c * 8 + j], dwp[it][j]);
          if (!RMS) atomicAdd(&lb[c * 8 + j], dbp[it][j]);
        }
      }
    }
    __syncthreads();
    float* pw = pdw + int64_t(blockIdx.x) * cols;
    float* pb = (!RMS) ? pdb + int64_t(blockIdx.x) * cols : nullptr;
    for (int i = threadIdx.x; i < cols; i += blockDim.x) {
      pw[i] = lw[i];
      if (!RMS) pb[i] = lb[i];
    }
  }
}

// ---- backward dγ/dβ (two-phase column reduction) --------------------------
// Phase 1: each (col-tile, stripe) block accumulates its stripe's rows into
// a [stripes, cols] fp32 partial panel (vectorized s16x8 row reads) — a
// single-phase version with ~1024 same-address atomicAdds per column
// measured 4x slower (per-address L2 serialization). Phase 2 is
// launch_colred_finish.
template <bool RMS>
__global__ void norm_bwd_dwdb_part_k(const ushort* __restrict__ dy,
                                     const ushort* __restrict__ x,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ rstd,
                                     float* __restrict__ pdw,
                                     float* __restrict__ pdb, int64_t rows,
                                     int cols) {
  const int c8 = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (c8 >= cols) return;
  const int64_t r0 = (rows * blockIdx.y) / gridDim.y;
  const int64_t r1 = (rows * (blockIdx.y + 1)) / gridDim.y;
  float dw_acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float db_acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int64_t r = r0; r < r1; ++r) {
    const float mu = RMS ? 0.f : mean[r];
    const float rs = rstd[r];
    s16x8 xv = *reinterpret_cast<const s16x8*>(x + r * int64_t(cols) + c8);
    s16x8 dv = *reinterpret_cast<const s16x8*>(dy + r * int64_t(cols) + c8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float dyv = bf2f(ushort(dv[j]));
      dw_acc[j] = fmaf(dyv, (bf2f(ushort(xv[j])) - mu) * rs, dw_acc[j]);
      db_acc[j] += dyv;
    }
  }
  float* pw = pdw + int64_t(blockIdx.y) * cols + c8;
#pragma unroll
  for (int j = 0; j < 8; ++j) pw[j] = dw_acc[j];
  if (!RMS) {
    float* pb = pdb + int64_t(blockIdx.y) * cols + c8;
#pragma unroll
    for (int j = 0; j < 8; ++j) pb[j] = db_acc[j];
  }
}

// ---- launch path ----------------------------------------------------------
// The instantiated row widths, in iterations of 64 lanes x 8 columns, for
// both directions (the backward stops at DTA_NORM_BWD_MAX_COLS). A row
// runs on the smallest entry >= ceil(cols / 8 / 64). Rounding up is exact:
// the iterations past the row's end are masked (c >= nchunk) and add
// nothing to the sums, so every entry wide enough gives the same bits.
constexpr int NORM_ITERS[] = {1, 2, 3, 4, 6, 8, 16};
constexpr int N_NORM_ITERS = sizeof(NORM_ITERS) / sizeof(int);
constexpr int ITER_COLS = WAVE * 8;  // columns one iteration covers
static_assert(NORM_ITERS[N_NORM_ITERS - 1] * ITER_COLS == DTA_NORM_FWD_MAX_COLS &&
              NORM_ITERS[N_NORM_ITERS - 2] * ITER_COLS == DTA_NORM_BWD_MAX_COLS);

// f(integral_constant<ITERS>) for the table entry that fits cols <= MAXC
template <int MAXC, int K = 0, class F>
void with_iters(int cols, F&& f) {
  if constexpr (K < N_NORM_ITERS && NORM_ITERS[K] * ITER_COLS <= MAXC) {
    if (cols <= NORM_ITERS[K] * ITER_COLS)
      f(std::integral_constant<int, NORM_ITERS[K]>{});
    else
      with_iters<MAXC, K + 1>(cols, f);
  } else {
    fprintf(stderr, "norm kernels: cols=%d beyond the limit %d\n", cols, MAXC);
    abort();  // the bindings check the limit first
  }
}

// f(bool_constant...) with run-time flags turned into template arguments
template <bool... Bs, class F>
void with_flags(F&& f) { f(std::bool_constant<Bs>{}...); }
template <bool... Bs, class F, class... Rest>
void with_flags(F&& f, bool b, Rest... rest) {
  b ? with_flags<Bs..., true>(f, rest...)
    : with_flags<Bs..., false>(f, rest...);
}

}  // namespace

void launch_norm_fwd(const NormFwdArgs& a, hipStream_t s) {
  const bool res = a.res != nullptr;
  const int64_t want = (a.rows + ROW_WAVES - 1) / ROW_WAVES;
  const int grid = int(want < 4096 ? (want > 0 ? want : 1) : 4096);
  const DropParams& d = a.drop;
  with_flags([&](auto RMS, auto RES, auto DROP) {
    if constexpr (RES || !DROP)
      with_iters<DTA_NORM_FWD_MAX_COLS>(a.cols, [&](auto I) {
        norm_fwd_k<I, RMS, RES, DROP><<<grid, 64 * ROW_WAVES, 0, s>>>(
            a.x, a.res, a.sum_out, a.w, a.b, a.y, a.mean, a.rstd, a.rows,
            a.cols, a.eps, d.rng, d.site, d.thr16, d.inv_keep);
      });
  }, a.rms, res, res && d.thr16 != 0);
}

void launch_norm_bwd(const NormBwdArgs& a, hipStream_t s) {
  const int grid = dta_norm_bwd_grid(a.rows);
  const DropParams& d = a.drop;
  with_flags([&](auto RMS, auto DS, auto DROP, auto FDW) {
    with_iters<DTA_NORM_BWD_MAX_COLS>(a.cols, [&](auto I) {
      norm_bwd_dx_k<I, RMS, DS, DROP, FDW><<<grid, 64 * ROW_WAVES, 0, s>>>(
          a.dy, a.ds, a.x, a.w, a.mean, a.rstd, a.dx, a.dres,
          FDW ? a.pdw : nullptr, FDW ? a.pdb : nullptr, a.rows, a.cols,
          d.rng, d.site, d.thr16, d.inv_keep);
    });
    if (!FDW) {
      const ColRedCfg cfg = dta_colred_cfg(a.rows, a.cols);
      norm_bwd_dwdb_part_k<RMS>
          <<<dim3(cfg.gx, unsigned(a.stripes)), cfg.threads, 0, s>>>(
              a.dy, a.x, a.mean, a.rstd, a.pdw, a.pdb, a.rows, a.cols);
    }
  }, a.rms, a.ds != nullptr, d.thr16 != 0, dta_norm_fused_dwdb(a.cols));
  launch_colred_finish({a.pdw, a.pdb, a.dw, a.db, a.dw_dst, a.db_dst,
                        a.stripes, a.cols, a.cols}, s);
}
