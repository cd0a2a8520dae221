// Forward projection GEMM with the bias and GELU applied to the accumulators:
//   y[T, N] = x[T, K] · w[N, K]^T (+ b)          EPI_NONE / EPI_BIAS
//   pre = bf16(x·w^T + b), h = bf16(gelu(pre))    EPI_BIAS_GELU (two outputs)
// bf16 operands, fp32 accumulation on mfma_f32_16x16x32_bf16, one rounding
// per output. GELU is applied to the ROUNDED pre, so h is bit for bit what
// gelu_fwd gives on the stored pre and the backward (which reads pre) sees the
// activation the forward used.
//
// Both operands are K-contiguous, so both tiles go into LDS as the row images
// they have in HBM and both MFMA fragments are single 16 B LDS reads (no
// transposed reads, unlike wgrad.hip).
//
// Structure:
//   * block = 512 threads (8 waves, 4 along tokens x 2 along features), tile
//     BM = 256 tokens x BN = 128 features; each wave owns 64 x 64 = 4 x 4
//     accumulators of 16 x 16. At 256 x 128 the tile asks L2 for 1 B per 85
//     flop; 128 x 128 (1 B per 64 flop) is bound by the operand stream.
//   * swapped product as head_loss.hip: A = w tile, B = x tile, so
//     D[feature][token] puts one token on a lane (lane & 15) with 4
//     consecutive features per accumulator in its registers
//     (4 (lane >> 4) + reg): the bias is 4 values per fragment, loaded once.
//   * K loop: ST stages of KB columns in LDS, register staging, ONE barrier
//     per K-step. Step i + ST - 1 is loaded from global memory before the
//     MFMAs of step i and written to its stage after them; that stage was
//     last read in step i - 1, which the barrier of step i - 1 has retired.
//     Two pipelines are instantiated:
//       2 x 32: KB = 32, two stages, 48 KB of LDS, 4 waves/SIMD = two blocks
//               per CU (one block's MFMAs cover the other's barrier);
//       3 x 64: KB = 64, three stages, 144 KB of LDS, one block per CU: the
//               stage written in step i is not read before step i + 2, so no
//               wave waits at the barrier for its own LDS writes to land.
//     The contract's K granule is 64 for both.
//   * LDS images. KB = 64: unpadded 128 B rows, the 16 B chunk XOR-swizzled
//     by (row >> 1) & 7, the image of head_loss.hip. KB = 32: 64 B rows; a
//     group of 16 rows is 1 KB with chunk c of row r at
//       ((r>>1)&3) * 256 + (r&1) * 128 + ((r>>3)&1) * 64 + (c ^ ((r>>1)&3)) * 16.
//     A fragment read (lane: row lane & 15, chunk lane >> 4) then falls on the
//     same 16 B slot of the 256 B bank row as in the KB = 64 image, lane for
//     lane, so it is conflict-free wherever that one is; the map is a
//     bijection of the group's 64 chunks.
//   * rows >= T: the load row is clamped to T - 1, nothing is stored. The
//     block's first row and every output row offset are int64; a lane's
//     offset inside the tile's 256 rows is 32-bit (ld_x, K < 2^22 at the
//     binding).
//   * epilogue through LDS, after the loop's last barrier has retired every
//     fragment read: each wave rounds its 64 x 64 block in two halves of 32
//     tokens into a private 4 KB region ([32 tokens][64 features] bf16, 128 B
//     rows, chunk ^ (token & 7)) and reads it back row-wise, so global stores
//     are 16 B per lane, 8 lanes covering the wave's 128 B of a row, not 8 B
//     fragments strided over 16 rows. EPI_BIAS_GELU passes twice, pre then h.
//   * grid = row tiles x feature tiles, one tile per block, through the
//     bijective XCD remap of wgrad.hip; the feature tiles of one row tile
//     (they share the x row panel) have consecutive ids and so share an L2.
//   * no atomics, no workspace, no host sync: capturable, bit-repeatable.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), the same
// for the three epilogues of a pipeline:
//   gemm_nt_k<*, 32, 2>: 116 VGPRs, 0 AGPRs, nothing spilled, no scratch,
//     49152 B LDS, occupancy 4 waves/SIMD = 2 blocks/CU (the waves_per_eu
//     attribute asks for it).
//   gemm_nt_k<*, 64, 3>: 135 VGPRs, 0 AGPRs, nothing spilled, no scratch,
//     147456 B LDS, occupancy 2 waves/SIMD = 1 block/CU (the LDS limit).
// Measured (profiles/r12_gemm_fwd.md): 2 x 32 is the faster pipeline at every
// flagship shape and is the default; the library is faster than both.
#include "dta_common.h"
#include "dta_kernels.h"

#ifndef DTA_GEMM_PIPE_DEFAULT
#define DTA_GEMM_PIPE_DEFAULT GEMM_PIPE_2X32
#endif

namespace {

constexpr int BM = DTA_GEMM_BM, BN = DTA_GEMM_BN;
constexpr int GM_THREADS = 512;
static_assert(BM == 256 && BN == 128 && DTA_GEMM_BK == 64,
              "wave layout, staging passes and the K granule");

constexpr int EP_WAVE = 32 * 64 * 2;   // a wave's epilogue region: 4 KB

// byte offset of 16 B chunk c of row r in a tile image with KB-column rows
template <int KB> DEV int img_off(int r, int c) {
  if (KB == 64) return r * 128 + ((c ^ ((r >> 1) & 7)) << 4);
  return (r >> 4) * 1024 + ((r >> 1) & 3) * 256 + (r & 1) * 128 +
         ((r >> 3) & 1) * 64 + ((c ^ ((r >> 1) & 3)) << 4);
}

// The epilogue's fp32 adds and multiplies stay scalar instructions: the
// packed two-lane fp32 forms are switched off for this kernel.
template <int EPI, int KB, int ST>
__global__ __launch_bounds__(GM_THREADS)
__attribute__((amdgpu_waves_per_eu(ST == 2 ? 4 : 2, ST == 2 ? 4 : 2)))
__attribute__((target("no-packed-fp32-ops")))
void gemm_nt_k(const ushort* __restrict__ x, int64_t ld_x,
               const ushort* __restrict__ w, const ushort* __restrict__ bias,
               ushort* __restrict__ y, ushort* __restrict__ aux, int64_t T,
               int N, int K) {
  static_assert(KB == 32 || KB == 64, "two row images");
  constexpr int CH = KB / 8;             // 16 B chunks per row
  constexpr int RPP = GM_THREADS / CH;   // rows one staging pass covers
  constexpr int XP = BM / RPP, WP = BN / RPP;
  constexpr int PASS_BYTES = RPP * KB * 2;   // 8 KB for both images
  constexpr int W_BYTES = BN * KB * 2, X_BYTES = BM * KB * 2;
  constexpr int STAGE = W_BYTES + X_BYTES;
  constexpr int KK = KB / 32;            // MFMA K-blocks per stage
  static_assert(ST * STAGE >= 8 * EP_WAVE, "the epilogue reuses the stages");
  __shared__ __attribute__((aligned(16))) char lds[ST * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform
  const int wt = wid >> 1, wf = wid & 1;   // token quarter, feature half
  const int fr = lane & 15, fq = lane >> 4;

  // block id -> (row tile, feature tile), feature tiles consecutive, through
  // the bijective XCD remap
  const int tiles_n = N / BN;
  const int nwg = gridDim.x;
  const int bq = nwg >> 3, br = nwg & 7;
  const int xcd = blockIdx.x & 7;
  const int wgid = (xcd < br ? xcd * (bq + 1) : br * (bq + 1) + (xcd - br) * bq) +
                   (blockIdx.x >> 3);
  const int tm = wgid / tiles_n, tn = wgid - tm * tiles_n;
  const int64_t m0 = int64_t(tm) * BM;
  const int n0 = tn * BN;
  const int rows_left = int(T - m0 < BM ? T - m0 : BM);   // 1 .. BM

  // staging: 16 B chunk sc of rows sr + p * RPP
  const int sc = tid & (CH - 1), sr = tid / CH;
  const int st_off = img_off<KB>(sr, sc);   // + p * PASS_BYTES for pass p
  const char* xb = reinterpret_cast<const char*>(x + m0 * ld_x);
  const char* wb = reinterpret_cast<const char*>(w + int64_t(n0) * K);
  unsigned xo[XP], wo[WP];
#pragma unroll
  for (int p = 0; p < XP; ++p) {
    const int r = sr + p * RPP;
    xo[p] = unsigned(r < rows_left ? r : rows_left - 1) * (unsigned(ld_x) * 2u) +
            unsigned(sc * 16);
  }
#pragma unroll
  for (int p = 0; p < WP; ++p)
    wo[p] = unsigned(sr + p * RPP) * (unsigned(K) * 2u) + unsigned(sc * 16);

  // fragment reads: row fr of the wave's 16-row block i, chunk 4 kk + fq;
  // block i lies i * 16 * KB * 2 bytes further on in both images
  int a_rd[KK], b_rd[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    a_rd[kk] = img_off<KB>(wf * 64 + fr, kk * 4 + fq);
    b_rd[kk] = W_BYTES + img_off<KB>(wt * 64 + fr, kk * 4 + fq);
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  s16x8 gw[WP], gx[XP];
  auto gload = [&](int ks) __attribute__((always_inline)) {
    const char* wk = wb + ks * (KB * 2);
    const char* xk = xb + ks * (KB * 2);
#pragma unroll
    for (int p = 0; p < WP; ++p)
      gw[p] = *reinterpret_cast<const s16x8*>(wk + wo[p]);
#pragma unroll
    for (int p = 0; p < XP; ++p)
      gx[p] = *reinterpret_cast<const s16x8*>(xk + xo[p]);
  };
  auto lds_write = [&](char* buf) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < WP; ++p)
      *reinterpret_cast<s16x8*>(buf + st_off + p * PASS_BYTES) = gw[p];
#pragma unroll
    for (int p = 0; p < XP; ++p)
      *reinterpret_cast<s16x8*>(buf + W_BYTES + st_off + p * PASS_BYTES) = gx[p];
  };

  const int nk = K / KB;   // >= 1: K % 64 == 0
#pragma unroll
  for (int s = 0; s < ST - 1; ++s)
    if (s < nk) {
      gload(s);
      lds_write(lds + s * STAGE);
    }
  __syncthreads();

  int cur = 0, nxt = ST - 1;   // stage computed / stage written this step
  for (int it = 0; it < nk; ++it) {
    const bool more = it + ST - 1 < nk;   // block-uniform
    if (more) gload(it + ST - 1);

    const char* buf = lds + cur * STAGE;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      bf16x8 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = as_bf16x8(*reinterpret_cast<const s16x8*>(
            buf + a_rd[kk] + i * (16 * KB * 2)));
        b[i] = as_bf16x8(*reinterpret_cast<const s16x8*>(
            buf + b_rd[kk] + i * (16 * KB * 2)));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[i][n] = mfma_bf16(a[i], b[n], acc[i][n]);
    }

    if (more) lds_write(lds + nxt * STAGE);
    __syncthreads();
    cur = cur + 1 == ST ? 0 : cur + 1;
    nxt = nxt + 1 == ST ? 0 : nxt + 1;
  }

  // ---- epilogue -----------------------------------------------------------
  // bias of this lane's features n0 + wf*64 + 16 i + 4 fq + r (2 B loads: a
  // flat-plane bias view has no alignment)
  float bv[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      bv[i][r] = EPI == GEMM_EPI_NONE
                     ? 0.f
                     : bf2f(bias[n0 + wf * 64 + i * 16 + 4 * fq + r]);

  char* ep = lds + wid * EP_WAVE;
  // write: token t = 16 nn + fr of the half, features 16 i + 4 fq .. + 3
  const int ep_wr = fr * 128 + (fq & 1) * 8;
  const int ep_sw = fr & 7, ep_c = fq >> 1;
  // read: row lane >> 3 (+ 8 per pass), chunk lane & 7
  const int rd_row = lane >> 3;
  const int ep_rd = rd_row * 128 + (((lane & 7) ^ (rd_row & 7)) << 4);
  const int64_t out_col = n0 + wf * 64 + (lane & 7) * 8;
  constexpr int NOUT = EPI == GEMM_EPI_BIAS_GELU ? 2 : 1;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s16x4 v;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float f = acc[i][half * 2 + nn][r];
            ushort p = f2bf(EPI == GEMM_EPI_NONE ? f : f + bv[i][r]);
            if (o == 1) p = f2bf(gelu_f(bf2f(p)));
            v[r] = short(p);
          }
          *reinterpret_cast<s16x4*>(ep + nn * (16 * 128) + ep_wr +
                                    (((i * 2 + ep_c) ^ ep_sw) << 4)) = v;
        }
      __syncthreads();
      ushort* dst = o == 0 ? y : aux;
#pragma unroll
      for (int ps = 0; ps < 4; ++ps) {
        const s16x8 v =
            *reinterpret_cast<const s16x8*>(ep + ps * (8 * 128) + ep_rd);
        const int row = wt * 64 + half * 32 + ps * 8 + rd_row;
        if (row < rows_left)
          *reinterpret_cast<s16x8*>(dst + (m0 + row) * int64_t(N) + out_col) = v;
      }
      __syncthreads();
    }
  }
}

template <int KB, int ST>
void launch_pipe(const GemmArgs& a, unsigned grid, hipStream_t s) {
  switch (a.epi) {
    case GEMM_EPI_NONE:
      gemm_nt_k<GEMM_EPI_NONE, KB, ST><<<grid, GM_THREADS, 0, s>>>(
          a.x, a.ld_x, a.w, a.bias, a.y, a.aux, a.T, a.N, a.K);
      break;
    case GEMM_EPI_BIAS:
      gemm_nt_k<GEMM_EPI_BIAS, KB, ST><<<grid, GM_THREADS, 0, s>>>(
          a.x, a.ld_x, a.w, a.bias, a.y, a.aux, a.T, a.N, a.K);
      break;
    default:
      gemm_nt_k<GEMM_EPI_BIAS_GELU, KB, ST><<<grid, GM_THREADS, 0, s>>>(
          a.x, a.ld_x, a.w, a.bias, a.y, a.aux, a.T, a.N, a.K);
  }
}

}  // namespace

void launch_gemm_nt(const GemmArgs& a, hipStream_t s, int pipe) {
  const int64_t row_tiles = (a.T + BM - 1) / BM;
  const unsigned grid = unsigned(row_tiles * (a.N / BN));
  if ((pipe ? pipe : int(DTA_GEMM_PIPE_DEFAULT)) == GEMM_PIPE_3X64)
    launch_pipe<64, 3>(a, grid, s);
  else
    launch_pipe<32, 2>(a, grid, s);
}
