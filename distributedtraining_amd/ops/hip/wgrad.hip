// Weight-gradient GEMM with the bias gradient folded in:
//   dW[out, in] += dy[T, out]^T · x[T, in],   db[out] += sum_t dy[t, :]
// bf16 operands, fp32 accumulation, split over T (split-K), the partials
// folded in a fixed order into the bf16 flat-plane gradient views.
//
// Both operands are row-major with the summation index t as the row, so
// both MFMA fragments are k-strided. Each tile goes into LDS as the [t][cols]
// row image it has in HBM (coalesced 16 B loads, 16 B LDS writes) and both
// fragments come out of it by the transposed LDS read (ds_read_b64_tr_b16):
// per 16-lane group it returns a 4-row x 16-column block column-major, which
// is exactly the A[m][k] / B[k][n] operand of mfma_f32_16x16x32_bf16 (lane
// l: column l&15, k = 8(l>>4) + j). Two reads make one fragment.
//
// Structure:
//   * block = 512 threads (8 waves, 4 along out x 2 along in), tile
//     BM = 256 out x BN = 128 in, K-step BK = 32 rows of t; each
//     wave owns 64 x 64 = 4 x 4 accumulators of 16 x 16.
//   * two LDS buffers, one barrier per K-step: the global loads of step i+1
//     are issued before the MFMAs of step i and written to the other buffer
//     after them (three 16 B loads per thread and step).
//   * LDS image: row t of an operand tile lies at
//       (t & 7) * S + (t >> 3) * G,  S = row bytes + 32, G = 8 * S + 128
//     (dy: S = 544, G = 4480; x: S = 288, G = 2432). A transposed read's
//     32-lane half takes rows 4r+q and 8+4r+q (q = 0..3), 32 B of each: with
//     S = 32 and G = 128 (mod 256) those are the eight distinct 32 B slots of
//     the 256 B bank row, so every fragment read is conflict-free.
//   * EXEC is all ones at every transposed read: the loops and the bias
//     branch are block- or wave-uniform, there is no return before the last
//     barrier, and rows t >= T are staged as zeros (the ragged last K-step is
//     padded, never masked).
//   * grid = tiles x nsplit, slice-major: the blocks of one K slice (they
//     share the dy and x row panels) have consecutive ids after the bijective
//     XCD remap and so share an L2. Slices are whole K-steps; a slice without
//     steps stores zeros, so the slab is never zero-filled.
//   * BIAS instantiation: in the blocks of tile column 0 the four waves with
//     wn == 0 feed each dy fragment to one more MFMA as the B operand of a
//     0/1 row selector (4 more MFMAs per K-step, one extra accumulator); the
//     product's rows are sum_t dy. The no-bias instantiation has none of it.
//   * wgrad_fold_k sums the [nsplit] slabs of every element in ascending
//     slice order and delivers dst = bf16(float(dst) + sum) into the bf16
//     gradient view (2 B aligned in general: 4 elements per lane where the
//     view is 8 B aligned, else one), the bias partials likewise or as an
//     fp32 store. No float atomics; every output is written once.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   wgrad_k<false> 122 VGPRs, nothing spilled; wgrad_k<true> 128 VGPRs, 3
//   spilled (16 B scratch; the one reload inside the loop sits in the ragged
//   branch); 55296 B LDS; 4 waves/SIMD = 2 blocks/CU, which the waves_per_eu
//   attribute asks for: left alone hipcc takes 134 / 150 VGPRs and one block
//   per CU, which this one-barrier loop cannot keep busy.
#include "dta_common.h"
#include "dta_kernels.h"

namespace {

constexpr int BM = DTA_WGRAD_BM, BN = DTA_WGRAD_BN, BK = DTA_WGRAD_BK;
constexpr int WG_THREADS = 512;
static_assert(BM == 256 && BN == 128 && BK == 32, "wave layout and staging");

constexpr int A_S = BM * 2 + 32, A_G = 8 * A_S + 128;   // 544, 4480
constexpr int B_S = BN * 2 + 32, B_G = 8 * B_S + 128;   // 288, 2432
constexpr int A_BYTES = (BK / 8) * A_G;                 // 17920
constexpr int B_BYTES = (BK / 8) * B_G;                 // 9728
constexpr int BUF_BYTES = A_BYTES + B_BYTES;            // 27648
static_assert(A_S % 256 == 32 && B_S % 256 == 32, "bank spread of rows");
static_assert(A_G % 256 == 128 && B_G % 256 == 128, "bank spread of groups");

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// fragment of 16 columns x 32 rows t at p (this lane's address, see above)
DEV bf16x8 tr_frag(const char* p, int row_stride) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
  const s16x4 hi =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * row_stride));
  return as_bf16x8(__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <bool BIAS>
__global__ __launch_bounds__(WG_THREADS)
__attribute__((amdgpu_waves_per_eu(4, 4))) void wgrad_k(
    const ushort* __restrict__ dy, int64_t ld_dy, const ushort* __restrict__ x,
    int64_t ld_x, int64_t T, int out, int in, int nsplit,
    float* __restrict__ slab, float* __restrict__ bpart) {
  __shared__ __attribute__((aligned(16))) char lds[2 * BUF_BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform
  const int wm = wid >> 1, wn = wid & 1;
  const int fr = lane & 15, fq = lane >> 4;

  // block id -> (slice, tile), slice-major, through the bijective XCD remap
  const int tiles_n = in / BN;
  const int tiles = (out / BM) * tiles_n;
  const int nwg = gridDim.x;
  const int bq = nwg >> 3, br = nwg & 7;
  const int xcd = blockIdx.x & 7;
  const int wgid = (xcd < br ? xcd * (bq + 1) : br * (bq + 1) + (xcd - br) * bq) +
                   (blockIdx.x >> 3);
  const int slice = wgid / tiles, tile = wgid - slice * tiles;
  const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  const int64_t ksteps = (T + BK - 1) / BK;
  const int64_t k_begin = ksteps * slice / nsplit;
  const int64_t k_end = ksteps * (slice + 1) / nsplit;
  const int nsteps = int(k_end - k_begin);   // block-uniform, may be 0

  // staging: dy rows ar and ar + 16, 16 B chunk ac; x row br_, chunk bc
  const int ac = tid & 31, ar = tid >> 5;
  const int bc = tid & 15, br_ = tid >> 4;
  // a K-step's rows start at a block-uniform 64-bit base; the lane's part
  // of the byte offset is 32-bit (32 rows: ld < 2^25 at the binding)
  const char* abase = reinterpret_cast<const char*>(dy + m0);
  const char* bbase = reinterpret_cast<const char*>(x + n0);
  const unsigned a_col = ac * 16, b_col = bc * 16;
  const unsigned a_ldb = unsigned(ld_dy) * 2, b_ldb = unsigned(ld_x) * 2;
  const int a_st0 = (ar & 7) * A_S + (ar >> 3) * A_G + ac * 16;
  const int a_st1 = a_st0 + 2 * A_G;   // row ar + 16
  const int b_st = A_BYTES + (br_ & 7) * B_S + (br_ >> 3) * B_G + bc * 16;

  // fragment reads: lane 4q+p of group g -> row 8g + (4r) + q, columns 4p..
  const int tq = fr >> 2, tp = fr & 3;
  const int a_rd = tq * A_S + fq * A_G + (wm * 64 + 4 * tp) * 2;
  const int b_rd = A_BYTES + tq * B_S + fq * B_G + (wn * 64 + 4 * tp) * 2;

  const bool bias_wave = BIAS && tn == 0 && wn == 0;   // wave-uniform

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 bacc = {0.f, 0.f, 0.f, 0.f};

  s16x8 ga0, ga1, gb;
  const s16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  auto gload = [&](int64_t kstep) {
    const int64_t t0 = kstep * BK;
    const char* arow = abase + t0 * ld_dy * 2;
    const char* brow = bbase + t0 * ld_x * 2;
    if (t0 + BK <= T) {   // block-uniform: every step but a ragged last one
      ga0 = *reinterpret_cast<const s16x8*>(arow + (ar * a_ldb + a_col));
      ga1 = *reinterpret_cast<const s16x8*>(arow + ((ar + 16) * a_ldb + a_col));
      gb = *reinterpret_cast<const s16x8*>(brow + (br_ * b_ldb + b_col));
    } else {              // rows t >= T: load the last row, stage zeros
      const int rem = int(T - t0);   // 1 .. BK - 1 valid rows
      const int r0 = ar < rem ? ar : rem - 1;
      const int r1 = ar + 16 < rem ? ar + 16 : rem - 1;
      const int rb = br_ < rem ? br_ : rem - 1;
      ga0 = *reinterpret_cast<const s16x8*>(arow + (r0 * a_ldb + a_col));
      ga1 = *reinterpret_cast<const s16x8*>(arow + (r1 * a_ldb + a_col));
      gb = *reinterpret_cast<const s16x8*>(brow + (rb * b_ldb + b_col));
      if (ar >= rem) ga0 = zero8;
      if (ar + 16 >= rem) ga1 = zero8;
      if (br_ >= rem) gb = zero8;
    }
  };
  auto lds_write = [&](char* buf) {
    *reinterpret_cast<s16x8*>(buf + a_st0) = ga0;
    *reinterpret_cast<s16x8*>(buf + a_st1) = ga1;
    *reinterpret_cast<s16x8*>(buf + b_st) = gb;
  };

  if (nsteps > 0) {
    gload(k_begin);
    lds_write(lds);
  }
  __syncthreads();

  for (int it = 0; it < nsteps; ++it) {
    const bool more = it + 1 < nsteps;   // block-uniform
    if (more) gload(k_begin + it + 1);

    const char* buf = lds + (it & 1) * BUF_BYTES;
    bf16x8 a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = tr_frag(buf + a_rd + i * 32, A_S);
      b[i] = tr_frag(buf + b_rd + i * 32, B_S);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[i][n] = mfma_bf16(a[i], b[n], acc[i][n]);
    if (BIAS && bias_wave) {
      // rows 4i..4i+3 of the selector are ones, so rows 4i..4i+3 of the
      // product (lane group i) collect the column sums of fragment i: one
      // accumulator for all four. Built per step: four hoisted selector
      // fragments would cost the registers the second block per CU needs.
      int sel = tq;
      asm volatile("" : "+v"(sel));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const short one = sel == i ? short(0x3F80) : short(0);   // bf16 1.0
        const s16x8 o = {one, one, one, one, one, one, one, one};
        bacc = mfma_bf16(as_bf16x8(o), a[i], bacc);
      }
    }

    if (more) lds_write(lds + ((it + 1) & 1) * BUF_BYTES);
    __syncthreads();
  }

  // slab[slice][m][n]: row 4*fq + j, column fr of every 16 x 16 accumulator
  float* sp = slab + int64_t(slice) * out * int64_t(in) +
              int64_t(m0 + wm * 64 + 4 * fq) * in + n0 + wn * 64 + fr;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int n = 0; n < 4; ++n)
        sp[int64_t(i * 16 + j) * in + n * 16] = acc[i][n][j];
  if (BIAS && bias_wave)   // lane group fq holds fragment fq, column fr
    bpart[int64_t(slice) * out + m0 + wm * 64 + fq * 16 + fr] = bacc[0];
}

// sum of element e over the slabs, ascending slice order
DEV float fold1(const float* __restrict__ p, int64_t stride, int ns) {
  float s = p[0];
#pragma unroll 4
  for (int i = 1; i < ns; ++i) s += p[int64_t(i) * stride];
  return s;
}

// blocks [0, wblocks): weights; the rest: bias. VEC: dw is 8 B aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void wgrad_fold_k(
    const float* __restrict__ slab, int ns, int64_t n_w, ushort* __restrict__ dw,
    int wblocks, const float* __restrict__ bpart, int n_b,
    ushort* __restrict__ db, float* __restrict__ bout) {
  if (int(blockIdx.x) < wblocks) {
    if (VEC) {
      const int64_t e = (int64_t(blockIdx.x) * 256 + threadIdx.x) * 4;
      if (e < n_w) {   // n_w % 4 == 0
        f32x4 s = *reinterpret_cast<const f32x4*>(slab + e);
#pragma unroll 4
        for (int i = 1; i < ns; ++i)
          s += *reinterpret_cast<const f32x4*>(slab + int64_t(i) * n_w + e);
        s16x4 d = *reinterpret_cast<const s16x4*>(dw + e);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          d[j] = short(f2bf(bf2f(ushort(d[j])) + s[j]));
        *reinterpret_cast<s16x4*>(dw + e) = d;
      }
    } else {
      const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
      if (e < n_w) dw[e] = f2bf(bf2f(dw[e]) + fold1(slab + e, n_w, ns));
    }
  } else {
    const int e = (int(blockIdx.x) - wblocks) * 256 + threadIdx.x;
    if (e < n_b) {
      const float s = fold1(bpart + e, n_b, ns);
      if (db) db[e] = f2bf(bf2f(db[e]) + s);
      else bout[e] = s;
    }
  }
}

}  // namespace

void launch_wgrad(const WgradArgs& a, hipStream_t s) {
  const int tiles = (a.out / BM) * (a.in / BN);
  const unsigned grid = unsigned(tiles) * unsigned(a.nsplit);
  if (a.bpart)
    wgrad_k<true><<<grid, WG_THREADS, 0, s>>>(a.dy, a.ld_dy, a.x, a.ld_x, a.T,
                                              a.out, a.in, a.nsplit, a.slab,
                                              a.bpart);
  else
    wgrad_k<false><<<grid, WG_THREADS, 0, s>>>(a.dy, a.ld_dy, a.x, a.ld_x, a.T,
                                               a.out, a.in, a.nsplit, a.slab,
                                               nullptr);
  const int64_t n_w = int64_t(a.out) * a.in;
  const bool vec = reinterpret_cast<uintptr_t>(a.dw) % 8 == 0;
  const int wblocks = int((n_w + (vec ? 1024 : 256) - 1) / (vec ? 1024 : 256));
  const int n_b = a.bpart ? a.out : 0;
  const unsigned fgrid = unsigned(wblocks + (n_b + 255) / 256);
  if (vec)
    wgrad_fold_k<true><<<fgrid, 256, 0, s>>>(a.slab, a.nsplit, n_w, a.dw,
                                             wblocks, a.bpart, n_b, a.db,
                                             a.bout);
  else
    wgrad_fold_k<false><<<fgrid, 256, 0, s>>>(a.slab, a.nsplit, n_w, a.dw,
                                              wblocks, a.bpart, n_b, a.db,
                                              a.bout);
}
