// Int4 weight-only skinny GEMM for serving decode (W4A16), 1 <= M <= 16:
//   y[M, N] = x[M, K] · Wq[N, K]^T (+ bias),
//   Wq[n, k] = float(u[n, k] - 8) * s[n, k / 128]
// bf16 activations and output, 4-bit codes u = q + 8 in 1 .. 15 (q in -7 .. 7)
// with one fp32 scale per (row, group of 128 along K), fp32 accumulation on
// mfma_f32_16x16x32_bf16, one rounding per output. A decode projection is a
// weight stream; this kernel reads 0.53 B per weight against 1.03 of the int8
// kernel (w8_gemv.hip), whose decomposition it keeps: swapped product, x in
// LDS once per block, weights in registers only, optional K split with a
// fixed-order fold.
//
// Packed weight (ops/w8.py writes it once, offline; docs/serving.md):
//   rows padded with the zero code (nibble 8) to Np = ceil16(N);
//   codes  uint8 [Np/16][K/128][64][16]: the 1 KB of a (16-row tile, group)
//          in lane order, lane l = row l % 16, the 32 columns 32 (l / 16) ..
//          of the group. Its 16 B are four dwords; dword d is the whole A
//          fragment of MFMA d of the group: the MFMA's k index 8 (l / 16) + e
//          stands for column 32 (l / 16) + 8 d + e, and the activation
//          fragment below uses the same order. Nibble s of the dword (bits
//          4 s .. 4 s + 3) is element 2 s, nibble s + 4 is element 2 s + 1,
//          s = 0 .. 3;
//   scales fp32 [Np/16][K/128][16]: 64 B per (tile, group), as for int8.
//
// What is this kernel's own:
//   * unpack without converts. 0x4300 | n is the bf16 number 128 + n, exact
//     for n < 128, so ((dword >> 4 s) & 0x000F000F) | 0x43004300 is the packed
//     pair of fragment elements 2 s, 2 s + 1 as the exact bf16 values 136 + q:
//     a shift and one and-or per pair, 7 integer ops per MFMA, no cvt (the
//     int8 kernel spends 8 sign-extends, 8 int -> float and 4 packing
//     converts on the same fragment). The group accumulator ga then holds
//     sum (136 + q) x. The offset leaves on the matrix unit as well: every B
//     fragment is multiplied a second time, by a constant A fragment of
//     -136 (bf16 0xC308, exact), into a second accumulator go, and
//       acc[row] += scale[row] * (ga[row] + go[row]).
//     Two independent chains of 4 MFMAs per group on a matrix unit that a
//     weight stream otherwise leaves idle. The price is cancellation:
//     136 |sum x| is about 30 x the code sum at randn-like x, so the fp32
//     rounding of the two chains comes back as about 2e-6 of a group's
//     result, against bf16's 2^-8 output rounding (measured figures:
//     profiles/r19_w4_gemv.md). The other route, a
//     per-(token, group) fp32 sum of x formed while the stage is written and
//     subtracted as 136 * xsum in the scale FMA, was built and measured: its
//     16-lane butterflies sit between the stage barriers where nothing hides
//     them, and it lost to int8 at M = 16 (profiles/r19_w4_gemv.md).
//   * loads in flight. A lane's group is one 16 B code load plus one 16 B
//     scale load, half of int8's bytes, so the register ring is DEPTH = 8
//     groups deep: 16 loads per lane, 16 KB of requests per wave of which
//     8 KB are codes (what w8_gemv_k keeps in flight at depth 4), in 64 ring
//     VGPRs. Eight groups are also exactly one 1024-column LDS stage, so one
//     turn of the ring is one stage: straight-line code between two barriers,
//     and slot i is group i of the stage. A slot is refilled right after it
//     is consumed; the refills of a stage's last groups are in flight across
//     the next stage's barriers.
//   * split rule dta_w4_nsplit (dta_kernels.h): two blocks per CU, but a
//     slice is never shorter than one turn of the ring (8 groups) where K has
//     two turns to share out, and K < 2048 is not split at all.
//
// Structure (as w8_gemv_k): block = 256 threads, 4 waves, 64 output rows (one
// 16-row tile per wave) and one K slice (blockIdx.y). x stage [16 tokens]
// [1024] bf16 = 32 KB of LDS, 16 B chunk index XOR-ed with the token so
// that the 16 tokens of a fragment read fall on 16 different chunks of a
// 256 B bank row; rows >= M are zeroed once. D[row][token] puts
// token l % 16 on a lane with rows 4 (l / 16) + r in its registers. nsplit == 1:
// acc + bias in fp32, one bf16 rounding, direct store; nsplit > 1: fp32
// partials [nsplit, M, N], folded in ascending slice order by the int8
// route's fold kernel. Every loop bound and every branch around a barrier is
// block-uniform; a wave whose tile lies past Np skips its loads and MFMAs
// wave-uniformly and still stages x and reaches every barrier. Rows >= N and
// tokens >= M are never stored. No atomics, every output written once:
// bit-repeatable and capturable.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950) are listed
// in docs/kernels.md.
#include "dta_common.h"
#include "dta_kernels.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;

constexpr int W4_THREADS = 256;
constexpr int W4_STAGE = 1024;            // x columns per LDS stage
constexpr int W4_ROW_BYTES = W4_STAGE * 2;
constexpr int W4_DEPTH = DTA_W4_RING;     // groups in flight per lane
constexpr int W4_SG = W4_STAGE / DTA_W8_GROUP;   // groups per stage
static_assert(W4_SG == W4_DEPTH, "one turn of the ring is one LDS stage");

// dword d of a lane's codes -> the A fragment of MFMA d: 136 + q, exact
DEV bf16x8 nibbles_to_bf16(unsigned w) {
  union { i32x4 i; bf16x8 b; } u;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    u.i[s] = int(((w >> (4 * s)) & 0x000F000Fu) | 0x43004300u);
  return u.b;
}

// The scale FMAs and the bias add stay scalar instructions: the packed
// two-lane fp32 forms are switched off for these kernels.
template <bool SPLIT>
__global__ __launch_bounds__(W4_THREADS)
__attribute__((target("no-packed-fp32-ops")))
void w4_gemv_k(const ushort* __restrict__ x,
               const unsigned char* __restrict__ codes,
               const float* __restrict__ scales,
               const ushort* __restrict__ bias, ushort* __restrict__ y,
               float* __restrict__ part, int M, int N, int K, int kslice) {
  __shared__ __attribute__((aligned(16))) char xs[16 * W4_ROW_BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ft = lane & 15, fq = lane >> 4;   // token / row, K quarter

  const int tiles = (N + 15) >> 4;
  const int tile = blockIdx.x * 4 + wid;
  const bool active = tile < tiles;           // wave-uniform
  const int groups = K / DTA_W8_GROUP;
  const int k_begin = blockIdx.y * kslice;
  const int k_end = k_begin + kslice < K ? k_begin + kslice : K;
  const int ngs = k_end > k_begin ? (k_end - k_begin) / DTA_W8_GROUP : 0;

  // this lane's 16 B of group 0 of the slice; + 1 KB per group
  const unsigned char* cp =
      codes + (int64_t(tile) * groups + k_begin / DTA_W8_GROUP) * 1024 +
      lane * 16;
  // its 4 row scales of group 0 of the slice; + 16 floats per group
  const float* sp =
      scales + (int64_t(tile) * groups + k_begin / DTA_W8_GROUP) * 16 + 4 * fq;

  // B fragment of MFMA d: token ft, chunk 4 fq + d of the group's 16, XOR-ed
  // with the token; + 256 B per group of the stage
  int b_rd[4];
#pragma unroll
  for (int d = 0; d < 4; ++d)
    b_rd[d] = ft * W4_ROW_BYTES + (((4 * fq + d) ^ ft) << 4);

  i32x4 cw[W4_DEPTH];
  f32x4 sc[W4_DEPTH];
  // g is clamped to the slice: the refills past its end re-read the last
  // group (from cache) and are never consumed, which keeps a slot's compute
  // and refill one straight-line block
  auto wload = [&](int slot, int g) __attribute__((always_inline)) {
    g = g < ngs ? g : ngs - 1;
    cw[slot] = *reinterpret_cast<const i32x4*>(cp + int64_t(g) * 1024);
    sc[slot] = *reinterpret_cast<const f32x4*>(sp + int64_t(g) * 16);
  };

  // the offset fragment: -136 (0xC308) in every element, 0x4300 | u being
  // 128 + 8 + q
  union { i32x4 i; bf16x8 b; } cu;
  cu.i = i32x4{int(0xC308C308u), int(0xC308C308u), int(0xC308C308u),
               int(0xC308C308u)};
  const bf16x8 coff = cu.b;

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (active && ngs > 0) {
#pragma unroll
    for (int i = 0; i < W4_DEPTH; ++i) wload(i, i);
  }

  // rows >= M of the stage are zero for the whole kernel
#pragma unroll 1
  for (int i = tid; i < (16 - M) * (W4_ROW_BYTES / 16); i += W4_THREADS)
    *reinterpret_cast<i32x4*>(xs + M * W4_ROW_BYTES + i * 16) =
        i32x4{0, 0, 0, 0};

  for (int g0 = 0; g0 < ngs; g0 += W4_SG) {     // block-uniform
    const int gn = ngs - g0 < W4_SG ? ngs - g0 : W4_SG;
    const int cpr = gn * (DTA_W8_GROUP / 8);    // 16 B chunks per row
    if (g0) __syncthreads();   // the previous stage has been read
    const ushort* xk = x + k_begin + g0 * DTA_W8_GROUP;
#pragma unroll 2
    for (int i = tid; i < M * cpr; i += W4_THREADS) {
      const int t = i / cpr, c = i - t * cpr;
      *reinterpret_cast<s16x8*>(xs + t * W4_ROW_BYTES + ((c ^ t) << 4)) =
          *reinterpret_cast<const s16x8*>(xk + int64_t(t) * K + c * 8);
    }
    __syncthreads();
    if (!active) continue;     // wave-uniform; the barriers are above
    // One turn of the ring, straight-line: with a branch per slot the
    // compiler has to assume the slot's loads are the youngest in flight and
    // drains the ring before every group. The groups past a ragged stage's
    // end run their MFMAs on stale LDS and drop the result (i * 256 stays
    // inside the row).
#pragma unroll
    for (int i = 0; i < W4_DEPTH; ++i) {
      const bool valid = i < gn;           // wave-uniform
      f32x4 ga = {0.f, 0.f, 0.f, 0.f}, go = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        int w = cw[i][d];
        // opaque here: the shifts must not move up to the load, which would
        // wait for it where it is issued
        asm volatile("" : "+v"(w));
        const bf16x8 a = nibbles_to_bf16(unsigned(w));
        const bf16x8 b = as_bf16x8(
            *reinterpret_cast<const s16x8*>(xs + b_rd[d] + i * 256));
        ga = mfma_bf16(a, b, ga);
        go = mfma_bf16(coff, b, go);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        acc[r] = valid ? __builtin_fmaf(sc[i][r], ga[r] + go[r], acc[r])
                       : acc[r];
      // the slot's scales are consumed before its refill is issued, so the
      // refill lands in the ring registers themselves
      __builtin_amdgcn_sched_barrier(0);
      wload(i, g0 + i + W4_DEPTH);
    }
  }

  // D[row][token]: token ft, rows n0 .. n0 + 3
  const int n0 = tile * 16 + 4 * fq;
  if (!active || ft >= M || n0 >= N) return;   // no barrier below
  if (SPLIT) {
    float* p = part + (int64_t(blockIdx.y) * M + ft) * N + n0;
    if ((N & 3) == 0) {
      *reinterpret_cast<f32x4*>(p) = acc;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n0 + r < N) p[r] = acc[r];
    }
  } else {
    ushort* o = y + int64_t(ft) * N + n0;
    s16x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float bv = (bias && n0 + r < N) ? bf2f(bias[n0 + r]) : 0.f;
      v[r] = short(f2bf(acc[r] + bv));
    }
    if ((N & 3) == 0) {
      *reinterpret_cast<s16x4*>(o) = v;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n0 + r < N) o[r] = ushort(v[r]);
    }
  }
}

// packed codes + scales -> dense bf16 [N, K]: one lane per 16 B of codes, the
// 32 columns of its quarter of a group, 64 B of output
__global__ __launch_bounds__(256)
__attribute__((target("no-packed-fp32-ops")))
void w4_dequant_k(const unsigned char* __restrict__ codes,
                  const float* __restrict__ scales, ushort* __restrict__ w,
                  int N, int K, int64_t nvec) {
  const int groups = K / DTA_W8_GROUP;
  for (int64_t v = int64_t(blockIdx.x) * 256 + threadIdx.x; v < nvec;
       v += int64_t(gridDim.x) * 256) {
    const int l = int(v & 63);
    const int64_t tg = v >> 6;                 // tile * groups + group
    const int64_t tile = tg / groups;
    const int g = int(tg - tile * groups);
    const int64_t row = tile * 16 + (l & 15);
    if (row >= N) continue;
    const i32x4 c = *reinterpret_cast<const i32x4*>(codes + v * 16);
    const float s = scales[tg * 16 + (l & 15)];
    ushort* o = w + row * K + g * DTA_W8_GROUP + 32 * (l >> 4);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const unsigned dw = unsigned(c[d]);
      s16x8 out;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int u = int((dw >> (4 * ((e >> 1) + 4 * (e & 1)))) & 15u);
        out[e] = short(f2bf(float(u - 8) * s));
      }
      *reinterpret_cast<s16x8*>(o + 8 * d) = out;
    }
  }
}

}  // namespace

void launch_w4_gemv(const W8GemvArgs& a, hipStream_t s) {
  const int groups = a.K / DTA_W8_GROUP;
  const int per = (groups + a.nsplit - 1) / a.nsplit;
  const dim3 grid(unsigned((a.N + DTA_W8_ROWS - 1) / DTA_W8_ROWS),
                  unsigned(a.nsplit));
  const unsigned char* codes = static_cast<const unsigned char*>(a.codes);
  if (a.nsplit == 1) {
    w4_gemv_k<false><<<grid, W4_THREADS, 0, s>>>(
        a.x, codes, a.scales, a.bias, a.y, nullptr, a.M, a.N, a.K,
        per * DTA_W8_GROUP);
    return;
  }
  w4_gemv_k<true><<<grid, W4_THREADS, 0, s>>>(
      a.x, codes, a.scales, nullptr, nullptr, a.part, a.M, a.N, a.K,
      per * DTA_W8_GROUP);
  launch_w8_fold(a.part, a.bias, a.y, a.nsplit, int64_t(a.M) * a.N, a.N, s);
}

void launch_w4_dequant(const unsigned char* codes, const float* scales,
                       bf16_t* w, int N, int K, hipStream_t s) {
  const int64_t nvec = int64_t((N + 15) / 16) * (K / DTA_W8_GROUP) * 64;
  w4_dequant_k<<<elementwise_grid(nvec, 256, 1), 256, 0, s>>>(
      codes, scales, w, N, K, nvec);
}
