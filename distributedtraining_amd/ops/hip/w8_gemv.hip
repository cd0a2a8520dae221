// Int8 weight-only skinny GEMM for serving decode (W8A16), 1 <= M <= 16:
//   y[M, N] = x[M, K] · Wq[N, K]^T (+ bias),  Wq[n, k] = float(q[n, k]) * s[n, k / 128]
// bf16 activations and output, int8 codes with one fp32 scale per (row, group
// of 128 along K), fp32 accumulation on mfma_f32_16x16x32_bf16, one rounding
// per output. A decode projection is a weight stream; this kernel reads half
// the bytes of the bf16 one and spends its VALU on the int8 -> bf16 convert
// only (exact: |q| <= 127 fits bf16's significand), the product runs on the
// matrix unit, so up to 16 tokens cost no extra weight traffic.
//
// Packed weight (ops/w8.py writes it once, offline; docs/serving.md):
//   rows padded with zero codes to Np = ceil16(N);
//   codes  int8 [Np/16][K/64][64][16]: the 1 KB of a (16-row tile, 64-wide
//          K-step) in lane order, lane l = row l % 16, K columns
//          16 (l / 16) .. + 15 of the step. A wave reads a contiguous KB with
//          one 16 B load per lane, and that load is the A operand of two
//          MFMAs: bytes 8 j .. 8 j + 7 are MFMA j's fragment, i.e. the MFMA's
//          k index 8 (l / 16) + e stands for column 16 (l / 16) + 8 j + e, and
//          the activation fragment below uses the same order;
//   scales fp32 [Np/16][K/128][16]: 64 B per (tile, group).
//
// Structure:
//   * block = 256 threads, 4 waves, 64 output rows (one 16-row tile per wave)
//     and one K slice (blockIdx.y, a multiple of 128 columns). The slice is
//     walked in stages of <= 1024 columns.
//   * x stage: [16 tokens][1024] bf16 = 32 KB of LDS, written once per stage
//     by the whole block (16 B chunks, rows >= M zeroed once) and read by all
//     four waves: x comes from L2 once per 64 rows. Rows are 2 KB apart, so
//     the 16 B chunk index is XOR-ed with the token: the 16 tokens of a
//     fragment read (lane: token l % 16, chunk 2 (l / 16) + j of the step's 8)
//     fall on 16 different chunks of a 256 B bank row.
//   * weights never touch LDS. Per group of 128 columns a lane issues two 16 B
//     code loads and one 16 B load of its 4 row scales (the D rows
//     4 (l / 16) .. + 3); DEPTH = 4 groups are kept in flight ahead of the
//     converts in a register ring (8 code loads + 4 scale loads per lane,
//     8 KB per wave), refilled right after a slot is consumed and running
//     across the stage barriers.
//   * swapped product as gemm.hip: A = weight tile, B = x, so D[row][token]
//     puts token l % 16 on a lane with rows 4 (l / 16) + r in its registers.
//     The 4 MFMAs of a group accumulate the integer-valued codes against x in
//     a zeroed group accumulator, then acc += scale_row * group_acc, 4 fp32
//     FMAs per lane per group. Nothing is rounded before the store.
//   * nsplit == 1: acc + bias in fp32, one bf16 rounding, direct store.
//     nsplit > 1: fp32 partials [nsplit, M, N]; w8_fold_k sums them in
//     ascending slice order, adds the bias and rounds once.
//   * every loop bound and every branch around a barrier is block-uniform; a
//     wave whose tile lies past Np skips its loads and MFMAs wave-uniformly
//     and still stages x and reaches every barrier. Rows >= N and tokens >= M
//     are never stored. No atomics, every output written once: bit-repeatable
//     and capturable.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950) are listed
// in docs/kernels.md.
#include "dta_common.h"
#include "dta_kernels.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;

constexpr int W8_THREADS = 256;
constexpr int W8_STAGE = 1024;            // x columns per LDS stage
constexpr int W8_ROW_BYTES = W8_STAGE * 2;
constexpr int W8_DEPTH = 4;               // groups in flight per lane
static_assert((W8_STAGE / DTA_W8_GROUP) % W8_DEPTH == 0,
              "a stage holds whole turns of the register ring");

// The scale FMAs and the bias add stay scalar instructions: the packed
// two-lane fp32 forms are switched off for these kernels.
template <bool SPLIT>
__global__ __launch_bounds__(W8_THREADS)
__attribute__((target("no-packed-fp32-ops")))
void w8_gemv_k(const ushort* __restrict__ x, const char* __restrict__ codes,
               const float* __restrict__ scales,
               const ushort* __restrict__ bias, ushort* __restrict__ y,
               float* __restrict__ part, int M, int N, int K, int kslice) {
  __shared__ __attribute__((aligned(16))) char xs[16 * W8_ROW_BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ft = lane & 15, fq = lane >> 4;   // token / row, K quarter

  const int tiles = (N + 15) >> 4;
  const int tile = blockIdx.x * 4 + wid;
  const bool active = tile < tiles;           // wave-uniform
  const int k_begin = blockIdx.y * kslice;
  const int k_end = k_begin + kslice < K ? k_begin + kslice : K;
  const int ngs = k_end > k_begin ? (k_end - k_begin) / DTA_W8_GROUP : 0;

  // this lane's 16 B of K-step 0 of the slice; + 1 KB per K-step
  const char* cp = codes + (int64_t(tile) * (K / 64) + k_begin / 64) * 1024 +
                   lane * 16;
  // its 4 row scales of group 0 of the slice; + 16 floats per group
  const float* sp = scales +
                    (int64_t(tile) * (K / DTA_W8_GROUP) +
                     k_begin / DTA_W8_GROUP) * 16 + 4 * fq;

  // B fragment of K-step s, MFMA j: token ft, chunk 8 s + 2 fq + j of the
  // group's 16, XOR-ed with the token; + 256 B per group of the stage
  int b_rd[2][2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      b_rd[s][j] = ft * W8_ROW_BYTES + (((8 * s + 2 * fq + j) ^ ft) << 4);

  i32x4 cw[W8_DEPTH][2];
  f32x4 sc[W8_DEPTH];
  // g is clamped to the slice: the refills past its end re-read the last
  // group (from cache) and are never consumed, which keeps a slot's compute
  // and refill one straight-line block
  auto wload = [&](int slot, int g) __attribute__((always_inline)) {
    g = g < ngs ? g : ngs - 1;
    cw[slot][0] = *reinterpret_cast<const i32x4*>(cp + int64_t(g) * 2048);
    cw[slot][1] =
        *reinterpret_cast<const i32x4*>(cp + int64_t(g) * 2048 + 1024);
    sc[slot] = *reinterpret_cast<const f32x4*>(sp + int64_t(g) * 16);
  };

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (active && ngs > 0) {
#pragma unroll
    for (int i = 0; i < W8_DEPTH; ++i) wload(i, i);
  }

  // rows >= M of the stage are zero for the whole kernel
#pragma unroll 1
  for (int i = tid; i < (16 - M) * (W8_ROW_BYTES / 16); i += W8_THREADS)
    *reinterpret_cast<i32x4*>(xs + M * W8_ROW_BYTES + i * 16) =
        i32x4{0, 0, 0, 0};

  constexpr int SG = W8_STAGE / DTA_W8_GROUP;   // groups per stage
  for (int g0 = 0; g0 < ngs; g0 += SG) {        // block-uniform
    const int gn = ngs - g0 < SG ? ngs - g0 : SG;
    const int cpr = gn * (DTA_W8_GROUP / 8);    // 16 B chunks per row
    if (g0) __syncthreads();   // the previous stage has been read
    const ushort* xk = x + k_begin + g0 * DTA_W8_GROUP;
#pragma unroll 2
    for (int i = tid; i < M * cpr; i += W8_THREADS) {
      const int t = i / cpr, c = i - t * cpr;
      *reinterpret_cast<s16x8*>(xs + t * W8_ROW_BYTES + ((c ^ t) << 4)) =
          *reinterpret_cast<const s16x8*>(xk + int64_t(t) * K + c * 8);
    }
    __syncthreads();
    if (!active) continue;     // wave-uniform; the barriers are above
    // One turn of the ring is straight-line code: with a branch per slot the
    // compiler has to assume the slot's loads are the youngest in flight and
    // drains the ring before every group. A ragged last turn runs its MFMAs
    // on stale LDS and drops the result (gl * 256 stays inside the row).
    for (int gb = 0; gb < gn; gb += W8_DEPTH) {
#pragma unroll
      for (int i = 0; i < W8_DEPTH; ++i) {
        const int gl = gb + i;             // group of the stage, slot i
        const bool valid = gl < gn;        // wave-uniform
        f32x4 ga = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            int lo = cw[i][s][2 * j], hi = cw[i][s][2 * j + 1];
            // opaque here: the byte extracts must not move up to the load,
            // which would wait for it where it is issued
            asm volatile("" : "+v"(lo), "+v"(hi));
            const bf16x8 a = codes_to_bf16(lo, hi);
            const bf16x8 b = as_bf16x8(*reinterpret_cast<const s16x8*>(
                xs + b_rd[s][j] + gl * 256));
            ga = mfma_bf16(a, b, ga);
          }
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[r] = valid ? __builtin_fmaf(sc[i][r], ga[r], acc[r]) : acc[r];
        // the slot's scales are consumed before its refill is issued, so the
        // refill lands in the ring registers themselves
        __builtin_amdgcn_sched_barrier(0);
        wload(i, g0 + gl + W8_DEPTH);
      }
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

// y[e] = bf16(sum over the slices in ascending order + bias), e over [M, N]
__global__ __launch_bounds__(256)
__attribute__((target("no-packed-fp32-ops")))
void w8_fold_k(const float* __restrict__ part, const ushort* __restrict__ bias,
               ushort* __restrict__ y, int nsplit, int64_t MN, int N) {
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < MN;
       e += int64_t(gridDim.x) * 256) {
    float s = part[e];
    for (int i = 1; i < nsplit; ++i) s += part[int64_t(i) * MN + e];
    if (bias) s += bf2f(bias[e % N]);
    y[e] = f2bf(s);
  }
}

// packed codes + scales -> dense bf16 [N, K]: one lane per 16 B of codes
__global__ __launch_bounds__(256)
__attribute__((target("no-packed-fp32-ops")))
void w8_dequant_k(const char* __restrict__ codes,
                  const float* __restrict__ scales, ushort* __restrict__ w,
                  int N, int K, int64_t nvec) {
  const int ksteps = K / 64;
  for (int64_t v = int64_t(blockIdx.x) * 256 + threadIdx.x; v < nvec;
       v += int64_t(gridDim.x) * 256) {
    const int l = int(v & 63);
    const int64_t tk = v >> 6;                 // tile * ksteps + kstep
    const int64_t tile = tk / ksteps;
    const int ks = int(tk - tile * ksteps);
    const int64_t row = tile * 16 + (l & 15);
    if (row >= N) continue;
    const i32x4 c = *reinterpret_cast<const i32x4*>(codes + v * 16);
    const float s =
        scales[(tile * (K / DTA_W8_GROUP) + (ks >> 1)) * 16 + (l & 15)];
    ushort* o = w + row * K + ks * 64 + 16 * (l >> 4);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      s16x8 out;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int d = c[2 * h + (e >> 2)];
        out[e] = short(
            f2bf(float(static_cast<signed char>(d >> (8 * (e & 3)))) * s));
      }
      *reinterpret_cast<s16x8*>(o + 8 * h) = out;
    }
  }
}

}  // namespace

void launch_w8_gemv(const W8GemvArgs& a, hipStream_t s) {
  const int groups = a.K / DTA_W8_GROUP;
  const int per = (groups + a.nsplit - 1) / a.nsplit;
  const dim3 grid(unsigned((a.N + DTA_W8_ROWS - 1) / DTA_W8_ROWS),
                  unsigned(a.nsplit));
  const char* codes = static_cast<const char*>(a.codes);
  if (a.nsplit == 1) {
    w8_gemv_k<false><<<grid, W8_THREADS, 0, s>>>(
        a.x, codes, a.scales, a.bias, a.y, nullptr, a.M, a.N, a.K,
        per * DTA_W8_GROUP);
    return;
  }
  w8_gemv_k<true><<<grid, W8_THREADS, 0, s>>>(
      a.x, codes, a.scales, nullptr, nullptr, a.part, a.M, a.N, a.K,
      per * DTA_W8_GROUP);
  launch_w8_fold(a.part, a.bias, a.y, a.nsplit, int64_t(a.M) * a.N, a.N, s);
}

void launch_w8_fold(const float* part, const bf16_t* bias, bf16_t* y,
                    int nsplit, int64_t MN, int N, hipStream_t s) {
  w8_fold_k<<<elementwise_grid(MN, 256, 1), 256, 0, s>>>(part, bias, y,
                                                         nsplit, MN, N);
}

void launch_w8_dequant(const signed char* codes, const float* scales,
                       bf16_t* w, int N, int K, hipStream_t s) {
  const int64_t nvec = int64_t((N + 15) / 16) * (K / 64) * 64;
  w8_dequant_k<<<elementwise_grid(nvec, 256, 1), 256, 0, s>>>(
      reinterpret_cast<const char*>(codes), scales, w, N, K, nvec);
}
