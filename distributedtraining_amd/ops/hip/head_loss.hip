// Fused LM-head loss, forward only: logits = x @ Wᵀ on the MFMA units with
// every finished accumulator tile folded straight into an online
// log-sum-exp — the [T, V] logits never exist in memory. For the no-grad
// consumers (validator scoring, cached base loss, sharded validation) that
// need only the scalar loss; training still goes through lm_head_ce
// (backward needs the logits).
//
// Shapes: x [T, K] bf16, w [V, K] bf16 (the tied embedding as stored),
// both row-contiguous and 16 B aligned, K % 64 == 0 (no BK = 32 tail);
// targets [T] int64. Checked at the binding.
//
// Structure:
//   * block = 256 threads (4 waves, 2 vocab x 2 token), tile 128 tokens x
//     128 vocab, BK = 64, two LDS buffers, ONE barrier per K-step: the
//     global loads of step i+1 are issued before the MFMAs of step i and
//     written to the other buffer after them. The (vocab tile, k) loop is
//     flattened so the prefetch also runs across the epilogue.
//   * swapped product as in attention.hip: A = W tile, B = x tile, so
//     D[vocab][token] puts one token on a lane (col = lane&15) with 4 vocab
//     entries per fragment in its registers (row = 4*(lane>>4)+reg). Both
//     fragments are single 16 B LDS reads of a K-contiguous row.
//   * LDS image: unpadded [128][64] bf16 per operand (128 B rows) with the
//     16 B chunk XOR-swizzled by (row>>1)&7 — each ds_read_b128 lane group
//     (MI355X: {0-3,12-15,20-27}, ...) then covers 16 distinct 16 B slots of
//     the 256 B bank row, and the 8 lanes that stage one row write one full
//     128 B line.
//   * epilogue per tile, in exp2 units as ce.hip: columns >= V -> -inf, the
//     target column's UNSCALED fp32 accumulator goes to tlogit[row] (one
//     writer per row), every lane keeps its own running (m, s) for its 4
//     tokens over the vocab entries it sees. Nothing is rounded to bf16.
//   * grid = (ceil(T/128), nsplit): a block walks the vocab tiles of its
//     split; at the end lanes sharing a token fold with two shfl_xor steps,
//     the two waves sharing a row combine through LDS, and one partial
//     (m, s) per (split, row) goes to a [nsplit, T] fp32 workspace. A small
//     merge kernel folds the splits of each row in fixed order — no float
//     atomics on (m, s), so per-row results are bit-reproducible.
//   * rows >= T: clamped loads, no writes. All row offsets are int64.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   head_loss_k: 176 VGPRs, 0 AGPRs, 69 SGPRs, nothing spilled, no scratch,
//   65536 B LDS, occupancy 2 waves/SIMD = 2 blocks/CU (both the register
//   and the LDS limit). Without the launch bound's second argument hipcc
//   takes 176 + 88 AGPRs and drops to 1 wave/SIMD.
//   128x128 needs 64 KB for two buffers; a 256-wide tile would leave one
//   block per CU, which the plain one-barrier loop cannot keep busy.
#include "dta_common.h"
#include "dta_kernels.h"

namespace {

constexpr int HL_BM = DTA_HEAD_LOSS_TILE;  // tokens per block
constexpr int HL_BN = DTA_HEAD_LOSS_TILE;  // vocab entries per tile
constexpr int HL_BK = 64;
constexpr int HL_THREADS = 256;
constexpr int HL_TILE = 128 * HL_BK;       // bf16 elements per operand tile
constexpr int HL_BUF = 2 * HL_TILE;        // W tile + x tile

static_assert(HL_BM == 128 && HL_BN == 128, "wave layout assumes 128x128");

// element offset of 16 B chunk c (0..7) of row r in a swizzled [128][64] tile
DEV int hl_off(int r, int c) { return r * HL_BK + ((c ^ ((r >> 1) & 7)) << 3); }

DEV bf16x8 hl_frag(const ushort* tile, int r, int c) {
  return as_bf16x8(*reinterpret_cast<const s16x8*>(tile + hl_off(r, c)));
}

// (m, s) <- (m, s) (+) (m2, s2) in exp2 units. An all -inf side (a lane that
// has seen only masked tail columns) contributes exactly 0, never NaN.
DEV void hl_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  const float mu = (mn == -INFINITY) ? 0.f : mn;
  s = s * __builtin_exp2f(m - mu) + s2 * __builtin_exp2f(m2 - mu);
  m = mn;
}

__global__ __launch_bounds__(HL_THREADS, 2) void head_loss_k(
    const ushort* __restrict__ x, const ushort* __restrict__ w,
    const int64_t* __restrict__ targets, int64_t T, int64_t V, int K,
    int ntiles, float* __restrict__ ws_m, float* __restrict__ ws_s,
    float* __restrict__ tlogit) {
  // single LDS object: staging buffers, reused for the cross-wave combine
  __shared__ __attribute__((aligned(16))) ushort lds[2 * HL_BUF];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int wv = wid >> 1, wt = wid & 1;  // wave's vocab / token half
  const int fr = lane & 15, fq = lane >> 4;
  const int64_t m0 = int64_t(blockIdx.x) * HL_BM;
  const int nsplit = gridDim.y, split = blockIdx.y;
  const int t_begin = int(int64_t(split) * ntiles / nsplit);
  const int t_end = int(int64_t(split + 1) * ntiles / nsplit);
  const int nk = K / HL_BK;
  const int total = (t_end - t_begin) * nk;

  // staging: thread -> 16 B chunk sc of rows sr + 32p (p = 0..3)
  const int sc = tid & 7, sr = tid >> 3;
  const int st_off = hl_off(sr, sc);  // (row+32p)>>1 & 7 == (row>>1) & 7
  const ushort* xp[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int64_t r = m0 + sr + 32 * p;
    xp[p] = x + (r < T ? r : T - 1) * int64_t(K) + sc * 8;
  }

  // this lane's 4 tokens: block row wt*64 + 16n + fr
  int tg[4];
  float m_l[4], s_l[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int64_t r = m0 + wt * 64 + n * 16 + fr;
    const int64_t t = targets[r < T ? r : T - 1];
    tg[n] = (r < T && t >= 0 && t < V) ? int(t) : -1;
    m_l[n] = -INFINITY;
    s_l[n] = 0.f;
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  s16x8 gw[4], gx[4];
  int tile = t_begin, ks = 0;  // (tile, k-step) of the NEXT load

  auto gload = [&]() {
    const int64_t v0 = int64_t(tile) * HL_BN;
    const int k0 = ks * HL_BK;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int64_t wr = v0 + sr + 32 * p;
      gw[p] = *reinterpret_cast<const s16x8*>(
          w + (wr < V ? wr : V - 1) * int64_t(K) + k0 + sc * 8);
      gx[p] = *reinterpret_cast<const s16x8*>(xp[p] + k0);
    }
    if (++ks == nk) { ks = 0; ++tile; }
  };
  auto lds_write = [&](ushort* buf) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      *reinterpret_cast<s16x8*>(buf + st_off + p * 32 * HL_BK) = gw[p];
      *reinterpret_cast<s16x8*>(buf + HL_TILE + st_off + p * 32 * HL_BK) =
          gx[p];
    }
  };

  gload();
  lds_write(lds);
  __syncthreads();

  int ctile = t_begin, cks = 0;  // (tile, k-step) being computed
  for (int it = 0; it < total; ++it) {
    const bool more = it + 1 < total;  // block-uniform
    if (more) gload();

    const ushort* wb = lds + (it & 1) * HL_BUF;
    const ushort* xb = wb + HL_TILE;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = hl_frag(wb, wv * 64 + i * 16 + fr, kk * 4 + fq);
        b[i] = hl_frag(xb, wt * 64 + i * 16 + fr, kk * 4 + fq);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[i][n] = mfma_bf16(a[i], b[n], acc[i][n]);
    }

    if (++cks == nk) {
      // ---- epilogue: fold the finished 128x128 tile into (m, s) ----------
      const int64_t v0 = int64_t(ctile) * HL_BN;
      const int cbase = int(v0) + wv * 64 + 4 * fq;  // V < 2^31
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        float f[16];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int col = cbase + i * 16 + r;
            const float a = acc[i][n][r];
            if (col == tg[n])  // tg < V, and -1 for ignored / tail rows
              tlogit[m0 + wt * 64 + n * 16 + fr] = a;
            const float v = (col < V) ? a * LOG2E : -INFINITY;
            f[i * 4 + r] = v;
            mx = fmaxf(mx, v);
            acc[i][n][r] = 0.f;
          }
        const float mn = fmaxf(m_l[n], mx);
        const float mu = (mn == -INFINITY) ? 0.f : mn;
        float ps = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) ps += __builtin_exp2f(f[j] - mu);
        s_l[n] = s_l[n] * __builtin_exp2f(m_l[n] - mu) + ps;
        m_l[n] = mn;
      }
      cks = 0;
      ++ctile;
    }

    if (more) lds_write(lds + ((it + 1) & 1) * HL_BUF);
    __syncthreads();
  }

  // ---- lanes sharing a token (same fr): two cross-lane steps --------------
#pragma unroll
  for (int n = 0; n < 4; ++n) {
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
      const float mo = __shfl_xor(m_l[n], off);
      const float so = __shfl_xor(s_l[n], off);
      hl_merge(m_l[n], s_l[n], mo, so);
    }
  }
  // ---- the two waves sharing a row combine through LDS (the loop's last
  // barrier has retired every staging read) ---------------------------------
  float* red = reinterpret_cast<float*>(lds);  // [2 wv][2 (m,s)][128 rows]
  if (fq == 0) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int r = wt * 64 + n * 16 + fr;
      red[(wv * 2 + 0) * HL_BM + r] = m_l[n];
      red[(wv * 2 + 1) * HL_BM + r] = s_l[n];
    }
  }
  __syncthreads();
  if (tid < HL_BM) {
    const int64_t row = m0 + tid;
    if (row < T) {
      float m = red[0 * HL_BM + tid], s = red[1 * HL_BM + tid];
      hl_merge(m, s, red[2 * HL_BM + tid], red[3 * HL_BM + tid]);
      ws_m[int64_t(split) * T + row] = m;
      ws_s[int64_t(split) * T + row] = s;
    }
  }
}

// fold the splits of each row in fixed order (bit-reproducible)
__global__ void head_loss_merge_k(const float* __restrict__ ws_m,
                                  const float* __restrict__ ws_s, int nsplit,
                                  int64_t T, float* __restrict__ m_run,
                                  float* __restrict__ s_run) {
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < T;
       t += int64_t(gridDim.x) * blockDim.x) {
    float m = ws_m[t], s = ws_s[t];
    for (int sp = 1; sp < nsplit; ++sp)
      hl_merge(m, s, ws_m[int64_t(sp) * T + t], ws_s[int64_t(sp) * T + t]);
    m_run[t] = m;
    s_run[t] = s;
  }
}

}  // namespace

void launch_head_loss(const bf16_t* x, const bf16_t* w,
                      const int64_t* targets, int64_t T, int64_t V, int K,
                      int nsplit, float* ws_m, float* ws_s, float* tlogit,
                      float* m_run, float* s_run, hipStream_t s) {
  const int ntiles = int((V + HL_BN - 1) / HL_BN);
  const dim3 grid((unsigned)((T + HL_BM - 1) / HL_BM), (unsigned)nsplit);
  head_loss_k<<<grid, HL_THREADS, 0, s>>>(x, w, targets, T, V, K, ntiles,
                                          ws_m, ws_s, tlogit);
  head_loss_merge_k<<<elementwise_grid(T, 256, 1), 256, 0, s>>>(
      ws_m, ws_s, nsplit, T, m_run, s_run);
}
