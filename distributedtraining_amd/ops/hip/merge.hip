// Averager merge plane: fused multi-source weighted merge and the
// meta-gradient (grad_W) segmented reduction.
//
// Reference semantics being fused (averaging_logic.py):
//   merged[e]  = sum_i W[i, seg(e)] * (base[e] + delta_i[e])   (:422-470)
//   grad_W[i,j]= sum_{e in seg j} g[e] * (base[e]+delta_i[e]-merged[e])
//                                                              (:512-522)
//                formed as (base[e] - merged[e]) + delta_i[e], see grad_w_k
// The reference re-loads every miner model from disk per batch; here all
// deltas are HBM-resident and each pass streams them once. They stay in the
// form they were gathered in: [N, P] fp32, [N, P] bf16, or blockwise int8
// ([N, nb*block] codes + [N, nb] fp32 scales). One loader (delta_at) turns
// any of the three into fp32 values in registers, so the packed forms are
// bit-identical to the fp32 kernels run on the dequantised rows: bf16 -> fp32
// is exact and int8 is float(q) * scale as ONE rounded fp32 multiply, never
// contracted into the add that follows.
//
// seg(e) is found by binary search over the LDS-cached offsets table
// (param-tensor boundaries; ~dozens to a few hundred entries).
//
// delta_quantize_int8_k makes the int8 form: one workgroup per quantisation
// block, w and base read once, the fp32 delta never written.
#include "dta_common.h"
#include "dta_kernels.h"

namespace {

constexpr int MAX_SEGS = 1024;   // parameter tensors per model (GPT-2: 75)
constexpr int MAX_MODELS = DTA_MERGE_MAX_MODELS;   // miners per node

DEV int find_seg(const int64_t* offs, int n_segs, int64_t e) {
  int lo = 0, hi = n_segs;  // invariant: offs[lo] <= e < offs[hi]
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (e < offs[mid]) hi = mid; else lo = mid;
  }
  return lo;
}

// a * b rounded to fp32 on its own. hipcc contracts across statements by
// default, and its __fmul_rn is a plain `x * y` in a header compiled with
// that default: v_pk_fma_f32 swallowed the product into the caller's
// base + delta. The pragma covers the multiply written HERE.
DEV float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// ---- delta storage ---------------------------------------------------------
// KIND is a DeltaKind (dta_kernels.h); the view itself is PackedView.
// delta_at<KIND, V>(d, i, e, out): V consecutive elements e.. of row i as
// fp32. V == 4 wants e % 4 == 0 and is one 8 B (bf16) or 4 B (int8) load per
// lane; the launchers pick V == 1 where a row start is not 8 B aligned
// (bf16 with P % 4 != 0). Reading past P is in bounds for int8 only (rows are
// padded to whole blocks). block % 4 == 0, so the 4 codes share one scale.
// V == 1 (grad_W, tails) loads the aligned 4 B word that holds the element
// and picks it out: never less than 4 B per lane, neighbouring lanes share
// the word. int8 rows are whole words. A bf16 word may reach into the next
// row, so WORD is for callers that know N * P is even (the last word then
// ends with the buffer); without it the element is a 2 B load. A per-lane
// choice between the two inside the loop measured 4.09 ms for grad_W
// against 1.78 ms: the branch keeps the loop's loads from overlapping.
template <int KIND, int V, bool WORD = false>
DEV void delta_at(const PackedView& d, int i, int64_t e, float (&out)[V]) {
  static_assert(V == 1 || V == 4, "one element or one vector");
  if constexpr (KIND == DELTA_F32) {
    const float* p = static_cast<const float*>(d.data) + int64_t(i) * d.ld + e;
#pragma unroll
    for (int k = 0; k < V; ++k) out[k] = p[k];
  } else if constexpr (KIND == DELTA_BF16) {
    const ushort* p =
        static_cast<const ushort*>(d.data) + int64_t(i) * d.ld + e;
    if constexpr (V == 4) {
      const s16x4 v = *reinterpret_cast<const s16x4*>(p);
#pragma unroll
      for (int k = 0; k < 4; ++k) out[k] = bf2f(ushort(v[k]));
    } else {
      if constexpr (WORD) {
        const int odd = int((int64_t(i) * d.ld + e) & 1);
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p - odd);
        out[0] = bf2f(ushort(w >> (16 * odd)));
      } else {
        out[0] = bf2f(p[0]);
      }
    }
  } else {
    const signed char* p =
        static_cast<const signed char*>(d.data) + int64_t(i) * d.ld + e;
    const float sc = d.scales[int64_t(i) * d.nb + (e >> d.shift)];
    // comm.py dequantises with a plain multiply: mul_rn, not a * b
    if constexpr (V == 4) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        out[k] = mul_rn(float(int(w << (24 - 8 * k)) >> 24), sc);
    } else {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(p - (e & 3));
      out[0] = mul_rn(float(int(w << (24 - 8 * int(e & 3))) >> 24), sc);
    }
  }
}

// The kernels take the view as plain parameters, so the two pointers keep
// __restrict__, and rebuild it first thing.
#define DELTA_PARAMS                                                        \
  const void* __restrict__ dl_data, const float* __restrict__ dl_scales,    \
      int64_t dl_ld, int64_t dl_nb, int dl_shift
#define DELTA_ARGS(d) (d).data, (d).scales, (d).ld, (d).nb, (d).shift
#define DELTA_VIEW(name)                                                    \
  const PackedView name{dl_data, dl_scales, dl_ld, dl_nb, dl_shift, KIND}

// one pass over P; W cached in LDS ([N,S] fp32, N*S <= 32K floats).
// V elements per lane and iteration; a vector may straddle a segment
// boundary, so seg is looked up per element there.
template <int KIND, int V>
__global__ void weighted_merge_k(const float* __restrict__ base,
                                 DELTA_PARAMS,
                                 const float* __restrict__ W,
                                 const int64_t* __restrict__ offsets,
                                 int n_models, int n_segs, int64_t P,
                                 float* __restrict__ out) {
  DELTA_VIEW(deltas);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int64_t* s_off = reinterpret_cast<int64_t*>(smem);
  float* s_w = reinterpret_cast<float*>(smem + (n_segs + 1) * sizeof(int64_t)
                                        + ((n_segs + 1) & 1) * 8);
  for (int i = threadIdx.x; i <= n_segs; i += blockDim.x)
    s_off[i] = offsets[i];
  for (int i = threadIdx.x; i < n_models * n_segs; i += blockDim.x)
    s_w[i] = W[i];
  __syncthreads();

  int64_t e = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * V;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x * V;
  for (; e < P; e += stride) {
    // elements of this vector inside the plane (the last one may be cut)
    const int n = (V == 1 || e + V <= P) ? V : int(P - e);
    int seg[V];
    float b[V], acc[V];
    seg[0] = find_seg(s_off, n_segs, e);
#pragma unroll
    for (int k = 1; k < V; ++k)
      seg[k] = (e + k < s_off[seg[k - 1] + 1])
                   ? seg[k - 1] : find_seg(s_off, n_segs, e + k);
    if (V == 4 && n == 4) {
      const f32x4 vb = *reinterpret_cast<const f32x4*>(base + e);
#pragma unroll
      for (int k = 0; k < V; ++k) b[k] = vb[k];
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) b[k] = k < n ? base[e + k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    for (int i = 0; i < n_models; ++i) {
      float d[V];
      delta_at<KIND, V>(deltas, i, e, d);
#pragma unroll
      for (int k = 0; k < V; ++k)
        acc[k] = fmaf(s_w[i * n_segs + seg[k]], b[k] + d[k], acc[k]);
    }
    if (V == 4 && n == 4) {
      *reinterpret_cast<f32x4*>(out + e) =
          f32x4{acc[0], acc[1], acc[2], acc[3]};
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (k < n) out[e + k] = acc[k];
    }
  }
}

// grad_W: grid = (chunks, n_models); each block reduces one aligned chunk
// (single segment) for one miner, then one atomicAdd into grad_w[i, seg].
// chunks: [n_chunks, 3] int64 rows (start, end, seg) built host-side from
// the offsets so no chunk crosses a segment boundary.
// Lane t sums elements start + t, start + t + 256, ... in that order, for
// every storage, so grad_W of packed deltas is bit-identical to the fp32
// kernel on the dequantised rows. The delta is read an element per lane like
// g, base and merged (delta_at<KIND, 1>). A variant that loaded whole vectors
// per lane and handed the elements round through LDS, to keep this order,
// measured 2.19 ms against 1.72 ms for this one and 1.92 ms for fp32
// (profiles/r05_packed_merge.md): the barrier per tile cost more than the
// three quarters of the delta loads it saved, next to three other loads per
// element.
constexpr int GW_THREADS = 256;

template <bool G_BF16, int KIND, bool WORD = false>
__global__ void grad_w_k(const void* __restrict__ gp,
                         const float* __restrict__ base,
                         DELTA_PARAMS,
                         const float* __restrict__ merged,
                         const int64_t* __restrict__ chunks, int n_segs,
                         int64_t P, float* __restrict__ grad_w) {
  DELTA_VIEW(deltas);
  __shared__ float lds[16];
  const int64_t start = chunks[blockIdx.x * 3 + 0];
  const int64_t end = chunks[blockIdx.x * 3 + 1];
  const int seg = int(chunks[blockIdx.x * 3 + 2]);
  const int i = blockIdx.y;
  float acc = 0.f;
  for (int64_t e = start + threadIdx.x; e < end; e += blockDim.x) {
    float g = G_BF16 ? bf2f(reinterpret_cast<const ushort*>(gp)[e])
                     : reinterpret_cast<const float*>(gp)[e];
    float d[1];
    delta_at<KIND, 1, WORD>(deltas, i, e, d);
    // (base - merged) first: with W near 1/N merged is base + mean delta, so
    // that difference is exact and the sum rounds at an ulp of delta.
    // (base + d) - merged rounds at an ulp of BASE, 6e-8 |base| / |delta|
    // of the term (measured: docs/test_accuracy.md).
    acc = fmaf(g, (base[e] - merged[e]) + d[0], acc);
  }
  acc = block_sum<16>(acc, lds);
  if (threadIdx.x == 0) atomicAdd(grad_w + int64_t(i) * n_segs + seg, acc);
}

// w += alpha * dequant(row i): the validator's theta += delta_i without an
// fp32 copy of the delta. Same fmaf as axpy_k.
template <int KIND, int V>
__global__ void axpy_packed_k(float* __restrict__ w, DELTA_PARAMS, int row,
                              float alpha, int64_t P) {
  DELTA_VIEW(deltas);
  int64_t e = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * V;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x * V;
  for (; e < P; e += stride) {
    float d[V];
    if (V == 4 && e + 4 <= P) {
      delta_at<KIND, V>(deltas, row, e, d);
      const f32x4 a = *reinterpret_cast<const f32x4*>(w + e);
      *reinterpret_cast<f32x4*>(w + e) =
          f32x4{fmaf(alpha, d[0], a[0]), fmaf(alpha, d[1], a[1]),
                fmaf(alpha, d[2], a[2]), fmaf(alpha, d[3], a[3])};
    } else {
      for (int64_t t = e; t < P && t < e + V; ++t) {
        float d1[1];
        delta_at<KIND, 1>(deltas, row, t, d1);
        w[t] = fmaf(alpha, d1[0], w[t]);
      }
    }
  }
}

// ---- blockwise int8 quantiser ----------------------------------------------
// codes/scales of d = w - base (or of x alone, base == nullptr), equal bit
// for bit to comm.quantize_blockwise_int8 on the CPU:
//   scale = max(absmax / 127, 1e-12), q = clamp(rint(d / scale), -127, 127)
// with IEEE fp32 divisions and rint to even. One workgroup per block, 16
// elements per lane (64 B in, one 16 B store of codes out); elements past P
// count as 0 and the tail block still gets all its codes. The absmax is
// reduced on the BIT PATTERNS of |d|: for non-negative floats unsigned order
// is float order and every NaN sorts above +inf, so a NaN anywhere in the
// block reaches the scale, as torch.amax does (fmaxf would drop it). No
// early return: every lane reaches the barrier.
constexpr int QUANT_PER_LANE = 16;

__global__ void delta_quantize_int8_k(const float* __restrict__ w,
                                      const float* __restrict__ base,
                                      int64_t P, int block,
                                      signed char* __restrict__ codes,
                                      float* __restrict__ scales) {
  __shared__ uint32_t lds[16];
  const int64_t blk0 = int64_t(blockIdx.x) * block;
  const int off = int(threadIdx.x) * QUANT_PER_LANE;
  const bool active = off < block;      // block 256: 16 of the 64 lanes
  const int64_t e0 = blk0 + off;
  float d[QUANT_PER_LANE];
  if (active && e0 + QUANT_PER_LANE <= P) {
#pragma unroll
    for (int v = 0; v < QUANT_PER_LANE / 4; ++v) {
      f32x4 a = *reinterpret_cast<const f32x4*>(w + e0 + 4 * v);
      if (base != nullptr) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(base + e0 + 4 * v);
        a = f32x4{a[0] - b[0], a[1] - b[1], a[2] - b[2], a[3] - b[3]};
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) d[4 * v + k] = a[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < QUANT_PER_LANE; ++k) {
      const int64_t e = e0 + k;
      float a = 0.f;
      if (active && e < P) a = base != nullptr ? w[e] - base[e] : w[e];
      d[k] = a;
    }
  }
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < QUANT_PER_LANE; ++k) {
    const uint32_t bits = __float_as_uint(fabsf(d[k]));
    m = bits > m ? bits : m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t other = uint32_t(__shfl_xor(int(m), o));
    m = other > m ? other : m;
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nw = (blockDim.x + 63) >> 6;
  if (lane == 0) lds[wid] = m;
  __syncthreads();
  m = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (k < nw) m = lds[k] > m ? lds[k] : m;
  const float absmax = __uint_as_float(m);
  // clamp_min keeps a NaN (torch.clamp does); a < on NaN is false
  float scale = __fdiv_rn(absmax, 127.0f);
  if (scale < 1e-12f) scale = 1e-12f;
  if (threadIdx.x == 0) scales[blockIdx.x] = scale;
  if (active) {
    uint32_t pk[QUANT_PER_LANE / 4];
#pragma unroll
    for (int v = 0; v < QUANT_PER_LANE / 4; ++v) {
      uint32_t word = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float r = rintf(__fdiv_rn(d[4 * v + k], scale));
        r = fminf(fmaxf(r, -127.0f), 127.0f);
        // NaN (poisoned block, or inf / inf): code 0
        const int q = (r != r) ? 0 : int(r);
        word |= (uint32_t(q) & 0xFFu) << (8 * k);
      }
      pk[v] = word;
    }
    typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
    *reinterpret_cast<u32x4*>(codes + e0) = u32x4{pk[0], pk[1], pk[2], pk[3]};
  }
}

size_t merge_shmem(int n_models, int n_segs) {
  return (n_segs + 1) * sizeof(int64_t) + 8 +
         size_t(n_models) * n_segs * sizeof(float);
}

// V == 4 needs every row start 8 B aligned; int8 rows are whole blocks
bool packed_vec4(const PackedView& d, int64_t P) {
  return d.kind == DELTA_I8 || P % 4 == 0;
}

}  // namespace

size_t dta_merge_shmem(int n_models, int n_segs) {
  return merge_shmem(n_models, n_segs);
}

void launch_weighted_merge(const float* base, const float* deltas,
                           const float* W, const int64_t* offsets,
                           int n_models, int n_segs, int64_t P, float* out,
                           hipStream_t s) {
  const int block = 256;
  const int grid = elementwise_grid(P, block, 1);
  const PackedView d{deltas, nullptr, P, 0, 0, DELTA_F32};
  weighted_merge_k<DELTA_F32, 1>
      <<<grid, block, merge_shmem(n_models, n_segs), s>>>(
          base, DELTA_ARGS(d), W, offsets, n_models, n_segs, P, out);
}

void launch_weighted_merge_packed(const float* base, const PackedView& d,
                                  const float* W, const int64_t* offsets,
                                  int n_models, int n_segs, int64_t P,
                                  float* out, hipStream_t s) {
  const int block = 256;
  const size_t shmem = merge_shmem(n_models, n_segs);
  const bool v4 = packed_vec4(d, P);
  const int grid = elementwise_grid(P, block, v4 ? 4 : 1);
#define MERGE_GO(KIND, V)                                                   \
  weighted_merge_k<KIND, V><<<grid, block, shmem, s>>>(                     \
      base, DELTA_ARGS(d), W, offsets, n_models, n_segs, P, out)
  if (d.kind == DELTA_I8) MERGE_GO(DELTA_I8, 4);
  else if (v4) MERGE_GO(DELTA_BF16, 4);
  else MERGE_GO(DELTA_BF16, 1);
#undef MERGE_GO
}

void launch_grad_merge_weights(const void* g, bool g_is_bf16,
                               const float* base, const float* deltas,
                               const float* merged, const int64_t* chunks,
                               int n_models, int n_chunks, int64_t P,
                               float* grad_w, int n_segs, hipStream_t s) {
  dim3 grid(n_chunks, n_models);
  const PackedView d{deltas, nullptr, P, 0, 0, DELTA_F32};
  if (g_is_bf16)
    grad_w_k<true, DELTA_F32><<<grid, GW_THREADS, 0, s>>>(
        g, base, DELTA_ARGS(d), merged, chunks, n_segs, P, grad_w);
  else
    grad_w_k<false, DELTA_F32><<<grid, GW_THREADS, 0, s>>>(
        g, base, DELTA_ARGS(d), merged, chunks, n_segs, P, grad_w);
}

void launch_grad_merge_weights_packed(const void* g, bool g_is_bf16,
                                      const float* base, const PackedView& d,
                                      const float* merged,
                                      const int64_t* chunks, int n_models,
                                      int n_chunks, int64_t P, float* grad_w,
                                      int n_segs, hipStream_t s) {
  dim3 grid(n_chunks, n_models);
#define GRADW_GO(GB, KIND, WORD)                                            \
  grad_w_k<GB, KIND, WORD><<<grid, GW_THREADS, 0, s>>>(                     \
      g, base, DELTA_ARGS(d), merged, chunks, n_segs, P, grad_w)
  if (d.kind == DELTA_I8) {
    if (g_is_bf16) GRADW_GO(true, DELTA_I8, true);
    else GRADW_GO(false, DELTA_I8, true);
  } else if ((int64_t(n_models) * P) % 2 == 0) {   // see delta_at
    if (g_is_bf16) GRADW_GO(true, DELTA_BF16, true);
    else GRADW_GO(false, DELTA_BF16, true);
  } else {
    if (g_is_bf16) GRADW_GO(true, DELTA_BF16, false);
    else GRADW_GO(false, DELTA_BF16, false);
  }
#undef GRADW_GO
}

void launch_axpy_packed(float* w, const PackedView& d, int row, float alpha,
                        int64_t P, hipStream_t s) {
  const int block = 256;
  const bool v4 = packed_vec4(d, P);
  const int grid = elementwise_grid(P, block, v4 ? 4 : 1);
  if (d.kind == DELTA_I8)
    axpy_packed_k<DELTA_I8, 4><<<grid, block, 0, s>>>(
        w, DELTA_ARGS(d), row, alpha, P);
  else if (v4)
    axpy_packed_k<DELTA_BF16, 4><<<grid, block, 0, s>>>(
        w, DELTA_ARGS(d), row, alpha, P);
  else
    axpy_packed_k<DELTA_BF16, 1><<<grid, block, 0, s>>>(
        w, DELTA_ARGS(d), row, alpha, P);
}

void launch_delta_quantize_int8(const float* w, const float* base, int64_t P,
                                int block, int64_t nb, signed char* codes,
                                float* scales, hipStream_t s) {
  int threads = (block / QUANT_PER_LANE + 63) / 64 * 64;
  if (threads < 64) threads = 64;
  delta_quantize_int8_k<<<unsigned(nb), threads, 0, s>>>(w, base, P, block,
                                                         codes, scales);
}
