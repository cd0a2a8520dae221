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
//
// A fourth form is sparse: blockwise top-k entries (delta_topk_k makes them,
// with an error-feedback residual). delta_at cannot express it; its three
// consumers are kernels of their own further down and hold the same
// contract, the fp32 kernel's bits on the densified rows.
#include "dta_common.h"
#include "dta_kernels.h"

#include <utility>

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

// delta_at in two halves, for a kernel that issues the loads of many rows
// before it uses any of them: delta_raw only loads (the words as they are
// stored, and the scale for int8), raw_value turns element k of the vector
// into the fp32 value delta_at gives. With the conversion next to the load,
// inside a branch per row, every row's load was waited for before the next
// was issued (the robust merge ran 2 to 3 times longer on bf16 and int8).
// Alignment and bounds as for delta_at; bf16 with V == 1 is the 2 B load.
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
template <int KIND, int V> constexpr int raw_words() {
  return KIND == DELTA_F32 ? V : (KIND == DELTA_BF16 && V == 4) ? 2 : 1;
}
template <int KIND, int V>
DEV void delta_raw(const PackedView& d, int i, int64_t e,
                   uint32_t (&raw)[raw_words<KIND, V>()], float& sc) {
  static_assert(V == 1 || V == 4, "one element or one vector");
  if constexpr (KIND == DELTA_F32) {
    const float* p = static_cast<const float*>(d.data) + int64_t(i) * d.ld + e;
#pragma unroll
    for (int k = 0; k < V; ++k) raw[k] = __float_as_uint(p[k]);
  } else if constexpr (KIND == DELTA_BF16) {
    const ushort* p =
        static_cast<const ushort*>(d.data) + int64_t(i) * d.ld + e;
    if constexpr (V == 4) {
      const u32x2 v = *reinterpret_cast<const u32x2*>(p);
      raw[0] = v[0];
      raw[1] = v[1];
    } else {
      raw[0] = p[0];
    }
  } else {
    const signed char* p =
        static_cast<const signed char*>(d.data) + int64_t(i) * d.ld + e;
    sc = d.scales[int64_t(i) * d.nb + (e >> d.shift)];
    raw[0] = *reinterpret_cast<const uint32_t*>(V == 4 ? p : p - (e & 3));
  }
}
template <int KIND, int V>
DEV float raw_value(const uint32_t (&raw)[raw_words<KIND, V>()], float sc,
                    int k, int64_t e) {
  if constexpr (KIND == DELTA_F32) {
    return __uint_as_float(raw[k]);
  } else if constexpr (KIND == DELTA_BF16) {
    if constexpr (V == 4)
      return bf2f(ushort(raw[k >> 1] >> (16 * (k & 1))));
    else
      return bf2f(ushort(raw[0]));
  } else {
    const int b = V == 4 ? k : int(e & 3);
    return mul_rn(float(int(raw[0] << (24 - 8 * b)) >> 24), sc);
  }
}
// raw words and scale whose every element is a NaN
template <int KIND> DEV void raw_nan(uint32_t& word, float& sc) {
  word = KIND == DELTA_F32 ? 0x7FC00000u : KIND == DELTA_BF16 ? 0x7FC07FC0u
                                                               : 0u;
  sc = __uint_as_float(0x7FC00000u);
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

// ---- robust merge: coordinate-wise trimmed mean / median ---------------------
// out[e] = base[e] + mean of the values at sorted positions t .. N-1-t of
// delta_0[e] .. delta_{N-1}[e]; outside[i] counts the elements at which
// miner i lies strictly outside that kept interval. The definition is the
// CPU path of ops.trimmed_merge and the kernel equals it bit for bit: the
// order is taken on integer keys, the kept values are summed in ascending
// position from the first one, then one IEEE division and one add.
//
// order key of a float: flip every bit of a negative, the sign bit of the
// rest, so unsigned order is -inf < .. < -0 < +0 < .. < +inf; every NaN is
// 0xFFFFFFFF, above all of them. The pad rows N .. NP-1 get that key too:
// equal keys are the same value, so positions 0 .. N-1 of the sorted NP
// hold the sorted N whatever a tie with a pad did.
constexpr uint32_t KEY_NAN = 0xFFFFFFFFu;

DEV uint32_t order_key(float v) {
  const uint32_t b = __float_as_uint(v);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return KEY_NAN;
  return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
// KEY_NAN comes back as the NaN 0x7FFFFFFF; the kernel makes every NaN it
// stores 0x7FC00000
DEV float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// Batcher's odd-even merge sort of NP keys as a list of comparators, built
// at compile time: 5 / 19 / 63 / 191 for NP = 4 / 8 / 16 / 32.
template <int NP>
struct SortNet {
  int n;
  unsigned char lo[NP * 6], hi[NP * 6];
};
template <int NP>
constexpr SortNet<NP> make_sort_net() {
  SortNet<NP> net{};
  for (int p = 1; p < NP; p <<= 1)
    for (int k = p; k >= 1; k >>= 1)
      for (int j = k % p; j + k < NP; j += 2 * k)
        for (int i = 0; i < k && i + j + k < NP; ++i)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
            net.lo[net.n] = (unsigned char)(i + j);
            net.hi[net.n] = (unsigned char)(i + j + k);
            ++net.n;
          }
  return net;
}
template <int NP> constexpr int sort_net_size() {
  return NP == 4 ? 5 : NP == 8 ? 19 : NP == 16 ? 63 : 191;
}
// every index below is a constant expression: the keys stay in registers
// (a runtime-indexed array would go to scratch)
template <int NP, int A, int B>
DEV void compare_exchange(uint32_t (&s)[NP]) {
  const uint32_t a = s[A], b = s[B];
  s[A] = a < b ? a : b;
  s[B] = a < b ? b : a;
}
template <int NP, int... C>
DEV void sort_keys(uint32_t (&s)[NP], std::integer_sequence<int, C...>) {
  constexpr SortNet<NP> net = make_sort_net<NP>();
  static_assert(net.n == sizeof...(C), "comparator count");
  (compare_exchange<NP, net.lo[C], net.hi[C]>(s), ...);
}

constexpr int TRIM_THREADS = 256;
constexpr int TRIM_WAVES = TRIM_THREADS / WAVE;

// One pass over P, V elements per lane and iteration as in weighted_merge_k.
// The N loads of a vector are issued (delta_raw) before any is converted or
// sorted, so they are in flight together. n_models and trim are runtime:
// rows past n_models are pads, and the kept range is taken with masks over
// the unrolled positions. A lane holds the vectors of the NP rows as they
// were stored and, per element, the NP keys twice: as they came (for the
// counts) and sorted. cnt[] lives across the grid-stride loop; at the end it
// is folded per wave, through LDS per block, and one 64-bit integer
// atomicAdd per (block, miner) goes into outside (zero-filled by the caller;
// null: no counts). No barrier in the loop and no return before the one
// after it. Every instantiation the launcher uses has no scratch and no
// spill (docs/kernels.md); <32, 4> would not fit 256 vector registers, so
// 32 rows take one element per lane.
template <int KIND, int NP, int V>
__global__ void __launch_bounds__(TRIM_THREADS)
trimmed_merge_k(const float* __restrict__ base, DELTA_PARAMS, int n_models,
                int trim, int64_t P, float* __restrict__ out,
                unsigned long long* __restrict__ outside) {
  __shared__ uint32_t s_cnt[TRIM_WAVES][NP];
  uint32_t cnt[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) cnt[i] = 0;
  const float fm = float(n_models - 2 * trim);   // kept values, >= 1

  int64_t e = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * V;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x * V;
  for (; e < P; e += stride) {
    const int n = (V == 1 || e + V <= P) ? V : int(P - e);
    // The row stride and the row count are re-read through an empty asm in
    // every trip. Left loop-invariant, the NP row pointers (and NP scale
    // pointers for int8) and a lane mask per row (i < n_models) are hoisted
    // out of the loop into scalar registers, which NP = 16 and 32 do not
    // have: the resource report showed hundreds of spilled SGPRs. Formed
    // next to their use they cost a few scalar instructions.
    int64_t ld = dl_ld, nb = dl_nb;
    int rows = n_models;
    asm volatile("" : "+s"(ld), "+s"(nb), "+s"(rows));
    const PackedView deltas{dl_data, dl_scales, ld, nb, dl_shift, KIND};
    constexpr int RW = raw_words<KIND, V>();
    uint32_t raw[NP][RW];
    float sc[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      // a pad row stays NaN, the key above every real one
#pragma unroll
      for (int w = 0; w < RW; ++w) raw_nan<KIND>(raw[i][w], sc[i]);
      if (i < rows) delta_raw<KIND, V>(deltas, i, e, raw[i], sc[i]);
    }
    float b[V], r[V];
    if (V == 4 && n == 4) {
      const f32x4 vb = *reinterpret_cast<const f32x4*>(base + e);
#pragma unroll
      for (int k = 0; k < V; ++k) b[k] = vb[k];
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) b[k] = k < n ? base[e + k] : 0.f;
    }
    // likewise the words made of the kept range below, three per position:
    // they are formed after the loads. With V == 4 they serve four elements
    // and stay live across four sorts; 3 * 16 of them no longer fit the
    // scalar file (18 to 22 spilled SGPRs), so that instantiation makes them
    // in vector registers, which it has to spare.
    int first = trim, last = n_models - 1 - trim;   // kept positions
    if constexpr (V == 4 && NP >= 16)
      asm volatile("" : "+v"(first), "+v"(last));
    else
      asm volatile("" : "+s"(first), "+s"(last));
#pragma unroll
    for (int k = 0; k < V; ++k) {
      // the keys of element k as the rows came (for the counts) and sorted
      uint32_t key[NP], s[NP];
#pragma unroll
      for (int i = 0; i < NP; ++i)
        s[i] = key[i] = order_key(raw_value<KIND, V>(raw[i], sc[i], k, e));
      sort_keys<NP>(s, std::make_integer_sequence<int, sort_net_size<NP>()>{});
      // kept: all ones at a kept position, one 32-bit word (a select per
      // position holds a 64-bit lane mask each instead). The sorted keys
      // ascend, so the interval's ends are a min and a max under the mask.
      // The sum starts at -0.0, the one float with -0.0 + x == x in bits for
      // every x, and a position that is not kept adds -0.0: the same bits as
      // starting FROM the first kept value, so a kept -0.0 alone stays -0.0.
      uint32_t klo = KEY_NAN, khi = 0;
      float sum = -0.f;
      {
#pragma clang fp contract(off)
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          // first <= j <= last iff (j - first) | (last - j) has no sign bit
          const int x = (j - first) | (last - j);
          const uint32_t kept = ~uint32_t(x >> 31);
          const uint32_t lo_j = s[j] | ~kept, hi_j = s[j] & kept;
          klo = lo_j < klo ? lo_j : klo;
          khi = hi_j > khi ? hi_j : khi;
          const uint32_t term = (__float_as_uint(key_value(s[j])) & kept) |
                                (uint32_t(x) & 0x80000000u);
          sum = sum + __uint_as_float(term);
        }
        const float mean = __fdiv_rn(sum, fm);
        const float o = b[k] + mean;
        // inf - inf has no one NaN: every NaN leaves as 0x7FC00000
        r[k] = o != o ? __uint_as_float(0x7FC00000u) : o;
      }
      if (k < n) {
        // key outside [klo, khi], as one unsigned compare
        const uint32_t span = khi - klo;
#pragma unroll
        for (int i = 0; i < NP; ++i)
          cnt[i] += (key[i] - klo > span) ? 1u : 0u;
      }
    }
    if (V == 4 && n == 4) {
      *reinterpret_cast<f32x4*>(out + e) = f32x4{r[0], r[1], r[2], r[3]};
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (k < n) out[e + k] = r[k];
    }
  }

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (outside != nullptr) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      uint32_t c = cnt[i];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c += uint32_t(__shfl_xor(int(c), o));
      if (lane == 0) s_cnt[wid][i] = c;
    }
  }
  __syncthreads();
  if (outside != nullptr && int(threadIdx.x) < n_models) {
    unsigned long long tot = 0;
#pragma unroll
    for (int w = 0; w < TRIM_WAVES; ++w) tot += s_cnt[w][threadIdx.x];
    if (tot != 0) atomicAdd(outside + threadIdx.x, tot);
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

// ---- blockwise top-k compressor ---------------------------------------------
// entries / residual of d = (w - base) + residual_in (base, residual_in
// optional), equal bit for bit to comm.topk_compress_blockwise on the CPU.
// One workgroup per block, lane t owns elements 16t .. 16t+15 like the int8
// quantiser, d lives in registers only. The key of an element is the bit
// pattern of |d| (NaN sorts above +inf and is always kept).
//   1. radix select of the k-th largest key T: four 8-bit passes, each a
//      256-bin LDS histogram of the keys that still match the prefix (integer
//      atomics: any order gives the same counts), wave 0 suffix-scans the
//      bins and picks the digit. `need` keys equal to T are kept next to
//      every key above it.
//   2. one block-wide exclusive scan of (keys > T, keys == T) per lane, packed
//      in one word: the ties are ranked in index order, the lowest `need`
//      win, and a lane's first output slot is gt_before + min(ties_before,
//      need), so the entries land in ascending idx.
//   3. entries go through LDS and leave as 16 B stores; the residual leaves
//      as the lane's four 16 B stores. A lane reads its own residual_in
//      elements before it writes them, so the two may alias.
// Every loop bound is block-uniform and no lane returns before a barrier.
constexpr int TOPK_PER_LANE = 16;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// bf16 bits of a float, round to nearest even ON THE BITS as the CPU
// definition does it (a NaN is 0x7FC0): no dependence on the denormal mode
DEV uint32_t topk_bf16_bits(uint32_t bits) {
  if ((bits & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u;
  return (bits + 0x7FFFu + ((bits >> 16) & 1u)) >> 16;
}

__global__ void delta_topk_k(const float* __restrict__ w,
                             const float* __restrict__ base,
                             const float* residual_in, float* residual_out,
                             int64_t P, int block, int k,
                             int* __restrict__ entries) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint32_t* s_ent = reinterpret_cast<uint32_t*>(smem);   // [k]
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_wave[16];
  __shared__ uint32_t s_sel[2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t e0 = int64_t(blockIdx.x) * block + tid * TOPK_PER_LANE;

  float d[TOPK_PER_LANE];
  if (e0 + TOPK_PER_LANE <= P) {
#pragma unroll
    for (int v = 0; v < TOPK_PER_LANE / 4; ++v) {
      f32x4 a = *reinterpret_cast<const f32x4*>(w + e0 + 4 * v);
      if (base != nullptr) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(base + e0 + 4 * v);
        a = f32x4{a[0] - b[0], a[1] - b[1], a[2] - b[2], a[3] - b[3]};
      }
      if (residual_in != nullptr) {
        const f32x4 r =
            *reinterpret_cast<const f32x4*>(residual_in + e0 + 4 * v);
        a = f32x4{a[0] + r[0], a[1] + r[1], a[2] + r[2], a[3] + r[3]};
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) d[4 * v + j] = a[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < TOPK_PER_LANE; ++j) {
      const int64_t e = e0 + j;
      float a = 0.f;
      if (e < P) {
        a = base != nullptr ? w[e] - base[e] : w[e];
        if (residual_in != nullptr) a = a + residual_in[e];
      }
      d[j] = a;
    }
  }
  uint32_t key[TOPK_PER_LANE];
#pragma unroll
  for (int j = 0; j < TOPK_PER_LANE; ++j)
    key[j] = __float_as_uint(d[j]) & 0x7FFFFFFFu;

  for (int b = tid; b < 256; b += blockDim.x) s_hist[b] = 0;
  // ---- 1. radix select ------------------------------------------------------
  uint32_t prefix = 0, need = uint32_t(k);
#pragma unroll
  for (int shift = 24; shift >= 0; shift -= 8) {
    const uint32_t hi_mask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
    __syncthreads();            // bins zeroed, s_sel of the last pass read
    // neighbours mostly share a digit: one atomic per run of equal digits
    int cur = -1;
    uint32_t run = 0;
#pragma unroll
    for (int j = 0; j < TOPK_PER_LANE; ++j) {
      if (((key[j] ^ prefix) & hi_mask) == 0) {
        const int bin = int((key[j] >> shift) & 255u);
        if (bin == cur) {
          ++run;
        } else {
          if (run) atomicAdd(&s_hist[cur], run);
          cur = bin;
          run = 1;
        }
      }
    }
    if (run) atomicAdd(&s_hist[cur], run);
    __syncthreads();
    if (wid == 0) {
      // lane l owns bins 4l .. 4l+3; above = count in the bins of lanes > l
      uint32_t c[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = s_hist[4 * lane + j];
      const uint32_t mine = c[0] + c[1] + c[2] + c[3];
      uint32_t suf = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t other = uint32_t(__shfl_down(int(suf), o));
        if (lane + o < 64) suf += other;
      }
      uint32_t gt = suf - mine;
#pragma unroll
      for (int j = 3; j >= 0; --j) {
        // exactly one bin of the 256 has gt < need <= gt + count
        if (gt < need && need <= gt + c[j]) {
          s_sel[0] = uint32_t(4 * lane + j);
          s_sel[1] = need - gt;
        }
        gt += c[j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) s_hist[4 * lane + j] = 0;
    }
    __syncthreads();
    prefix |= s_sel[0] << shift;
    need = s_sel[1];
  }
  const uint32_t T = prefix;    // the k-th largest key; `need` ties are kept

  // ---- 2. slots -------------------------------------------------------------
  uint32_t cnt = 0;             // (keys == T) << 16 | (keys > T)
#pragma unroll
  for (int j = 0; j < TOPK_PER_LANE; ++j)
    cnt += (key[j] > T ? 1u : 0u) + (key[j] == T ? 0x10000u : 0u);
  uint32_t inc = cnt;           // inclusive scan inside the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t other = uint32_t(__shfl_up(int(inc), o));
    if (lane >= o) inc += other;
  }
  if (lane == 63) s_wave[wid] = inc;
  __syncthreads();
  uint32_t before = inc - cnt;
#pragma unroll
  for (int q = 0; q < 16; ++q)
    if (q < wid) before += s_wave[q];
  uint32_t tie_rank = before >> 16;
  uint32_t slot = (before & 0xFFFFu) + (tie_rank < need ? tie_rank : need);

  // ---- 3. entries and residual ---------------------------------------------
  float res[TOPK_PER_LANE];
#pragma unroll
  for (int j = 0; j < TOPK_PER_LANE; ++j) {
    bool keep = key[j] > T;
    if (key[j] == T) {
      keep = tie_rank < need;
      ++tie_rank;
    }
    float r = d[j];
    // slot < k always: the kept elements of the block are exactly k
    if (keep && slot < uint32_t(k)) {
      const uint32_t bf = topk_bf16_bits(__float_as_uint(d[j]));
      s_ent[slot++] = (uint32_t(tid * TOPK_PER_LANE + j) << 16) | bf;
      r = d[j] - __uint_as_float(bf << 16);
    }
    if ((__float_as_uint(r) & 0x7F800000u) == 0x7F800000u) r = 0.f;
    res[j] = r;
  }
  if (residual_out != nullptr) {
    if (e0 + TOPK_PER_LANE <= P) {
#pragma unroll
      for (int v = 0; v < TOPK_PER_LANE / 4; ++v)
        *reinterpret_cast<f32x4*>(residual_out + e0 + 4 * v) = f32x4{
            res[4 * v], res[4 * v + 1], res[4 * v + 2], res[4 * v + 3]};
    } else {
#pragma unroll
      for (int j = 0; j < TOPK_PER_LANE; ++j)
        if (e0 + j < P) residual_out[e0 + j] = res[j];
    }
  }
  __syncthreads();
  u32x4* dst = reinterpret_cast<u32x4*>(entries + int64_t(blockIdx.x) * k);
  for (int v = tid; v < k / 4; v += blockDim.x)
    dst[v] = *reinterpret_cast<const u32x4*>(s_ent + 4 * v);
}

// ---- top-k deltas: the three consumers ---------------------------------------
// data: int32 [N, ld = nb*k] entries (idx << 16 | bf16 bits), k per block of
// 1 << shift elements, ascending idx. Each result equals the fp32 kernel on
// the densified rows bit for bit: the kernels below densify one (row, tile)
// at a time in LDS and then do per element exactly what the dense kernels
// do. A tile is min(block, TOPK_TILE) elements; a block wider than a tile is
// walked tile by tile, every tile looking through all k entries of its
// block. Two tiles alternate, so one barrier covers a scatter: a lane zeroes
// the tile elements it has just read (nobody else reads them), which leaves
// that tile clean for the scatter after the next barrier.
constexpr int TOPK_TILE = 4096;
constexpr int TOPK_THREADS = 256;
constexpr int TOPK_VECS = TOPK_TILE / (4 * TOPK_THREADS);   // per lane

struct TopkArgs {
  const int* data;
  int64_t ld;
  int shift, k, tile;
};

// entries of row i that fall into [lo, hi) of the tile starting at t0 go to
// their place in `tile` (fp32 [a.tile], clean on entry)
DEV void topk_scatter(const TopkArgs& a, int i, int64_t t0, int64_t lo,
                      int64_t hi, float* tile) {
  const int64_t blk = t0 >> a.shift;
  const int64_t b0 = blk << a.shift;
  const int* ent = a.data + int64_t(i) * a.ld + blk * a.k;
  for (int j = threadIdx.x; j < a.k; j += blockDim.x) {
    const uint32_t en = uint32_t(ent[j]);
    const int64_t e = b0 + int64_t(en >> 16);
    // hi <= P and hi <= t0 + tile: entries past the plane or outside the
    // tile are skipped here
    if (e >= lo && e < hi) tile[e - t0] = __uint_as_float(en << 16);
  }
}

__global__ void __launch_bounds__(TOPK_THREADS)
weighted_merge_topk_k(const float* __restrict__ base, TopkArgs a,
                      const float* __restrict__ W,
                      const int64_t* __restrict__ offsets, int n_models,
                      int n_segs, int64_t P, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_tile = reinterpret_cast<float*>(smem);          // [2][a.tile]
  int64_t* s_off = reinterpret_cast<int64_t*>(smem + 2 * a.tile * 4);
  float* s_w = reinterpret_cast<float*>(
      smem + 2 * a.tile * 4 + (n_segs + 1) * sizeof(int64_t) +
      ((n_segs + 1) & 1) * 8);
  for (int i = threadIdx.x; i <= n_segs; i += blockDim.x)
    s_off[i] = offsets[i];
  for (int i = threadIdx.x; i < n_models * n_segs; i += blockDim.x)
    s_w[i] = W[i];
  for (int i = threadIdx.x; i < 2 * a.tile; i += blockDim.x) s_tile[i] = 0.f;
  __syncthreads();

  const int64_t n_tiles = (P + a.tile - 1) / a.tile;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t t0 = t * a.tile;
    const int64_t hi = t0 + a.tile < P ? t0 + a.tile : P;
    int seg[TOPK_VECS][4];
    float b[TOPK_VECS][4], acc[TOPK_VECS][4];
#pragma unroll
    for (int v = 0; v < TOPK_VECS; ++v) {
      const int64_t e = t0 + (threadIdx.x + v * TOPK_THREADS) * 4;
      const bool live = (threadIdx.x + v * TOPK_THREADS) * 4 < a.tile;
      if (live && e + 4 <= P) {
        const f32x4 vb = *reinterpret_cast<const f32x4*>(base + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[v][j] = vb[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          b[v][j] = (live && e + j < P) ? base[e + j] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // past the plane: any valid segment, the element is never stored
        const int64_t ej = e + j < P ? e + j : P - 1;
        seg[v][j] = (j > 0 && ej < s_off[seg[v][j - 1] + 1])
                        ? seg[v][j - 1] : find_seg(s_off, n_segs, ej);
        acc[v][j] = 0.f;
      }
    }
    topk_scatter(a, 0, t0, t0, hi, s_tile);
    for (int i = 0; i < n_models; ++i) {
      __syncthreads();
      float* cur = s_tile + (i & 1) * a.tile;
      if (i + 1 < n_models)
        topk_scatter(a, i + 1, t0, t0, hi, s_tile + ((i + 1) & 1) * a.tile);
#pragma unroll
      for (int v = 0; v < TOPK_VECS; ++v) {
        const int l = (threadIdx.x + v * TOPK_THREADS) * 4;
        if (l < a.tile) {
          const f32x4 dv = *reinterpret_cast<const f32x4*>(cur + l);
          *reinterpret_cast<f32x4*>(cur + l) = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[v][j] = fmaf(s_w[i * n_segs + seg[v][j]], b[v][j] + dv[j],
                             acc[v][j]);
        }
      }
    }
#pragma unroll
    for (int v = 0; v < TOPK_VECS; ++v) {
      const int l = (threadIdx.x + v * TOPK_THREADS) * 4;
      const int64_t e = t0 + l;
      if (l < a.tile) {
        if (e + 4 <= P) {
          *reinterpret_cast<f32x4*>(out + e) =
              f32x4{acc[v][0], acc[v][1], acc[v][2], acc[v][3]};
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (e + j < P) out[e + j] = acc[v][j];
        }
      }
    }
    __syncthreads();   // tile 0 is clean before the next scatter into it
  }
}

// grid = (chunks, n_models) and lane t sums start + t, + 256, ... in
// ascending order, as grad_w_k does. A chunk starts at a segment offset, so
// it is walked over the tiles it overlaps; only entries inside the chunk are
// scattered, so every scattered element is read, and zeroed, by its lane.
template <bool G_BF16>
__global__ void __launch_bounds__(GW_THREADS)
grad_w_topk_k(const void* __restrict__ gp, const float* __restrict__ base,
              TopkArgs a, const float* __restrict__ merged,
              const int64_t* __restrict__ chunks, int n_segs, int64_t P,
              float* __restrict__ grad_w) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_tile = reinterpret_cast<float*>(smem);          // [2][a.tile]
  __shared__ float lds[16];
  const int64_t start = chunks[blockIdx.x * 3 + 0];
  const int64_t end = chunks[blockIdx.x * 3 + 1];
  const int seg = int(chunks[blockIdx.x * 3 + 2]);
  const int i = blockIdx.y;
  for (int j = threadIdx.x; j < 2 * a.tile; j += blockDim.x) s_tile[j] = 0.f;
  __syncthreads();
  float acc = 0.f;
  int64_t e = start + threadIdx.x;
  const int64_t t_first = start / a.tile;
  const int64_t t_end = (end + a.tile - 1) / a.tile;   // start == end: none
  if (t_first < t_end)
    topk_scatter(a, i, t_first * a.tile, start,
                 end < (t_first + 1) * a.tile ? end : (t_first + 1) * a.tile,
                 s_tile);
  for (int64_t t = t_first; t < t_end; ++t) {
    __syncthreads();
    const int64_t t0 = t * a.tile;
    const int64_t hi = end < t0 + a.tile ? end : t0 + a.tile;
    float* cur = s_tile + ((t - t_first) & 1) * a.tile;
    if (t + 1 < t_end)
      topk_scatter(a, i, t0 + a.tile, t0 + a.tile,
                   end < t0 + 2 * int64_t(a.tile) ? end
                                                  : t0 + 2 * int64_t(a.tile),
                   s_tile + ((t + 1 - t_first) & 1) * a.tile);
    // the plain loop of grad_w_k. Loading 8 elements ahead with predicated
    // loads measured 5.95 ms against 3.38 ms for this form
    // (profiles/r09_topk_deltas.md).
    for (; e < hi; e += GW_THREADS) {
      const float g = G_BF16 ? bf2f(reinterpret_cast<const ushort*>(gp)[e])
                             : reinterpret_cast<const float*>(gp)[e];
      const float d = cur[e - t0];
      cur[e - t0] = 0.f;
      acc = fmaf(g, (base[e] - merged[e]) + d, acc);
    }
  }
  acc = block_sum<16>(acc, lds);
  if (threadIdx.x == 0) atomicAdd(grad_w + int64_t(i) * n_segs + seg, acc);
}

// w[e] = fma(alpha, v, w[e]) over the in-range entries of one row: the
// indices of a row are unique, so plain stores. Four entries per lane (one
// 16 B load; k % 4 == 0 keeps them in one block).
__global__ void axpy_topk_k(float* __restrict__ w, TopkArgs a, int row,
                            float alpha, int64_t P) {
  const int* ent = a.data + int64_t(row) * a.ld;
  int64_t q = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * 4;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x * 4;
  for (; q < a.ld; q += stride) {
    const u32x4 en = *reinterpret_cast<const u32x4*>(ent + q);
    const int64_t b0 = (q / a.k) << a.shift;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t e = b0 + int64_t(en[j] >> 16);
      if (e < P) w[e] = fmaf(alpha, __uint_as_float(en[j] << 16), w[e]);
    }
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

int64_t dta_trimmed_sweep(int kind, int n_models, int64_t P) {
  return int64_t(MAX_RESIDENT_BLOCKS) * TRIM_THREADS *
         dta_trimmed_vec(kind, n_models, P);
}

void launch_trimmed_merge(const float* base, const PackedView& d,
                          int n_models, int trim, int64_t P, float* out,
                          int64_t* outside, hipStream_t s) {
  const int np = dta_trimmed_pad(n_models);
  const int v = dta_trimmed_vec(d.kind, n_models, P);
  const int grid = elementwise_grid(P, TRIM_THREADS, v);
  auto* cnt = reinterpret_cast<unsigned long long*>(outside);
#define TRIM_GO(KIND, NP, V)                                                \
  trimmed_merge_k<KIND, NP, V><<<grid, TRIM_THREADS, 0, s>>>(               \
      base, DELTA_ARGS(d), n_models, trim, P, out, cnt)
#define TRIM_NP(KIND, V)                                                    \
  do {                                                                      \
    if (np == 4) TRIM_GO(KIND, 4, V);                                       \
    else if (np == 8) TRIM_GO(KIND, 8, V);                                  \
    else TRIM_GO(KIND, 16, V);                                              \
  } while (0)
  // 32 keys are one element per lane (dta_trimmed_vec): <32, 4> would need
  // more than the 256 vector registers and is not built
#define TRIM_KIND(KIND)                                                     \
  do {                                                                      \
    if (np == 32) TRIM_GO(KIND, 32, 1);                                     \
    else if (v == 4) TRIM_NP(KIND, 4);                                      \
    else TRIM_NP(KIND, 1);                                                  \
  } while (0)
  if (d.kind == DELTA_I8) TRIM_KIND(DELTA_I8);
  else if (d.kind == DELTA_BF16) TRIM_KIND(DELTA_BF16);
  else TRIM_KIND(DELTA_F32);
#undef TRIM_KIND
#undef TRIM_NP
#undef TRIM_GO
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

// ---- top-k deltas -------------------------------------------------------------
namespace {
TopkArgs topk_args(const TopkView& d) {
  const int block = 1 << d.shift;
  return TopkArgs{d.data, d.ld, d.shift, d.k,
                  block < TOPK_TILE ? block : TOPK_TILE};
}
}  // namespace

size_t dta_topk_merge_shmem(int n_models, int n_segs, int block) {
  return 2 * sizeof(float) * size_t(block < TOPK_TILE ? block : TOPK_TILE) +
         merge_shmem(n_models, n_segs);
}

void launch_delta_topk(const float* w, const float* base,
                       const float* residual_in, float* residual_out,
                       int64_t P, int block, int k, int64_t nb, int* entries,
                       hipStream_t s) {
  const int threads = block / TOPK_PER_LANE;
  const size_t shmem = size_t(k) * sizeof(int);
  delta_topk_k<<<unsigned(nb), threads, shmem, s>>>(
      w, base, residual_in, residual_out, P, block, k, entries);
}

void launch_weighted_merge_topk(const float* base, const TopkView& d,
                                const float* W, const int64_t* offsets,
                                int n_models, int n_segs, int64_t P,
                                float* out, hipStream_t s) {
  const TopkArgs a = topk_args(d);
  const int64_t n_tiles = (P + a.tile - 1) / a.tile;
  const int grid =
      int(n_tiles < MAX_RESIDENT_BLOCKS ? n_tiles : MAX_RESIDENT_BLOCKS);
  const size_t shmem = dta_topk_merge_shmem(n_models, n_segs, 1 << d.shift);
  weighted_merge_topk_k<<<grid, TOPK_THREADS, shmem, s>>>(
      base, a, W, offsets, n_models, n_segs, P, out);
}

void launch_grad_merge_weights_topk(const void* g, bool g_is_bf16,
                                    const float* base, const TopkView& d,
                                    const float* merged,
                                    const int64_t* chunks, int n_models,
                                    int n_chunks, int64_t P, float* grad_w,
                                    int n_segs, hipStream_t s) {
  const TopkArgs a = topk_args(d);
  dim3 grid(n_chunks, n_models);
  const size_t shmem = 2 * sizeof(float) * size_t(a.tile);
  if (g_is_bf16)
    grad_w_topk_k<true><<<grid, GW_THREADS, shmem, s>>>(
        g, base, a, merged, chunks, n_segs, P, grad_w);
  else
    grad_w_topk_k<false><<<grid, GW_THREADS, shmem, s>>>(
        g, base, a, merged, chunks, n_segs, P, grad_w);
}

void launch_axpy_topk(float* w, const TopkView& d, int row, float alpha,
                      int64_t P, hipStream_t s) {
  const int block = 256;
  const int grid = elementwise_grid(d.ld, block, 4);
  axpy_topk_k<<<grid, block, 0, s>>>(w, topk_args(d), row, alpha, P);
}
