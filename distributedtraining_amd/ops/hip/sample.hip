// Fused token sampler for graph-replayed decode: one row of bf16 logits in,
// one token out, with temperature, top-k, top-p, the draw and generate()'s
// bookkeeping (done / eos, the next step's input token, the ids column) in
// one launch that a hipGraph can hold. CPU definition: ops/sampling.py.
//
// One workgroup of 1024 lanes per row.
//
//   keys     A bf16 logit maps to an order-preserving 16-bit key (NaN counts
//            as -inf, -0 as +0); 0 is no logit at all and marks the slots
//            outside the row. Temperature is a positive scale and leaves the
//            order alone, so each filter is one key threshold and a logit is
//            kept iff key >= T. Rows of up to SMP_REG_ROUNDS * 8192 - 16
//            logits stay in registers as packed keys (4 VGPRs per 16 B
//            chunk) after the one read; wider rows are read again from L2 by
//            every pass, up to DTA_SAMPLE_MAX_V.
//   slots    The row is cut where its memory is 16 B aligned: slot 0 is the
//            up to 7 logits before the first aligned address, slots 1..n the
//            aligned chunks (one 16 B load each), slot n+1 the tail; head and
//            tail take scalar loads, so any row stride and any V work. Slot s
//            belongs to lane s % 1024 in round s / 1024 (coalesced), and
//            logit j of slot s is index a0 + 8 (s - 1) + j.
//   mass     w = exp2((l - max) * log2e / temperature), converted once to
//            fixed point with 40 fractional bits in a uint64 (V <= 2^20: a
//            row sum stays below 2^60). Every histogram, scan and comparison
//            after that is integer and LDS integer atomics commute, so the
//            token repeats bit for bit. No float atomics.
//   radix    A threshold is found by two histogram passes, high byte then
//            low byte, 256 bins each (16 replicas per bin, picked by lane, so
//            a popular bin is not one serialised LDS address). With A(b) the
//            sum of the bins above b, wave 0 scans for the lowest b with
//            A(b) <= q. Top-k: counts, q = k - 1, so Tk is the k-th largest
//            key and its ties stay. Top-p: masses of the keys >= Tk,
//            q = p * W, so a key is kept iff the mass strictly above it is
//            <= p * W, ties together.
//   draw     h = rng_elem_hash(rng_site_seed(ctr, SITE_SAMPLE), row),
//            target = mulhi64(h, W') with W' the kept mass; the token is the
//            lowest kept index whose inclusive prefix sum, in index order,
//            exceeds target: per-round totals (wave sums, one LDS atomic per
//            wave and round) name the round, one block scan over that
//            round's slots names the lane, the lane walks its 8 logits.
//
// All loop bounds are block-uniform and no lane leaves before the last
// barrier. The counter is read, never written: the caller's captured
// rng_tick advances it.
#include "dta_common.h"
#include "dta_kernels.h"

namespace {

#define SMP_INL __attribute__((always_inline))   // lambdas: keys stay in VGPRs
constexpr int SMP_THREADS = 1024;
constexpr int SMP_WAVES = SMP_THREADS / WAVE;
constexpr int SMP_REP = 16;          // histogram replicas per bin
constexpr int SMP_REG_ROUNDS = 7;    // register-resident rounds: 28 VGPRs of keys
constexpr int SMP_MAX_ROUNDS =
    (DTA_SAMPLE_MAX_V / 8 + 2 + SMP_THREADS - 1) / SMP_THREADS;
constexpr uint32_t SMP_KEY_NINF = 0x007Fu;   // -inf and NaN
constexpr uint32_t SMP_KEY_PINF = 0xFF80u;

struct SmpLds {
  unsigned long long hist[256 * SMP_REP];
  unsigned long long val[256];
  unsigned long long rtot[SMP_MAX_ROUNDS];
  unsigned long long wtot[SMP_WAVES];
  unsigned long long above, q;
  uint32_t red[SMP_WAVES];
  int bin;
};

struct SmpRow {
  const ushort* p;
  int V, a0, nslots, nrounds;
};

DEV uint32_t smp_key(uint32_t u) {
  if ((u & 0x7FFFu) > 0x7F80u) return SMP_KEY_NINF;
  if (u == 0x8000u) return 0x8000u;
  return (u & 0x8000u) ? (~u & 0xFFFFu) : (u | 0x8000u);
}
DEV float smp_val(uint32_t key) {
  return bf2f(ushort((key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu)));
}
DEV uint32_t smp_key_at(const uint32_t (&k)[4], int j) {
  return (k[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
}
DEV unsigned long long smp_weight(uint32_t key, float mx, float scale) {
  const float w = __builtin_amdgcn_exp2f((smp_val(key) - mx) * scale);
  return (unsigned long long)(w * 0x1p40f);
}

// packed keys of slot s; 0 where the slot reaches outside the row
DEV void smp_load(const SmpRow& R, int s, uint32_t (&k)[4]) {
  k[0] = k[1] = k[2] = k[3] = 0u;
  if (s >= R.nslots) return;
  const int i0 = R.a0 + 8 * (s - 1);
  if (i0 >= 0 && i0 + 8 <= R.V) {
    const uint4 v = *reinterpret_cast<const uint4*>(R.p + i0);
    const uint32_t raw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int w = 0; w < 4; ++w)
      k[w] = smp_key(raw[w] & 0xFFFFu) | (smp_key(raw[w] >> 16) << 16);
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = i0 + j;
    if (i >= 0 && i < R.V) k[j >> 1] |= smp_key(R.p[i]) << (16 * (j & 1));
  }
}

// f(round, keys) over this lane's slots: the register copy, or a fresh read
template <bool REG, class F>
DEV void smp_each(const SmpRow& R, const uint32_t (*kk)[4], F f) {
  if constexpr (REG) {
#pragma unroll
    for (int r = 0; r < SMP_REG_ROUNDS; ++r) f(r, kk[r]);
  } else {
    for (int r = 0; r < R.nrounds; ++r) {
      uint32_t k[4];
      smp_load(R, r * SMP_THREADS + int(threadIdx.x), k);
      f(r, k);
    }
  }
}

DEV uint32_t smp_block_max(uint32_t v, SmpLds& L) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t t = __shfl_xor(v, off);
    v = t > v ? t : v;
  }
  if ((threadIdx.x & 63) == 0) L.red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < SMP_WAVES; ++i) r = L.red[i] > r ? L.red[i] : r;
  __syncthreads();
  return r;
}

// L.hist holds a finished histogram. Finds the lowest bin b with
// base + A(b) <= q, A(b) the sum of the bins above b (base <= q, so bin 255
// always qualifies); from_total: q = mulhi64(p64, sum of all bins). Leaves
// bin, base + A(bin) and q in L.
DEV void smp_pick(SmpLds& L, unsigned long long base, unsigned long long q,
                  bool from_total, unsigned long long p64) {
  const int t = threadIdx.x;
  if (t < 256) {
    unsigned long long s = 0;
#pragma unroll
    for (int i = 0; i < SMP_REP; ++i)      // rotated: spreads the LDS banks
      s += L.hist[t * SMP_REP + ((i + t) & (SMP_REP - 1))];
    L.val[t] = s;
  }
  __syncthreads();
  if (t < WAVE) {
    unsigned long long v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = L.val[4 * t + j];
    const unsigned long long s = v[0] + v[1] + v[2] + v[3];
    unsigned long long incl = s;           // sum of the bins >= 4 t
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      const unsigned long long o = __shfl_down(incl, off);
      if (t + off < WAVE) incl += o;
    }
    const unsigned long long total = __shfl(incl, 0);
    if (from_total) q = __umul64hi(p64, total);
    const unsigned long long a3 = base + (incl - s);   // above bin 4 t + 3
    const unsigned long long a2 = a3 + v[3], a1 = a2 + v[2], a0 = a1 + v[1];
    const unsigned long long has = __ballot(a3 <= q);
    if (t == __ffsll((long long)has) - 1) {
      const int j = a0 <= q ? 0 : a1 <= q ? 1 : a2 <= q ? 2 : 3;
      L.bin = 4 * t + j;
      L.above = j == 0 ? a0 : j == 1 ? a1 : j == 2 ? a2 : a3;
      L.q = q;
    }
  }
  __syncthreads();
}

DEV void smp_hist_clear(SmpLds& L) {
  for (int i = threadIdx.x; i < 256 * SMP_REP; i += SMP_THREADS) L.hist[i] = 0;
  __syncthreads();
}

// The key threshold of one filter over the keys >= tmin. MASS false: the
// largest key with at least q + 1 keys at or above it (q = k - 1). MASS
// true: the lowest key whose mass strictly above it is <= p64 / 2^64 of the
// mass of all keys >= tmin.
template <bool REG, bool MASS>
DEV uint32_t smp_threshold(const SmpRow& R, const uint32_t (*kk)[4],
                           uint32_t tmin, unsigned long long q,
                           unsigned long long p64, float mx, float scale,
                           SmpLds& L) {
  const int rep = threadIdx.x & (SMP_REP - 1);
  smp_hist_clear(L);
  smp_each<REG>(R, kk, [&](int, const uint32_t (&k)[4]) SMP_INL {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t key = smp_key_at(k, j);
      if (key >= tmin) {
        const unsigned long long w = MASS ? smp_weight(key, mx, scale) : 1ull;
        atomicAdd(&L.hist[(key >> 8) * SMP_REP + rep], w);
      }
    }
  });
  __syncthreads();
  smp_pick(L, 0, q, MASS, p64);
  const uint32_t hi = uint32_t(L.bin);
  const unsigned long long base = L.above;
  q = L.q;
  smp_hist_clear(L);      // its barrier also orders the reads of L above
  smp_each<REG>(R, kk, [&](int, const uint32_t (&k)[4]) SMP_INL {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t key = smp_key_at(k, j);
      if (key >= tmin && (key >> 8) == hi) {
        const unsigned long long w = MASS ? smp_weight(key, mx, scale) : 1ull;
        atomicAdd(&L.hist[(key & 0xFFu) * SMP_REP + rep], w);
      }
    }
  });
  __syncthreads();
  smp_pick(L, base, q, false, 0);
  const uint32_t t = (hi << 8) | uint32_t(L.bin);
  __syncthreads();
  return t;
}

// generate()'s bookkeeping for one row, by one lane
DEV void smp_emit(const SampleArgs& a, int row, int token) {
  long long t = token;
  if (a.done) {
    if (a.done[row]) t = a.eos;
    if (t == a.eos) a.done[row] = 1;
  }
  if (a.tok) a.tok[row] = t;
  if (a.ids) {
    int c = *a.pos_p;
    c = c < 0 ? 0 : (c < a.total ? c : a.total - 1);
    a.ids[int64_t(row) * a.ids_ld + c] = t;
  }
}

// The exponent arguments stay scalar fp32 instructions (packed two-lane forms
// off, as for the other serving kernels).
template <bool REG>
__global__ __launch_bounds__(SMP_THREADS)
__attribute__((target("no-packed-fp32-ops")))
void sample_tokens_k(SampleArgs a) {
  __shared__ SmpLds L;
  const int tid = threadIdx.x, row = blockIdx.x;
  SmpRow R;
  R.p = a.logits + int64_t(row) * a.ld;
  R.V = a.V;
  R.a0 = int(((16u - unsigned(reinterpret_cast<uintptr_t>(R.p) & 15u)) & 15u)
             >> 1);
  R.a0 = R.a0 < a.V ? R.a0 : a.V;
  R.nslots = (a.V - R.a0) / 8 + 2;
  R.nrounds = (R.nslots + SMP_THREADS - 1) / SMP_THREADS;
  const int nrounds = REG ? SMP_REG_ROUNDS : R.nrounds;

  uint32_t kk[REG ? SMP_REG_ROUNDS : 1][4];
  if constexpr (REG) {
#pragma unroll
    for (int r = 0; r < SMP_REG_ROUNDS; ++r)
      smp_load(R, r * SMP_THREADS + tid, kk[r]);
  }
  // index of logit j of this lane's slot in round r
  auto index_of = [&](int r, int j) SMP_INL {
    return R.a0 + 8 * (r * SMP_THREADS + tid - 1) + j;
  };

  uint32_t mk = 0;
  smp_each<REG>(R, kk, [&](int, const uint32_t (&k)[4]) SMP_INL {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t key = smp_key_at(k, j);
      mk = key > mk ? key : mk;
    }
  });
  mk = smp_block_max(mk, L);

  if (!(a.scale > 0.f) || mk == SMP_KEY_NINF || mk == SMP_KEY_PINF) {
    // greedy: the lowest index of the maximum (block max of ~index). The
    // branch is block-uniform; all lanes leave together after its barriers.
    uint32_t best = 0;
    smp_each<REG>(R, kk, [&](int r, const uint32_t (&k)[4]) SMP_INL {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (smp_key_at(k, j) == mk) {
          const uint32_t c = ~uint32_t(index_of(r, j));
          best = c > best ? c : best;
        }
    });
    best = smp_block_max(best, L);
    if (tid == 0) smp_emit(a, row, int(~best));
    return;
  }

  const float mx = smp_val(mk);
  uint32_t T = 1;     // every logit of the row; 0 is outside it
  if (a.top_k > 0)
    T = smp_threshold<REG, false>(R, kk, 1u, (unsigned long long)(a.top_k - 1),
                                  0, mx, a.scale, L);
  if (a.top_p64 != 0) {
    const uint32_t tp = smp_threshold<REG, true>(R, kk, T, 0, a.top_p64, mx,
                                                 a.scale, L);
    T = tp > T ? tp : T;
  }

  // kept mass per round
  if (tid < SMP_MAX_ROUNDS) L.rtot[tid] = 0;
  __syncthreads();
  auto slot_mass = [&](const uint32_t (&k)[4]) SMP_INL {
    unsigned long long s = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t key = smp_key_at(k, j);
      if (key >= T) s += smp_weight(key, mx, a.scale);
    }
    return s;
  };
  smp_each<REG>(R, kk, [&](int r, const uint32_t (&k)[4]) SMP_INL {
    unsigned long long s = slot_mass(k);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((tid & 63) == 0 && s) atomicAdd(&L.rtot[r], s);
  });
  __syncthreads();
  unsigned long long W = 0;
  for (int r = 0; r < nrounds; ++r) W += L.rtot[r];
  // the maximum weighs 2^40 and is always kept: W > 0, target < W
  const unsigned long long target =
      __umul64hi(rng_elem_hash(rng_site_seed(a.ctr, DTA_RNG_SITE_SAMPLE),
                               uint64_t(row)), W);
  int rr = 0;
  unsigned long long acc = 0;
  for (; rr < nrounds - 1; ++rr) {
    const unsigned long long t = L.rtot[rr];
    if (target < acc + t) break;
    acc += t;
  }

  // block scan over the slots of round rr (index order = lane order)
  uint32_t k[4];
  smp_load(R, rr * SMP_THREADS + tid, k);
  const unsigned long long s = slot_mass(k);
  unsigned long long incl = s;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const unsigned long long o = __shfl_up(incl, off);
    if ((tid & 63) >= off) incl += o;
  }
  if ((tid & 63) == 63) L.wtot[tid >> 6] = incl;
  __syncthreads();
  unsigned long long before = acc + incl - s;
  for (int w = 0; w < (tid >> 6); ++w) before += L.wtot[w];
  if (s && before <= target && target < before + s) {
    int token = 0;
    unsigned long long c = before;
    bool found = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t key = smp_key_at(k, j);
      if (key >= T) c += smp_weight(key, mx, a.scale);
      if (!found && c > target) {
        found = true;
        token = index_of(rr, j);
      }
    }
    smp_emit(a, row, token);
  }
}

}  // namespace

void launch_sample_tokens(const SampleArgs& a, hipStream_t s) {
  if (a.V / 8 + 2 <= SMP_REG_ROUNDS * SMP_THREADS)
    sample_tokens_k<true><<<a.B, SMP_THREADS, 0, s>>>(a);
  else
    sample_tokens_k<false><<<a.B, SMP_THREADS, 0, s>>>(a);
}
