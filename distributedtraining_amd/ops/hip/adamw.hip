// Fused decoupled AdamW over the flat parameter plane: one kernel updates
// fp32 master + m + v and writes the bf16 working copy (replaces the
// reference's torch.optim.AdamW step, training_manager.py:391).
// Memory-bound: ~(3 reads + 3 writes) x 4B + grad; float4-vectorized.
//
// Guarded step (clip / non-finite skip / LR schedule, all without a host
// round-trip): gradnorm_part_k -> step_ctl_k -> adamw_k<.., CTL = true>.
// The three communicate through a small device control block:
//   ctl_f fp32[6]  {lr, coef, grad_norm, bc1, bc2, unused}
//   ctl_i int32[4] {t, sched_step, skip_now, skipped_total}
// step_ctl_k is the only writer; t counts applied steps (bias correction),
// sched_step every step (the schedule's clock), skipped_total the steps
// dropped for a non-finite gradient. A bf16 gradient whose square overflows
// fp32 (|g| > 1.8e19) makes the sum infinite and counts as non-finite.
#include "dta_common.h"
#include "dta_kernels.h"

namespace {

// control block slots (file header)
enum { CTL_LR = 0, CTL_COEF = 1, CTL_NORM = 2, CTL_BC1 = 3, CTL_BC2 = 4 };
enum { CTL_T = 0, CTL_SCHED = 1, CTL_SKIP_NOW = 2, CTL_SKIPPED = 3 };

// bc_p: optional device pointer {bc1, bc2} maintained by adamw_tick_k so
// the step is hipGraph-capturable (step counter lives on device); if null
// the host-computed bc1/bc2 scalars are used. omb1/omb2: 1 - beta, formed in
// double on the host (launch_adamw).
// CTL: lr, bc1, bc2 and the clip factor come from the control block, and a
// set skip_now ends the kernel before it touches memory (the flag is the
// same for every thread; there is no barrier to miss). The clip factor
// scales g in registers: the gradient plane is never written. ctl_f / ctl_i
// are null and unread when CTL is false.
template <bool GRAD_BF16, bool WRITE_BF16, bool CTL>
__global__ void adamw_k(float* __restrict__ w, const void* __restrict__ gp,
                        float* __restrict__ m, float* __restrict__ v,
                        ushort* __restrict__ wout, float lr, float beta1,
                        float beta2, float omb1, float omb2, float eps,
                        float wd, float bc1, float bc2,
                        const float* __restrict__ bc_p, int64_t n,
                        const float* __restrict__ ctl_f,
                        const int* __restrict__ ctl_i) {
  int64_t i = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * 4;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x * 4;
  float coef = 1.0f;
  if (CTL) {
    if (ctl_i[CTL_SKIP_NOW]) return;
    lr = ctl_f[CTL_LR]; coef = ctl_f[CTL_COEF];
    bc1 = ctl_f[CTL_BC1]; bc2 = ctl_f[CTL_BC2];
  } else if (bc_p) { bc1 = bc_p[0]; bc2 = bc_p[1]; }
  const float decay = 1.0f - lr * wd;
  const float step_size = lr / bc1;
  const float inv_bc2 = 1.0f / bc2;
  for (; i + 4 <= n; i += stride) {
    f32x4 wv = *reinterpret_cast<const f32x4*>(w + i);
    f32x4 mv = *reinterpret_cast<const f32x4*>(m + i);
    f32x4 vv = *reinterpret_cast<const f32x4*>(v + i);
    f32x4 gv;
    if (GRAD_BF16) {
      s16x4 gr = *reinterpret_cast<const s16x4*>(
          reinterpret_cast<const ushort*>(gp) + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) gv[j] = bf2f(ushort(gr[j]));
    } else {
      gv = *reinterpret_cast<const f32x4*>(
          reinterpret_cast<const float*>(gp) + i);
    }
    s16x4 bo;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float g = CTL ? gv[j] * coef : gv[j];
      float mm = fmaf(beta1, mv[j], omb1 * g);
      float vvj = fmaf(beta2, vv[j], omb2 * g * g);
      float ww = wv[j] * decay;
      ww -= step_size * mm / (sqrtf(vvj * inv_bc2) + eps);
      mv[j] = mm; vv[j] = vvj; wv[j] = ww;
      if (WRITE_BF16) bo[j] = f2bf(ww);
    }
    *reinterpret_cast<f32x4*>(w + i) = wv;
    *reinterpret_cast<f32x4*>(m + i) = mv;
    *reinterpret_cast<f32x4*>(v + i) = vv;
    if (WRITE_BF16) *reinterpret_cast<s16x4*>(wout + i) = bo;
  }
  if (i < n && i + 4 > n)
    for (; i < n; ++i) {
      float g = GRAD_BF16 ? bf2f(reinterpret_cast<const ushort*>(gp)[i])
                          : reinterpret_cast<const float*>(gp)[i];
      if (CTL) g *= coef;
      float mm = fmaf(beta1, m[i], omb1 * g);
      float vvj = fmaf(beta2, v[i], omb2 * g * g);
      float ww = w[i] * decay;
      ww -= step_size * mm / (sqrtf(vvj * inv_bc2) + eps);
      m[i] = mm; v[i] = vvj; w[i] = ww;
      if (WRITE_BF16) wout[i] = f2bf(ww);
    }
}

// Device-side step counter tick: t += 1; bc = {1-beta1^t, 1-beta2^t}.
// Launched (1,1) right before adamw_k inside a captured graph.
// In double, as the host path does (one thread, once per step).
__global__ void adamw_tick_k(int* __restrict__ t, float* __restrict__ bc,
                             double beta1, double beta2) {
  const int nt = *t + 1;
  *t = nt;
  bc[0] = float(1.0 - pow(beta1, double(nt)));
  bc[1] = float(1.0 - pow(beta2, double(nt)));
}

// Sum of squares of the flat gradient plane, one fp32 partial per block:
// 16 B loads, fp32 fma per thread, block_sum, one plain store. The grid is
// elementwise_grid(n), so the partial count is a fixed function of n and the
// partials repeat bit for bit. The residue (n % VEC) belongs to the one
// thread whose next vector would straddle n, as in adamw_k.
template <bool GRAD_BF16>
__global__ void gradnorm_part_k(const void* __restrict__ gp,
                                float* __restrict__ part, int64_t n) {
  constexpr int VEC = GRAD_BF16 ? 8 : 4;
  __shared__ float red[16];
  int64_t i = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * VEC;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x * VEC;
  float acc = 0.f;
  for (; i + VEC <= n; i += stride) {
    if (GRAD_BF16) {
      s16x8 gr = *reinterpret_cast<const s16x8*>(
          reinterpret_cast<const ushort*>(gp) + i);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float g = bf2f(ushort(gr[j]));
        acc = fmaf(g, g, acc);
      }
    } else {
      f32x4 gv = *reinterpret_cast<const f32x4*>(
          reinterpret_cast<const float*>(gp) + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = fmaf(gv[j], gv[j], acc);
    }
  }
  if (i < n && i + VEC > n)
    for (; i < n; ++i) {
      const float g = GRAD_BF16
                          ? bf2f(reinterpret_cast<const ushort*>(gp)[i])
                          : reinterpret_cast<const float*>(gp)[i];
      acc = fmaf(g, g, acc);
    }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

constexpr int CTL_THREADS = 256;

// The schedule's value at step s (counted from 1), in double.
__device__ double lr_schedule(const StepCtlArgs& a, int s) {
  if (s <= a.warmup_steps) return a.lr_max * s / a.warmup_steps;
  if (a.schedule == LR_CONSTANT) return a.lr_max;
  const int span = a.total_steps - a.warmup_steps;
  const double p =
      fmin(1.0, double(s - a.warmup_steps) / double(span > 1 ? span : 1));
  if (a.schedule == LR_LINEAR) return a.lr_max + (a.min_lr - a.lr_max) * p;
  return a.min_lr +
         0.5 * (a.lr_max - a.min_lr) * (1.0 + cos(3.141592653589793 * p));
}

// One block: the tick's job plus the step's control decisions. The partials
// are folded in double in a fixed order (strided per-thread sums, then an
// LDS tree), so the norm repeats bit for bit. part null: tick and schedule
// only (coef 1, never skips).
__global__ void __launch_bounds__(CTL_THREADS)
step_ctl_k(StepCtlArgs a) {
  __shared__ double red[CTL_THREADS];
  const int tid = threadIdx.x;
  double sum = 0.0;
  if (a.part) {
    for (int i = tid; i < a.nparts; i += CTL_THREADS) sum += double(a.part[i]);
    red[tid] = sum;
    __syncthreads();
    for (int off = CTL_THREADS / 2; off > 0; off >>= 1) {
      if (tid < off) red[tid] += red[tid + off];
      __syncthreads();
    }
    sum = red[0];
  }
  if (tid != 0) return;
  const float norm = float(sqrt(sum));
  float coef = 1.0f;
  if (a.max_norm > 0.f) {
    // clip_grad_norm_'s formula; a NaN quotient stays NaN, as it does there
    const float c = a.max_norm / (norm + 1e-6f);
    coef = c > 1.0f ? 1.0f : c;
  }
  const int skip = (a.skip_nonfinite && !__builtin_isfinite(sum)) ? 1 : 0;
  const int s = a.ctl_i[CTL_SCHED] + 1;
  a.ctl_i[CTL_SCHED] = s;
  if (!skip) {
    const int nt = a.ctl_i[CTL_T] + 1;
    a.ctl_i[CTL_T] = nt;
    a.ctl_f[CTL_BC1] = float(1.0 - pow(a.beta1, double(nt)));
    a.ctl_f[CTL_BC2] = float(1.0 - pow(a.beta2, double(nt)));
  }
  a.ctl_f[CTL_LR] = float(lr_schedule(a, s));
  a.ctl_f[CTL_COEF] = coef;
  a.ctl_f[CTL_NORM] = norm;
  a.ctl_i[CTL_SKIP_NOW] = skip;
  a.ctl_i[CTL_SKIPPED] += skip;
}

}  // namespace

int dta_gradnorm_blocks(int64_t n, bool grad_is_bf16) {
  return elementwise_grid(n, 256, grad_is_bf16 ? 8 : 4);
}

void launch_gradnorm_part(const void* grad, bool grad_is_bf16, float* part,
                          int64_t n, hipStream_t s) {
  const int grid = dta_gradnorm_blocks(n, grad_is_bf16);
  if (grad_is_bf16)
    gradnorm_part_k<true><<<grid, 256, 0, s>>>(grad, part, n);
  else
    gradnorm_part_k<false><<<grid, 256, 0, s>>>(grad, part, n);
}

void launch_step_ctl(const StepCtlArgs& a, hipStream_t s) {
  step_ctl_k<<<1, CTL_THREADS, 0, s>>>(a);
}

void launch_adamw_tick(int* t, float* bc, double beta1, double beta2,
                       hipStream_t s) {
  adamw_tick_k<<<1, 1, 0, s>>>(t, bc, beta1, beta2);
}

void launch_adamw(float* master, const void* grad, bool grad_is_bf16,
                  float* m, float* v, bf16_t* out_bf16, int step,
                  const float* bc_p, float lr, double beta1d, double beta2d,
                  float eps, float wd, int64_t n, hipStream_t s) {
  const float bc1 = bc_p ? 1.0f : float(1.0 - std::pow(beta1d, double(step)));
  const float bc2 = bc_p ? 1.0f : float(1.0 - std::pow(beta2d, double(step)));
  const float beta1 = float(beta1d), beta2 = float(beta2d);
  const float omb1 = float(1.0 - beta1d), omb2 = float(1.0 - beta2d);
  const int block = 256;
  const int grid = elementwise_grid(n, block, 4);
  auto launch = [&](auto kern) {
    kern<<<grid, block, 0, s>>>(master, grad, m, v, out_bf16, lr, beta1,
                                beta2, omb1, omb2, eps, wd, bc1, bc2, bc_p,
                                n, nullptr, nullptr);
  };
  if (grad_is_bf16)
    out_bf16 ? launch(adamw_k<true, true, false>)
             : launch(adamw_k<true, false, false>);
  else
    out_bf16 ? launch(adamw_k<false, true, false>)
             : launch(adamw_k<false, false, false>);
}

void launch_adamw_guarded(float* master, const void* grad, bool grad_is_bf16,
                          float* m, float* v, bf16_t* out_bf16,
                          const float* ctl_f, const int* ctl_i, double beta1d,
                          double beta2d, float eps, float wd, int64_t n,
                          hipStream_t s) {
  const float beta1 = float(beta1d), beta2 = float(beta2d);
  const float omb1 = float(1.0 - beta1d), omb2 = float(1.0 - beta2d);
  const int block = 256;
  const int grid = elementwise_grid(n, block, 4);
  auto launch = [&](auto kern) {
    kern<<<grid, block, 0, s>>>(master, grad, m, v, out_bf16, 0.f, beta1,
                                beta2, omb1, omb2, eps, wd, 1.0f, 1.0f,
                                nullptr, n, ctl_f, ctl_i);
  };
  if (grad_is_bf16)
    out_bf16 ? launch(adamw_k<true, true, true>)
             : launch(adamw_k<true, false, true>);
  else
    out_bf16 ? launch(adamw_k<false, true, true>)
             : launch(adamw_k<false, false, true>);
}
