// Torch glue for the gfx950 kernel library (_dta_hip extension).
// All tensor-shape/dtype validation lives here; kernels get raw pointers.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "dta_kernels.h"

namespace {

using torch::Tensor;

inline hipStream_t stream() {
  return at::hip::getCurrentHIPStream().stream();
}
inline const bf16_t* bfp(const Tensor& t) {
  return reinterpret_cast<const bf16_t*>(t.data_ptr());
}
inline bf16_t* bfp_mut(Tensor& t) {
  return reinterpret_cast<bf16_t*>(t.data_ptr());
}

void check_bf16(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}
void check_f32(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// ---- dropout parameters ----------------------------------------------------
// p == 0 disables (defaults); else rng must be the int64 [1] device step
// counter. The quantisation of p lives in dta_kernels.h.
DropParams drop_params(const Tensor& rng, int64_t site, double p) {
  DropParams d;
  if (p > 0.0) {
    TORCH_CHECK(p < 1.0, "dropout p must be < 1");
    TORCH_CHECK(rng.numel() == 1 && rng.scalar_type() == torch::kInt64 &&
                    rng.is_cuda(), "rng must be an int64 [1] GPU counter");
    d.rng = reinterpret_cast<const unsigned long long*>(
        rng.data_ptr<int64_t>());
    d.site = (unsigned long long)site;
    dta_drop_quantize(p, d);
  }
  return d;
}

// ---- column-reduction destinations -----------------------------------------
// Optional trailing argument of colsum / *norm_bwd / gelu_bwd_colsum: a bf16
// [cols] gradient view (a flat-plane slice, any alignment) the reduction
// accumulates into instead of returning an fp32 tensor.
using OptTensor = c10::optional<Tensor>;
bf16_t* grad_dst(OptTensor& d, int64_t cols, const char* name) {
  if (!d.has_value() || !d->defined()) return nullptr;
  check_bf16(*d, name);
  TORCH_CHECK(d->numel() == cols, name, " must have cols elements");
  return bfp_mut(*d);
}

// ---- norms ----------------------------------------------------------------
// LayerNorm and RMSNorm share one implementation per direction; b == null
// selects RMSNorm (no bias, no mean).
int norm_cols(const Tensor& x, int max_cols, const char* what) {
  check_bf16(x, "x");
  TORCH_CHECK(x.size(1) % 8 == 0, "cols must be a multiple of 8");
  TORCH_CHECK(x.size(1) <= max_cols, what, " supports cols <= ", max_cols,
              " (register-resident row)");
  return int(x.size(1));
}

// res: empty tensor => plain norm; else fused residual (returns the bf16
// sum as an extra output feeding the ongoing residual stream). p > 0:
// the branch is dropout-ed BEFORE the add (sum = x + drop(res)).
// Returns {y, mean (undefined for RMS), rstd, sum}.
std::vector<Tensor> norm_fwd(Tensor x, Tensor res, Tensor w, const Tensor* b,
                             double eps, Tensor rng, int64_t site, double p) {
  const int cols = norm_cols(x, DTA_NORM_FWD_MAX_COLS, "norm forward");
  check_bf16(w, "w");
  if (b) check_bf16(*b, "b");
  const int64_t rows = x.size(0);
  const bool has_res = res.numel() > 0;
  if (has_res) check_bf16(res, "res");
  TORCH_CHECK(p == 0.0 || has_res, "dropout needs the residual branch");
  const DropParams drop = drop_params(rng, site, p);
  const auto f32 = x.options().dtype(torch::kFloat32);
  auto y = torch::empty_like(x);
  auto sum = has_res ? torch::empty_like(x) : torch::empty({0}, x.options());
  Tensor mean = b ? torch::empty({rows}, f32) : Tensor();
  auto rstd = torch::empty({rows}, f32);
  launch_norm_fwd({bfp(x), has_res ? bfp(res) : nullptr,
                   has_res ? bfp_mut(sum) : nullptr, bfp(w),
                   b ? bfp(*b) : nullptr, bfp_mut(y),
                   b ? mean.data_ptr<float>() : nullptr,
                   rstd.data_ptr<float>(), rows, cols, float(eps), drop, !b},
                  stream());
  return {y, mean, rstd, sum};
}

// ds: empty tensor => plain; else the gradient arriving on the sum
// stream, folded into dx (dx = ds + dNorm/dx). p > 0: also emits
// dres = dx ⊙ mask/(1-p) for the dropped branch.
// Returns {dx, dw32, db32 (undefined for RMS), dres}; fp32 grads: the ops
// layer casts. dw_dst / db_dst: accumulate that gradient into the bf16
// destination instead (its fp32 tensor is then undefined).
std::vector<Tensor> norm_bwd(Tensor dy, Tensor ds, Tensor x, Tensor w,
                             const Tensor* mean, Tensor rstd, Tensor rng,
                             int64_t site, double p, OptTensor dw_dst,
                             OptTensor db_dst) {
  const int cols = norm_cols(x, DTA_NORM_BWD_MAX_COLS, "norm backward");
  check_bf16(dy, "dy"); check_bf16(w, "w");
  const int64_t rows = x.size(0);
  const bool has_ds = ds.numel() > 0;
  if (has_ds) check_bf16(ds, "ds");
  const DropParams drop = drop_params(rng, site, p);
  auto dx = torch::empty_like(x);
  auto dres = drop.thr16 ? torch::empty_like(x)
                         : torch::empty({0}, x.options());
  const auto f32 = x.options().dtype(torch::kFloat32);
  bf16_t* dwd = grad_dst(dw_dst, cols, "dw_dst");
  bf16_t* dbd = mean ? grad_dst(db_dst, cols, "db_dst") : nullptr;
  Tensor dw32 = dwd ? Tensor() : torch::empty({cols}, f32);
  Tensor db32 = (mean && !dbd) ? torch::empty({cols}, f32) : Tensor();
  const int stripes = dta_norm_bwd_stripes(rows, cols);
  auto part = torch::empty({mean ? 2 : 1, stripes, cols}, f32);
  launch_norm_bwd({bfp(dy), has_ds ? bfp(ds) : nullptr, bfp(x), bfp(w),
                   mean ? mean->data_ptr<float>() : nullptr,
                   rstd.data_ptr<float>(), bfp_mut(dx),
                   drop.thr16 ? bfp_mut(dres) : nullptr,
                   dwd ? nullptr : dw32.data_ptr<float>(),
                   db32.defined() ? db32.data_ptr<float>() : nullptr,
                   part[0].data_ptr<float>(),
                   mean ? part[1].data_ptr<float>() : nullptr, dwd, dbd,
                   stripes, rows,
                   cols, drop, !mean},
                  stream());
  return {dx, dw32, db32, dres};
}

std::vector<Tensor> layernorm_fwd(Tensor x, Tensor res, Tensor w, Tensor b,
                                  double eps, Tensor rng, int64_t site,
                                  double p) {
  return norm_fwd(x, res, w, &b, eps, rng, site, p);
}
std::vector<Tensor> layernorm_bwd(Tensor dy, Tensor ds, Tensor x, Tensor w,
                                  Tensor mean, Tensor rstd, Tensor rng,
                                  int64_t site, double p, OptTensor dw_dst,
                                  OptTensor db_dst) {
  return norm_bwd(dy, ds, x, w, &mean, rstd, rng, site, p, dw_dst, db_dst);
}
std::vector<Tensor> rmsnorm_fwd(Tensor x, Tensor res, Tensor w, double eps,
                                Tensor rng, int64_t site, double p) {
  auto o = norm_fwd(x, res, w, nullptr, eps, rng, site, p);
  return {o[0], o[2], o[3]};  // y, rstd, sum
}
std::vector<Tensor> rmsnorm_bwd(Tensor dy, Tensor ds, Tensor x, Tensor w,
                                Tensor rstd, Tensor rng, int64_t site,
                                double p, OptTensor dw_dst) {
  auto o = norm_bwd(dy, ds, x, w, nullptr, rstd, rng, site, p, dw_dst,
                    c10::nullopt);
  return {o[0], o[1], o[3]};  // dx, dw32, dres
}

// ---- elementwise ----------------------------------------------------------
Tensor gelu_fwd(Tensor x) {
  auto y = torch::empty_like(x);
  if (x.scalar_type() == torch::kBFloat16) {
    check_bf16(x, "x");
    launch_gelu_fwd(bfp(x), bfp_mut(y), x.numel(), stream());
  } else {
    check_f32(x, "x");
    launch_gelu_fwd_f32(x.data_ptr<float>(), y.data_ptr<float>(), x.numel(),
                        stream());
  }
  return y;
}
Tensor gelu_bwd(Tensor dy, Tensor x) {
  auto dx = torch::empty_like(x);
  if (x.scalar_type() == torch::kBFloat16) {
    check_bf16(x, "x"); check_bf16(dy, "dy");
    launch_gelu_bwd(bfp(dy), bfp(x), bfp_mut(dx), x.numel(), stream());
  } else {
    launch_gelu_bwd_f32(dy.data_ptr<float>(), x.data_ptr<float>(),
                        dx.data_ptr<float>(), x.numel(), stream());
  }
  return dx;
}
Tensor swiglu_fwd(Tensor g, Tensor u) {
  check_bf16(g, "gate"); check_bf16(u, "up");
  auto y = torch::empty_like(g);
  launch_swiglu_fwd(bfp(g), bfp(u), bfp_mut(y), g.numel(), stream());
  return y;
}
// counter-based dropout: y = x ⊙ mask / keep. The same call with the same
// (rng value, site) regenerates the identical mask — backward is this very
// function applied to dy (no stored mask).
Tensor dropout_apply(Tensor x, Tensor rng, int64_t site, double p) {
  check_bf16(x, "x");
  TORCH_CHECK(p > 0.0 && p < 1.0, "dropout p must be in (0,1)");
  const DropParams drop = drop_params(rng, site, p);
  auto y = torch::empty_like(x);
  launch_dropout(bfp(x), bfp_mut(y), x.numel(), drop, stream());
  return y;
}

// dst must be a CONTIGUOUS bf16 view (a flat-grad slice); src fp32
void accum_f32_into_bf16(Tensor dst, Tensor src) {
  check_bf16(dst, "dst"); check_f32(src, "src");
  TORCH_CHECK(dst.numel() == src.numel(), "size mismatch");
  launch_accum_f32_bf16(bfp_mut(dst), src.data_ptr<float>(), dst.numel(),
                        stream());
}

void rng_tick(Tensor ctr) {
  TORCH_CHECK(ctr.numel() == 1 && ctr.scalar_type() == torch::kInt64 &&
                  ctr.is_cuda(), "ctr must be an int64 [1] GPU counter");
  launch_rng_tick(reinterpret_cast<unsigned long long*>(
                      ctr.data_ptr<int64_t>()), stream());
}

std::vector<Tensor> swiglu_bwd(Tensor dy, Tensor g, Tensor u) {
  check_bf16(dy, "dy");
  auto dg = torch::empty_like(g);
  auto du = torch::empty_like(u);
  launch_swiglu_bwd(bfp(dy), bfp(g), bfp(u), bfp_mut(dg), bfp_mut(du),
                    g.numel(), stream());
  return {dg, du};
}

// ---- flat plane ------------------------------------------------------------
void delta_sub(Tensor w, Tensor base, Tensor out) {
  check_f32(w, "w"); check_f32(base, "base"); check_f32(out, "out");
  launch_delta_sub(w.data_ptr<float>(), base.data_ptr<float>(),
                   out.data_ptr<float>(), w.numel(), stream());
}
void axpy(Tensor w, Tensor x, double alpha) {
  check_f32(w, "w"); check_f32(x, "x");
  launch_axpy(w.data_ptr<float>(), x.data_ptr<float>(), float(alpha),
              w.numel(), stream());
}
bool has_nan(Tensor x) {
  check_f32(x, "x");
  auto flag = torch::zeros({1}, x.options().dtype(torch::kInt32));
  launch_nan_any(x.data_ptr<float>(), x.numel(), flag.data_ptr<int>(),
                 stream());
  return flag.item<int>() != 0;
}
double l2norm_sq(Tensor x) {
  check_f32(x, "x");
  auto out = torch::zeros({1}, x.options());
  launch_l2norm_sq(x.data_ptr<float>(), x.numel(), out.data_ptr<float>(),
                   stream());
  return out.item<float>();
}

// bc: empty tensor => host bias-correction from 'step'; else a fp32[2]
// device buffer maintained by adamw_tick (hipGraph-capturable path).
void adamw_step(Tensor master, Tensor grad, Tensor m, Tensor v,
                Tensor out_bf16, int64_t step, double lr, double beta1,
                double beta2, double eps, double wd, Tensor bc) {
  check_f32(master, "master"); check_f32(m, "m"); check_f32(v, "v");
  const bool gb = grad.scalar_type() == torch::kBFloat16;
  bf16_t* outp = out_bf16.numel() ? bfp_mut(out_bf16) : nullptr;
  const float* bcp = bc.numel() ? bc.data_ptr<float>() : nullptr;
  launch_adamw(master.data_ptr<float>(), grad.data_ptr(), gb,
               m.data_ptr<float>(), v.data_ptr<float>(), outp, int(step),
               bcp, float(lr), beta1, beta2, float(eps), float(wd),
               master.numel(), stream());
}

void adamw_tick(Tensor t, Tensor bc, double beta1, double beta2) {
  TORCH_CHECK(t.scalar_type() == torch::kInt32 && t.is_cuda(), "t int32 gpu");
  check_f32(bc, "bc");
  launch_adamw_tick(t.data_ptr<int>(), bc.data_ptr<float>(), beta1, beta2,
                    stream());
}

// ---- guarded step: norm partials -> control block -> AdamW ------------------
// None of the three syncs or allocates; all are graph-capturable.
bool flat_grad_is_bf16(const Tensor& g, const char* name) {
  TORCH_CHECK(g.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(g.is_contiguous(), name, " must be contiguous");
  const bool gb = g.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(gb || g.scalar_type() == torch::kFloat32, name,
              " must be bf16 or fp32");
  return gb;
}
void check_ctl(const Tensor& ctl_f, const Tensor& ctl_i, const Tensor& like) {
  check_f32(ctl_f, "ctl_f");
  TORCH_CHECK(ctl_f.numel() == 6, "ctl_f must be fp32[6]");
  TORCH_CHECK(ctl_i.is_cuda() && ctl_i.scalar_type() == torch::kInt32 &&
                  ctl_i.is_contiguous() && ctl_i.numel() == 4,
              "ctl_i must be a contiguous int32[4] on GPU");
  TORCH_CHECK(ctl_f.device() == like.device() &&
                  ctl_i.device() == like.device(),
              "control block must be on the device of the plane");
}
int64_t grad_sumsq_blocks(int64_t n, bool is_bf16) {
  TORCH_CHECK(n >= 1, "empty plane");
  return dta_gradnorm_blocks(n, is_bf16);
}
void grad_sumsq_partials(Tensor flat, Tensor out) {
  const bool gb = flat_grad_is_bf16(flat, "flat");
  TORCH_CHECK(flat.numel() >= 1, "empty plane");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(flat.data_ptr()) % 16 == 0,
              "flat must be 16 B aligned");
  check_f32(out, "out");
  TORCH_CHECK(out.device() == flat.device(), "out must be on flat's device");
  TORCH_CHECK(out.numel() == dta_gradnorm_blocks(flat.numel(), gb),
              "out must have grad_sumsq_blocks(n) elements");
  launch_gradnorm_part(flat.data_ptr(), gb, out.data_ptr<float>(),
                       flat.numel(), stream());
}
// part: empty tensor => tick + schedule only
void step_control(Tensor part, Tensor ctl_f, Tensor ctl_i, double beta1,
                  double beta2, double max_norm, bool skip_nonfinite,
                  int64_t schedule, double lr_max, double min_lr,
                  int64_t warmup_steps, int64_t total_steps) {
  check_ctl(ctl_f, ctl_i, ctl_f);
  const bool has_part = part.numel() > 0;
  if (has_part) {
    check_f32(part, "part");
    TORCH_CHECK(part.device() == ctl_f.device(),
                "part must be on the control block's device");
  }
  TORCH_CHECK(has_part || (max_norm <= 0.0 && !skip_nonfinite),
              "clipping and the non-finite skip need the norm partials");
  TORCH_CHECK(part.numel() <= (int64_t(1) << 30), "too many partials");
  TORCH_CHECK(schedule >= LR_CONSTANT && schedule <= LR_COSINE,
              "unknown schedule");
  TORCH_CHECK(warmup_steps >= 0 && warmup_steps < (int64_t(1) << 31) &&
                  total_steps >= 0 && total_steps < (int64_t(1) << 31),
              "warmup_steps / total_steps out of range");
  TORCH_CHECK(schedule == LR_CONSTANT || total_steps > warmup_steps,
              "linear / cosine need total_steps > warmup_steps");
  launch_step_ctl({has_part ? part.data_ptr<float>() : nullptr,
                   int(part.numel()), ctl_f.data_ptr<float>(),
                   ctl_i.data_ptr<int>(), beta1, beta2, float(max_norm),
                   skip_nonfinite ? 1 : 0, int(schedule), lr_max, min_lr,
                   int(warmup_steps), int(total_steps)},
                  stream());
}
void adamw_step_guarded(Tensor master, Tensor grad, Tensor m, Tensor v,
                        Tensor out_bf16, Tensor ctl_f, Tensor ctl_i,
                        double beta1, double beta2, double eps, double wd) {
  check_f32(master, "master"); check_f32(m, "m"); check_f32(v, "v");
  const bool gb = flat_grad_is_bf16(grad, "grad");
  const int64_t n = master.numel();
  TORCH_CHECK(grad.numel() == n && m.numel() == n && v.numel() == n,
              "master, grad, m and v must have one length");
  TORCH_CHECK(grad.device() == master.device() &&
                  m.device() == master.device() &&
                  v.device() == master.device(), "planes on one device");
  check_ctl(ctl_f, ctl_i, master);
  bf16_t* outp = nullptr;
  if (out_bf16.numel()) {
    check_bf16(out_bf16, "out_bf16");
    TORCH_CHECK(out_bf16.numel() == n && out_bf16.device() == master.device(),
                "out_bf16 must match master");
    outp = bfp_mut(out_bf16);
  }
  launch_adamw_guarded(master.data_ptr<float>(), grad.data_ptr(), gb,
                       m.data_ptr<float>(), v.data_ptr<float>(), outp,
                       ctl_f.data_ptr<float>(), ctl_i.data_ptr<int>(), beta1,
                       beta2, float(eps), float(wd), n, stream());
}

// column sum of a [rows, cols] bf16 matrix -> fp32 [cols] (bias gradient),
// or accumulated into dst (nothing returned)
Tensor colsum(Tensor x, OptTensor dst) {
  check_bf16(x, "x");
  TORCH_CHECK(x.dim() == 2 && x.size(1) >= 1, "x must be [rows, cols]");
  const int64_t rows = x.size(0);
  const int cols = int(x.size(1));
  const int stripes = dta_colred_stripes(rows, cols);
  auto f32 = x.options().dtype(torch::kFloat32);
  auto part = torch::empty({stripes, dta_colred_ld(cols)}, f32);
  bf16_t* d = grad_dst(dst, cols, "dst");
  Tensor out = d ? Tensor() : torch::empty({cols}, f32);
  launch_colsum(bfp(x), part.data_ptr<float>(),
                d ? nullptr : out.data_ptr<float>(), d, rows, cols, stripes,
                stream());
  return out;
}

// {dx, db32}: dx = gelu_bwd(dy, x) bit for bit, db32 = colsum(dx) up to the
// order of the fp32 sum, from one pass over [rows, cols] bf16 where
// cols % 8 == 0 (else gelu_bwd then colsum). db_dst as colsum's dst.
// stripes > 0 overrides the automatic row-stripe count (measurement only).
std::vector<Tensor> gelu_bwd_colsum(Tensor dy, Tensor x, OptTensor db_dst,
                                    int64_t stripes_arg) {
  check_bf16(x, "x"); check_bf16(dy, "dy");
  TORCH_CHECK(x.dim() == 2 && dy.sizes() == x.sizes(),
              "dy, x must be [rows, cols]");
  const int64_t rows = x.size(0);
  const int cols = int(x.size(1));
  if (cols % 8 != 0) {
    auto dx = gelu_bwd(dy, x);
    return {dx, colsum(dx, db_dst)};
  }
  const int stripes =
      stripes_arg > 0 ? int(std::min<int64_t>(stripes_arg, 65535))
                      : dta_gelu_colsum_stripes(rows, cols);
  auto f32 = x.options().dtype(torch::kFloat32);
  auto dx = torch::empty_like(x);
  auto part = torch::empty({stripes, cols}, f32);
  bf16_t* d = grad_dst(db_dst, cols, "db_dst");
  Tensor out = d ? Tensor() : torch::empty({cols}, f32);
  launch_gelu_bwd_colsum(bfp(dy), bfp(x), bfp_mut(dx),
                         part.data_ptr<float>(),
                         d ? nullptr : out.data_ptr<float>(), d, rows, cols,
                         stripes, stream());
  return {dx, out};
}

// ---- weight gradient with the bias sum folded in (wgrad.hip) ---------------
// The shape contract of wgrad_bias, in one place: dy [T, out] and x [T, in]
// bf16 with unit column stride, row strides % 8 == 0 (the packed-qkv views
// have a row stride larger than their width), 16 B aligned bases, T >= 1,
// out a multiple of the tile's rows and in of its columns.
const char* wgrad_reject(const Tensor& dy, const Tensor& x) {
  if (!(dy.is_cuda() && x.is_cuda() && dy.device() == x.device()))
    return "dy and x must be on one GPU";
  if (dy.scalar_type() != torch::kBFloat16 ||
      x.scalar_type() != torch::kBFloat16)
    return "dy and x must be bf16";
  if (dy.dim() != 2 || x.dim() != 2 || dy.size(0) != x.size(0))
    return "dy must be [T, out] and x [T, in]";
  const int64_t T = dy.size(0), out = dy.size(1), in = x.size(1);
  if (T < 1 || T >= (int64_t(1) << 31)) return "T out of range";
  if (out < DTA_WGRAD_BM || out % DTA_WGRAD_BM != 0 || in < DTA_WGRAD_BN ||
      in % DTA_WGRAD_BN != 0 || out * in >= (int64_t(1) << 31))
    return "out / in must be multiples of the tile";
  if (dy.stride(1) != 1 || x.stride(1) != 1) return "unit column stride";
  // T == 1: the row stride is never used
  const int64_t lda = T > 1 ? dy.stride(0) : out, ldb = T > 1 ? x.stride(0) : in;
  if (lda < out || ldb < in || lda % 8 != 0 || ldb % 8 != 0 ||
      lda >= (int64_t(1) << 25) || ldb >= (int64_t(1) << 25))
    return "row strides must be >= the width, % 8 == 0 and < 2^25";
  if (reinterpret_cast<uintptr_t>(dy.data_ptr()) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 != 0)
    return "16-byte aligned operands";
  return nullptr;
}
bool wgrad_supported(Tensor dy, Tensor x) { return !wgrad_reject(dy, x); }
std::vector<int64_t> wgrad_tile() {
  return {DTA_WGRAD_BM, DTA_WGRAD_BN, DTA_WGRAD_BK};
}
int64_t wgrad_nsplit(int64_t T, int64_t out, int64_t in) {
  return dta_wgrad_nsplit(
      T, out, in, at::cuda::getCurrentDeviceProperties()->multiProcessorCount);
}

// dw = bf16(float(dw) + dy^T x) on the MFMA units, split over T and folded in
// a fixed order (bit-repeatable); dw: bf16 [out, in] contiguous gradient view
// of any alignment. The bias sum over t comes from the same pass over dy:
// db given -> db = bf16(float(db) + sum), nothing returned; else bias_f32 ->
// an fp32 [out] tensor is returned; else no bias is computed. nsplit 0: the
// automatic split. Capturable: workspaces from the allocator, no host sync.
Tensor wgrad_bias(Tensor dy, Tensor x, Tensor dw, OptTensor db, bool bias_f32,
                  int64_t nsplit) {
  const char* why = wgrad_reject(dy, x);
  TORCH_CHECK(!why, "wgrad_bias: ", why ? why : "");
  const int64_t T = dy.size(0), out = dy.size(1), in = x.size(1);
  check_bf16(dw, "dw");
  TORCH_CHECK(dw.device() == dy.device() && dw.dim() == 2 &&
                  dw.size(0) == out && dw.size(1) == in,
              "dw must be a contiguous bf16 [out, in] view on dy's device");
  bf16_t* dbp = grad_dst(db, out, "db");
  TORCH_CHECK(!dbp || db->device() == dy.device(), "db must be on dy's device");
  TORCH_CHECK(nsplit >= 0, "nsplit must be >= 0");
  // a forced count beyond the K-steps is legal: empty slices store zeros
  const int ns = nsplit == 0 ? int(wgrad_nsplit(T, out, in))
                             : int(std::min<int64_t>(nsplit, 1024));
  const bool bias = dbp || bias_f32;
  const auto f32 = dy.options().dtype(torch::kFloat32);
  auto slab = torch::empty({int64_t(ns), out, in}, f32);
  Tensor bpart = bias ? torch::empty({int64_t(ns), out}, f32) : Tensor();
  Tensor bout = (bias && !dbp) ? torch::empty({out}, f32) : Tensor();
  WgradArgs a;
  a.dy = bfp(dy); a.x = bfp(x);
  a.ld_dy = T > 1 ? dy.stride(0) : out;
  a.ld_x = T > 1 ? x.stride(0) : in;
  a.T = T; a.out = int(out); a.in = int(in); a.nsplit = ns;
  a.slab = slab.data_ptr<float>();
  a.bpart = bias ? bpart.data_ptr<float>() : nullptr;
  a.dw = bfp_mut(dw);
  a.db = dbp;
  a.bout = bout.defined() ? bout.data_ptr<float>() : nullptr;
  launch_wgrad(a, stream());
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "wgrad launch failed: ",
              hipGetErrorString(err));
  return bout;
}

// ---- merge plane -----------------------------------------------------------
// What every merge entry point, fp32 or packed, requires of its tables
// before anything is launched. offsets: an integer [n_segs + 1] table; the
// kernels read int64, so an int32 table is converted, never reinterpreted.
int merge_n_models(int64_t n) {
  TORCH_CHECK(n >= 1 && n <= DTA_MERGE_MAX_MODELS,
              "merge: 1 <= n_models <= ", DTA_MERGE_MAX_MODELS);
  return int(n);
}
int merge_n_segs(const Tensor& offsets) {
  TORCH_CHECK(offsets.dim() == 1 && offsets.numel() >= 2 &&
                  (offsets.scalar_type() == torch::kInt64 ||
                   offsets.scalar_type() == torch::kInt32),
              "offsets must be an int64 or int32 [n_segs + 1] tensor");
  TORCH_CHECK(offsets.numel() <= int64_t(DTA_MERGE_LDS_LIMIT / 8),
              "offsets do not fit the LDS budget of ", DTA_MERGE_LDS_LIMIT,
              " B");
  return int(offsets.numel() - 1);
}
Tensor merge_offsets(const Tensor& offsets, const Tensor& base) {
  return offsets.to(base.device(), torch::kInt64).contiguous();
}
// W [n_models, n_segs] as fp32 on base's device; it and the offsets must fit
// the dynamic LDS weighted_merge_k caches them in
Tensor merge_weights(const Tensor& W, const Tensor& base, int n_models,
                     int n_segs) {
  TORCH_CHECK(W.dim() == 2 && W.size(0) == n_models && W.size(1) == n_segs,
              "W must be [n_models, n_segs]");
  TORCH_CHECK(dta_merge_shmem(n_models, n_segs) <= DTA_MERGE_LDS_LIMIT,
              "offsets + W ([", n_models, ", ", n_segs,
              "]) do not fit the LDS budget of ", DTA_MERGE_LDS_LIMIT, " B");
  return W.to(base.device(), torch::kFloat32).contiguous();
}
// an fp32 plane of P elements. The fp32 kernels read one element per lane,
// so unlike the packed ones (check_plane) they ask for no 16-byte alignment
void check_plane_f32(const Tensor& t, int64_t P, const char* name) {
  check_f32(t, name);
  TORCH_CHECK(t.numel() == P, name, " must have P elements");
}
int check_deltas_f32(const Tensor& deltas, int64_t P) {
  check_f32(deltas, "deltas");
  TORCH_CHECK(P >= 1 && deltas.dim() == 2 && deltas.size(1) == P,
              "deltas must be [N, P]");
  return merge_n_models(deltas.size(0));
}

void weighted_merge(Tensor base, Tensor deltas, Tensor W, Tensor offsets,
                    Tensor out) {
  const int64_t P = base.numel();
  check_plane_f32(base, P, "base"); check_plane_f32(out, P, "out");
  const int n_models = check_deltas_f32(deltas, P);
  const int n_segs = merge_n_segs(offsets);
  auto Wc = merge_weights(W, base, n_models, n_segs);
  auto offs = merge_offsets(offsets, base);
  launch_weighted_merge(base.data_ptr<float>(), deltas.data_ptr<float>(),
                        Wc.data_ptr<float>(), offs.data_ptr<int64_t>(),
                        n_models, n_segs, P, out.data_ptr<float>(), stream());
}

// boundary-aligned chunk table for grad_W: [n_chunks, 3] int64 rows
// (start, end, seg) on base's device, none crossing a segment, <= 1M
// elements each. The offsets must tile [0, P): the kernel reads every
// element between a chunk's start and end.
Tensor grad_w_chunks(const Tensor& offsets, const Tensor& base, int n_segs) {
  auto offs_cpu = offsets.to(torch::kCPU, torch::kInt64).contiguous();
  const int64_t* op = offs_cpu.data_ptr<int64_t>();
  TORCH_CHECK(op[0] == 0 && op[n_segs] == base.numel(),
              "offsets must run from 0 to P");
  for (int j = 0; j < n_segs; ++j)
    TORCH_CHECK(op[j] <= op[j + 1], "offsets must not decrease");
  std::vector<int64_t> chunks;
  constexpr int64_t CH = 1 << 20;
  for (int j = 0; j < n_segs; ++j)
    for (int64_t s0 = op[j]; s0 < op[j + 1]; s0 += CH) {
      chunks.push_back(s0);
      chunks.push_back(std::min(s0 + CH, op[j + 1]));
      chunks.push_back(j);
    }
  // a blocking copy: the vector may die with this frame
  return torch::from_blob(chunks.data(), {int64_t(chunks.size())},
                          torch::kInt64)
      .to(base.device());
}

// g: the bf16 or fp32 [P] gradient plane both grad_W entry points read
bool check_grad_plane(const Tensor& g, int64_t P) {
  const bool gb = g.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(g.is_cuda() && g.is_contiguous() && g.numel() == P &&
                  (gb || g.scalar_type() == torch::kFloat32),
              "g must be a contiguous bf16/fp32 [P] GPU tensor");
  return gb;
}

Tensor grad_merge_weights(Tensor g, Tensor base, Tensor deltas, Tensor merged,
                          Tensor offsets) {
  const int64_t P = base.numel();
  check_plane_f32(base, P, "base"); check_plane_f32(merged, P, "merged");
  const bool gb = check_grad_plane(g, P);
  const int n_models = check_deltas_f32(deltas, P);
  const int n_segs = merge_n_segs(offsets);
  auto ch = grad_w_chunks(offsets, base, n_segs);
  const int n_chunks = int(ch.numel() / 3);
  auto gw = torch::zeros({n_models, n_segs},
                         base.options().dtype(torch::kFloat32));
  launch_grad_merge_weights(g.data_ptr(), gb, base.data_ptr<float>(),
                            deltas.data_ptr<float>(),
                            merged.data_ptr<float>(),
                            ch.data_ptr<int64_t>(), n_models, n_chunks, P,
                            gw.data_ptr<float>(), n_segs, stream());
  return gw;
}

// ---- packed deltas (bf16, or int8 codes + scales) ---------------------------
bool aligned16(const Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// data [N, P] bf16 with scales empty, or data [N, nb*block] int8 with scales
// [N, nb] fp32; P is the length of a dequantised row.
PackedView packed_view(const Tensor& data, const Tensor& scales, int64_t P,
                       int64_t block) {
  TORCH_CHECK(data.is_cuda() && data.dim() == 2 && data.is_contiguous(),
              "packed data must be a contiguous [N, cols] GPU tensor");
  TORCH_CHECK(data.size(0) >= 1 && data.size(0) <= DTA_MERGE_MAX_MODELS,
              "packed deltas: 1 <= n_models <= ", DTA_MERGE_MAX_MODELS);
  TORCH_CHECK(aligned16(data), "packed data must be 16-byte aligned");
  TORCH_CHECK(P >= 1, "packed deltas: empty plane");
  if (data.scalar_type() == torch::kBFloat16) {
    TORCH_CHECK(data.size(1) == P, "bf16 deltas must be [N, P]");
    return PackedView{data.data_ptr(), nullptr, P, 0, 0, DELTA_BF16};
  }
  TORCH_CHECK(data.scalar_type() == torch::kInt8,
              "packed data must be bf16 or int8");
  TORCH_CHECK(block >= DTA_QUANT_MIN_BLOCK && block <= DTA_QUANT_MAX_BLOCK &&
                  (block & (block - 1)) == 0,
              "block must be a power of two in [", DTA_QUANT_MIN_BLOCK, ", ",
              DTA_QUANT_MAX_BLOCK, "]");
  const int64_t nb = (P + block - 1) / block;
  TORCH_CHECK(data.size(1) == nb * block,
              "int8 codes must be [N, nb*block], nb = ceil(P / block)");
  check_f32(scales, "scales");
  TORCH_CHECK(scales.dim() == 2 && scales.size(0) == data.size(0) &&
                  scales.size(1) == nb, "scales must be [N, nb]");
  int shift = 0;
  while ((int64_t(1) << shift) < block) ++shift;
  return PackedView{data.data_ptr(), scales.data_ptr<float>(), nb * block, nb,
                    shift, DELTA_I8};
}

void check_plane(const Tensor& t, int64_t P, const char* name) {
  check_f32(t, name);
  TORCH_CHECK(t.numel() == P, name, " must have P elements");
  TORCH_CHECK(aligned16(t), name, " must be 16-byte aligned");
}

// ---- top-k deltas ----------------------------------------------------------
// The fourth wire form has no export names of its own: the packed entry
// points below take int32 entries as they take bf16 or int8 data (k is
// data.size(1) / nb), and quantize_int8 makes them when topk_k > 0.
bool is_topk(const Tensor& data) {
  return data.scalar_type() == torch::kInt32;
}
// entries per block of int32 [N, nb*k] data; topk_view checks the rest
int64_t topk_k_of(const Tensor& data, int64_t P, int64_t block) {
  TORCH_CHECK(data.dim() == 2 && P >= 1 && block >= 1,
              "topk entries must be [N, nb*k]");
  return data.size(1) / ((P + block - 1) / block);
}
// the format's limits (comm.check_topk_format); returns nb
int64_t check_topk_format(int64_t P, int64_t k, int64_t block) {
  TORCH_CHECK(P >= 1, "topk deltas: empty plane");
  TORCH_CHECK(block >= DTA_TOPK_MIN_BLOCK && block <= DTA_TOPK_MAX_BLOCK &&
                  (block & (block - 1)) == 0,
              "topk block must be a power of two in [", DTA_TOPK_MIN_BLOCK,
              ", ", DTA_TOPK_MAX_BLOCK, "]");
  TORCH_CHECK(k >= 4 && k % 4 == 0 && k <= block / 4,
              "topk k must be a multiple of 4 in [4, block / 4]");
  const int64_t nb = (P + block - 1) / block;
  TORCH_CHECK(nb < (int64_t(1) << 31), "too many top-k blocks");
  return nb;
}

// data: int32 [N, nb*k] entries of N rows of a P-element plane
TopkView topk_view(const Tensor& data, int64_t P, int64_t k, int64_t block) {
  const int64_t nb = check_topk_format(P, k, block);
  TORCH_CHECK(data.is_cuda() && data.dim() == 2 && data.is_contiguous() &&
                  data.scalar_type() == torch::kInt32,
              "topk entries must be a contiguous int32 [N, nb*k] GPU tensor");
  TORCH_CHECK(data.size(0) >= 1 && data.size(0) <= DTA_MERGE_MAX_MODELS,
              "topk deltas: 1 <= n_models <= ", DTA_MERGE_MAX_MODELS);
  TORCH_CHECK(data.size(1) == nb * k,
              "topk entries must be [N, nb*k], nb = ceil(P / block)");
  TORCH_CHECK(aligned16(data), "topk entries must be 16-byte aligned");
  int shift = 0;
  while ((int64_t(1) << shift) < block) ++shift;
  return TopkView{data.data_ptr<int>(), nb * k, shift, int(k)};
}

// entries [nb*k] of (x - base) + residual_in; base / residual_in /
// residual_out empty: not used / not used / not written
Tensor topk_compress(Tensor x, Tensor base, Tensor residual_in,
                     Tensor residual_out, int64_t k, int64_t block) {
  check_f32(x, "x");
  const int64_t P = x.numel();
  const int64_t nb = check_topk_format(P, k, block);
  TORCH_CHECK(aligned16(x), "x must be 16-byte aligned");
  const float *bp = nullptr, *rin = nullptr;
  float* rout = nullptr;
  if (base.numel()) {
    check_plane(base, P, "base");
    bp = base.data_ptr<float>();
  }
  if (residual_in.numel()) {
    check_plane(residual_in, P, "residual_in");
    rin = residual_in.data_ptr<float>();
  }
  if (residual_out.numel()) {
    check_plane(residual_out, P, "residual_out");
    rout = residual_out.data_ptr<float>();
  }
  auto entries = torch::empty({nb * k}, x.options().dtype(torch::kInt32));
  launch_delta_topk(x.data_ptr<float>(), bp, rin, rout, P, int(block), int(k),
                    nb, entries.data_ptr<int>(), stream());
  return entries;
}

void weighted_merge_topk(Tensor base, Tensor data, int64_t k, int64_t block,
                         Tensor W, Tensor offsets, Tensor out) {
  const int64_t P = base.numel();
  check_plane(base, P, "base"); check_plane(out, P, "out");
  const TopkView d = topk_view(data, P, k, block);
  const int n_models = merge_n_models(data.size(0));
  const int n_segs = merge_n_segs(offsets);
  auto Wc = merge_weights(W, base, n_models, n_segs);
  TORCH_CHECK(dta_topk_merge_shmem(n_models, n_segs, int(block)) <=
                  DTA_MERGE_LDS_LIMIT,
              "topk merge: tiles + offsets + W do not fit the LDS budget of ",
              DTA_MERGE_LDS_LIMIT, " B");
  auto offs = merge_offsets(offsets, base);
  launch_weighted_merge_topk(base.data_ptr<float>(), d, Wc.data_ptr<float>(),
                             offs.data_ptr<int64_t>(), n_models, n_segs, P,
                             out.data_ptr<float>(), stream());
}

Tensor grad_merge_weights_topk(Tensor g, Tensor base, Tensor data, int64_t k,
                               int64_t block, Tensor merged, Tensor offsets) {
  const int64_t P = base.numel();
  check_plane(base, P, "base"); check_plane(merged, P, "merged");
  const bool gb = check_grad_plane(g, P);
  const TopkView d = topk_view(data, P, k, block);
  const int n_models = merge_n_models(data.size(0));
  const int n_segs = merge_n_segs(offsets);
  auto ch = grad_w_chunks(offsets, base, n_segs);
  const int n_chunks = int(ch.numel() / 3);
  auto gw = torch::zeros({n_models, n_segs},
                         base.options().dtype(torch::kFloat32));
  launch_grad_merge_weights_topk(g.data_ptr(), gb, base.data_ptr<float>(), d,
                                 merged.data_ptr<float>(),
                                 ch.data_ptr<int64_t>(), n_models, n_chunks,
                                 P, gw.data_ptr<float>(), n_segs, stream());
  return gw;
}

void axpy_topk(Tensor w, Tensor data, int64_t k, int64_t block, int64_t row,
               double alpha) {
  const int64_t P = w.numel();
  check_plane(w, P, "w");
  const TopkView d = topk_view(data, P, k, block);
  TORCH_CHECK(row >= 0 && row < data.size(0), "row out of range");
  launch_axpy_topk(w.data_ptr<float>(), d, int(row), float(alpha), P,
                   stream());
}

void weighted_merge_packed(Tensor base, Tensor data, Tensor scales,
                           int64_t block, Tensor W, Tensor offsets,
                           Tensor out) {
  const int64_t P = base.numel();
  if (is_topk(data))
    return weighted_merge_topk(base, data, topk_k_of(data, P, block), block,
                               W, offsets, out);
  check_plane(base, P, "base"); check_plane(out, P, "out");
  const PackedView d = packed_view(data, scales, P, block);
  const int n_models = merge_n_models(data.size(0));
  const int n_segs = merge_n_segs(offsets);
  auto Wc = merge_weights(W, base, n_models, n_segs);
  auto offs = merge_offsets(offsets, base);
  launch_weighted_merge_packed(base.data_ptr<float>(), d,
                               Wc.data_ptr<float>(),
                               offs.data_ptr<int64_t>(), n_models, n_segs, P,
                               out.data_ptr<float>(), stream());
}

Tensor grad_merge_weights_packed(Tensor g, Tensor base, Tensor data,
                                 Tensor scales, int64_t block, Tensor merged,
                                 Tensor offsets) {
  const int64_t P = base.numel();
  if (is_topk(data))
    return grad_merge_weights_topk(g, base, data, topk_k_of(data, P, block),
                                   block, merged, offsets);
  check_plane(base, P, "base"); check_plane(merged, P, "merged");
  const bool gb = check_grad_plane(g, P);
  TORCH_CHECK(aligned16(g), "g must be 16-byte aligned");
  const PackedView d = packed_view(data, scales, P, block);
  const int n_models = merge_n_models(data.size(0));
  const int n_segs = merge_n_segs(offsets);
  auto ch = grad_w_chunks(offsets, base, n_segs);
  const int n_chunks = int(ch.numel() / 3);
  auto gw = torch::zeros({n_models, n_segs},
                         base.options().dtype(torch::kFloat32));
  launch_grad_merge_weights_packed(g.data_ptr(), gb, base.data_ptr<float>(),
                                   d, merged.data_ptr<float>(),
                                   ch.data_ptr<int64_t>(), n_models, n_chunks,
                                   P, gw.data_ptr<float>(), n_segs, stream());
  return gw;
}

void axpy_packed(Tensor w, Tensor data, Tensor scales, int64_t block,
                 int64_t row, double alpha) {
  const int64_t P = w.numel();
  if (is_topk(data))
    return axpy_topk(w, data, topk_k_of(data, P, block), block, row, alpha);
  check_plane(w, P, "w");
  const PackedView d = packed_view(data, scales, P, block);
  TORCH_CHECK(row >= 0 && row < data.size(0), "row out of range");
  launch_axpy_packed(w.data_ptr<float>(), d, int(row), float(alpha), P,
                     stream());
}

// ---- robust merge (merge.hip, trimmed_merge_k) -------------------------------
int trimmed_kind(const Tensor& data) {
  switch (data.scalar_type()) {
    case torch::kFloat32: return DELTA_F32;
    case torch::kBFloat16: return DELTA_BF16;
    case torch::kInt8: return DELTA_I8;
    default:
      TORCH_CHECK(false, "trimmed_merge: deltas must be fp32, bf16 or int8 "
                         "(top-k deltas have no coordinate-wise median)");
  }
}
// data [N, P] fp32 (scales empty, block unused), or bf16 / int8 + scales as
// the packed merge takes them. out [P] fp32 is written; outside, where given,
// is an int64 [N] tensor the counts are ADDED to (the caller zero-fills it).
void trimmed_merge(Tensor base, Tensor data, Tensor scales, int64_t block,
                   int64_t trim, Tensor out, OptTensor outside) {
  const int64_t P = base.numel();
  TORCH_CHECK(data.dim() == 2, "trimmed_merge: deltas must be [N, cols]");
  const int n_models = merge_n_models(data.size(0));
  TORCH_CHECK(trim >= 0 && 2 * trim < n_models,
              "trimmed_merge: need 0 <= 2 * trim < n_models, got trim ", trim,
              " for ", n_models, " deltas");
  const int kind = trimmed_kind(data);
  check_plane_f32(base, P, "base"); check_plane_f32(out, P, "out");
  PackedView d;
  if (kind == DELTA_F32) {
    check_deltas_f32(data, P);
    d = PackedView{data.data_ptr(), nullptr, P, 0, 0, DELTA_F32};
  } else {
    d = packed_view(data, scales, P, block);
  }
  if (dta_trimmed_vec(kind, n_models, P) == 4)
    TORCH_CHECK(aligned16(base) && aligned16(out) && aligned16(data),
                "trimmed_merge: base, out and the deltas must be 16-byte "
                "aligned");
  int64_t* cnt = nullptr;
  if (outside.has_value() && outside->defined()) {
    TORCH_CHECK(outside->is_cuda() && outside->is_contiguous() &&
                    outside->scalar_type() == torch::kInt64 &&
                    outside->dim() == 1 && outside->numel() == n_models,
                "outside must be a contiguous int64 [N] GPU tensor");
    cnt = outside->data_ptr<int64_t>();
  }
  launch_trimmed_merge(base.data_ptr<float>(), d, n_models, int(trim), P,
                       out.data_ptr<float>(), cnt, stream());
}
// elements one sweep of the launcher's capped grid covers (tests size a case
// that takes the grid-stride loop round a second time from it)
int64_t trimmed_sweep(Tensor data, int64_t P) {
  TORCH_CHECK(data.dim() == 2, "trimmed_merge: deltas must be [N, cols]");
  return dta_trimmed_sweep(trimmed_kind(data), merge_n_models(data.size(0)),
                           P);
}

// (codes [nb*block] int8, scales [nb] fp32) of x - base, or of x when base
// is empty. topk_k > 0: the top-k form of the same delta instead, {entries
// [nb*topk_k] int32} of (x - base) + residual_in, with the remainder
// written to residual_out (each used when given and not empty)
std::vector<Tensor> quantize_int8(Tensor x, Tensor base, int64_t block,
                                  int64_t topk_k,
                                  std::optional<Tensor> residual_in,
                                  std::optional<Tensor> residual_out) {
  if (topk_k != 0) {
    const Tensor none = x.new_empty({0});
    return {topk_compress(x, base, residual_in.value_or(none),
                          residual_out.value_or(none), topk_k, block)};
  }
  TORCH_CHECK(!residual_in && !residual_out,
              "quantize_int8: a residual belongs to the top-k form");
  check_f32(x, "x");
  const int64_t P = x.numel();
  TORCH_CHECK(P >= 1, "quantize_int8: empty input");
  TORCH_CHECK(aligned16(x), "x must be 16-byte aligned");
  TORCH_CHECK(block >= DTA_QUANT_MIN_BLOCK && block <= DTA_QUANT_MAX_BLOCK &&
                  (block & (block - 1)) == 0,
              "block must be a power of two in [", DTA_QUANT_MIN_BLOCK, ", ",
              DTA_QUANT_MAX_BLOCK, "]");
  const float* bp = nullptr;
  if (base.numel()) {
    check_plane(base, P, "base");
    bp = base.data_ptr<float>();
  }
  const int64_t nb = (P + block - 1) / block;
  TORCH_CHECK(nb < (int64_t(1) << 31), "too many quantisation blocks");
  auto codes = torch::empty({nb * block}, x.options().dtype(torch::kInt8));
  auto scales = torch::empty({nb}, x.options());
  launch_delta_quantize_int8(x.data_ptr<float>(), bp, P, int(block), nb,
                             reinterpret_cast<signed char*>(codes.data_ptr()),
                             scales.data_ptr<float>(), stream());
  return {codes, scales};
}

// ---- CE --------------------------------------------------------------------
std::vector<Tensor> ce_fwd(Tensor logits, Tensor targets,
                           int64_t ignore_index) {
  check_bf16(logits, "logits");
  TORCH_CHECK(targets.scalar_type() == torch::kInt64, "targets int64");
  const int64_t rows = logits.size(0), vocab = logits.size(1);
  auto lse = torch::empty({rows}, logits.options().dtype(torch::kFloat32));
  auto loss = torch::zeros({1}, logits.options().dtype(torch::kFloat32));
  auto count = torch::zeros({1}, logits.options().dtype(torch::kInt32));
  launch_ce_fwd(bfp(logits), targets.data_ptr<int64_t>(), rows, vocab,
                ignore_index, lse.data_ptr<float>(), loss.data_ptr<float>(),
                count.data_ptr<int>(), stream());
  return {loss.squeeze(0), lse, count.squeeze(0)};
}

// pipelined head-GEMM+CE forward helpers: ce_chunk folds one logits tile
// (a [rows, cols] view with leading dim ld, vocab offset v0) into per-row
// running (m, s) and records the target logit; ce_finalize emits
// lse / loss_sum / count from the state alone.
void ce_chunk(Tensor chunk, Tensor targets, int64_t v0, Tensor tlogit,
              Tensor m_run, Tensor s_run) {
  TORCH_CHECK(chunk.is_cuda() && chunk.scalar_type() == torch::kBFloat16 &&
                  chunk.dim() == 2 && chunk.stride(1) == 1,
              "chunk must be a bf16 [rows, cols] view, contiguous cols");
  check_f32(m_run, "m_run"); check_f32(s_run, "s_run");
  check_f32(tlogit, "tlogit");
  launch_ce_chunk(bfp(chunk), chunk.stride(0), chunk.size(0), chunk.size(1),
                  targets.data_ptr<int64_t>(), v0,
                  tlogit.data_ptr<float>(), m_run.data_ptr<float>(),
                  s_run.data_ptr<float>(), stream());
}

std::vector<Tensor> ce_finalize(Tensor targets, Tensor m_run, Tensor s_run,
                                Tensor tlogit, int64_t ignore_index) {
  const int64_t rows = m_run.numel();
  auto lse = torch::empty({rows}, m_run.options());
  auto loss = torch::zeros({1}, m_run.options());
  auto count = torch::zeros({1}, m_run.options().dtype(torch::kInt32));
  launch_ce_finalize(targets.data_ptr<int64_t>(), m_run.data_ptr<float>(),
                     s_run.data_ptr<float>(), tlogit.data_ptr<float>(),
                     rows, ignore_index, lse.data_ptr<float>(),
                     loss.data_ptr<float>(), count.data_ptr<int>(),
                     stream());
  return {loss.squeeze(0), lse, count.squeeze(0)};
}

// ---- fused LM-head loss (forward only) -------------------------------------
// x2 [T,K] @ w[V,K]^T folded into per-row lse / target logit with no [T,V]
// logits in memory. nsplit == 0: automatic vocab split from the CU count;
// an explicit value is clamped to the number of vocab tiles. Returns
// [loss_sum, lse (natural log), count, tlogit] as ce_fwd does.
std::vector<Tensor> head_loss_fwd(Tensor x2, Tensor w, Tensor targets,
                                  int64_t ignore_index, int64_t nsplit) {
  check_bf16(x2, "x");
  check_bf16(w, "w");
  TORCH_CHECK(x2.dim() == 2 && w.dim() == 2, "x must be [T,K], w [V,K]");
  const int64_t T = x2.size(0), K = x2.size(1), V = w.size(0);
  TORCH_CHECK(w.size(1) == K, "x and w disagree on K");
  TORCH_CHECK(K > 0 && K % 64 == 0 && K < (int64_t(1) << 31),
              "head_loss needs K % 64 == 0");
  TORCH_CHECK(V > 0 && V < (int64_t(1) << 31) - DTA_HEAD_LOSS_TILE,
              "head_loss: bad vocab size");
  TORCH_CHECK(T < (int64_t(1) << 31), "head_loss: too many rows");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x2.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "head_loss needs 16-byte aligned x and w");
  TORCH_CHECK(targets.is_cuda() && targets.scalar_type() == torch::kInt64 &&
                  targets.is_contiguous() && targets.dim() == 1 &&
                  targets.numel() == T,
              "targets must be a contiguous int64 [T] GPU tensor");
  TORCH_CHECK(nsplit >= 0, "nsplit must be >= 0");
  const auto f32 = x2.options().dtype(torch::kFloat32);
  auto lse = torch::empty({T}, f32);
  auto loss = torch::zeros({1}, f32);
  auto count = torch::zeros({1}, f32.dtype(torch::kInt32));
  auto tlogit = torch::zeros({T}, f32);
  if (T == 0) return {loss.squeeze(0), lse, count.squeeze(0), tlogit};
  const int64_t ntiles = (V + DTA_HEAD_LOSS_TILE - 1) / DTA_HEAD_LOSS_TILE;
  int ns;
  if (nsplit == 0) {
    ns = dta_head_loss_nsplit(
        T, V, at::cuda::getCurrentDeviceProperties()->multiProcessorCount);
  } else {
    ns = int(std::min<int64_t>(std::min<int64_t>(nsplit, ntiles), 65535));
  }
  auto ws = torch::empty({2, int64_t(ns), T}, f32);   // partial (m, s)
  auto run = torch::empty({2, T}, f32);               // merged m_run, s_run
  float* wsp = ws.data_ptr<float>();
  float* rp = run.data_ptr<float>();
  launch_head_loss(bfp(x2), bfp(w), targets.data_ptr<int64_t>(), T, V, int(K),
                   ns, wsp, wsp + int64_t(ns) * T, tlogit.data_ptr<float>(),
                   rp, rp + T, stream());
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "head_loss launch failed: ",
              hipGetErrorString(err));
  launch_ce_finalize(targets.data_ptr<int64_t>(), rp, rp + T,
                     tlogit.data_ptr<float>(), T, ignore_index,
                     lse.data_ptr<float>(), loss.data_ptr<float>(),
                     count.data_ptr<int>(), stream());
  return {loss.squeeze(0), lse, count.squeeze(0), tlogit};
}

// scale_dev: empty tensor => host 'scale' scalar; else a 0/1-dim fp32
// device scalar (dloss/count), keeping backward free of host syncs.
// v0/nt: vocab-tile offset + store policy for the tiled pipeline.
Tensor ce_bwd(Tensor logits, Tensor targets, Tensor lse, Tensor scale_dev,
              double scale, int64_t ignore_index, int64_t v0, bool nt) {
  check_bf16(logits, "logits");
  const int64_t rows = logits.size(0), vocab = logits.size(1);
  auto dl = torch::empty_like(logits);
  const float* scp = scale_dev.numel() ? scale_dev.data_ptr<float>() : nullptr;
  launch_ce_bwd(bfp(logits), targets.data_ptr<int64_t>(),
                lse.data_ptr<float>(), float(scale), scp, ignore_index, v0,
                nt, bfp_mut(dl), rows, vocab, stream());
  return dl;
}

// Training CE in one kernel: logits [rows, vocab] is OVERWRITTEN with
// dlogits = inv_count * (softmax - onehot), zeros on ignored rows.
// inv_count_dev: fp32 device scalar 1/max(count, 1), computed from targets
// before the call (no host sync). max_rows: rows in flight, 0 = automatic.
// lds_row: the variant that holds the row in LDS (lse then agrees with
// ce_fwd to rounding only); rows too wide for LDS take the default variant.
// Returns [loss_sum, lse, count] as ce_fwd does.
std::vector<Tensor> ce_fwd_bwd(Tensor logits, Tensor targets,
                               int64_t ignore_index, Tensor inv_count_dev,
                               int64_t max_rows, bool lds_row) {
  check_bf16(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(),
              "logits must be a contiguous [rows, vocab] tensor");
  TORCH_CHECK(targets.is_cuda() && targets.scalar_type() == torch::kInt64 &&
                  targets.is_contiguous() &&
                  targets.numel() == logits.size(0),
              "targets must be a contiguous int64 [rows] GPU tensor");
  check_f32(inv_count_dev, "inv_count");
  TORCH_CHECK(inv_count_dev.numel() == 1, "inv_count must be one element");
  TORCH_CHECK(max_rows >= 0, "max_rows must be >= 0");
  const int64_t rows = logits.size(0), vocab = logits.size(1);
  auto lse = torch::empty({rows}, logits.options().dtype(torch::kFloat32));
  auto loss = torch::zeros({1}, logits.options().dtype(torch::kFloat32));
  auto count = torch::zeros({1}, logits.options().dtype(torch::kInt32));
  const auto* prop = at::cuda::getCurrentDeviceProperties();
  if (lds_row &&
      launch_ce_fwd_bwd_lds(bfp_mut(logits), targets.data_ptr<int64_t>(),
                            rows, vocab, ignore_index,
                            inv_count_dev.data_ptr<float>(),
                            lse.data_ptr<float>(), loss.data_ptr<float>(),
                            count.data_ptr<int>(), prop->multiProcessorCount,
                            int64_t(prop->maxSharedMemoryPerMultiProcessor),
                            stream())) {
    const hipError_t err = hipGetLastError();
    TORCH_CHECK(err == hipSuccess, "ce_fwd_bwd (LDS row) launch failed: ",
                hipGetErrorString(err));
    return {loss.squeeze(0), lse, count.squeeze(0)};
  }
  const int blocks =
      max_rows ? int(std::min<int64_t>(max_rows, 65535))
               : dta_ce_fwd_bwd_blocks(vocab, prop->multiProcessorCount);
  launch_ce_fwd_bwd(bfp_mut(logits), targets.data_ptr<int64_t>(), rows, vocab,
                    ignore_index, inv_count_dev.data_ptr<float>(),
                    lse.data_ptr<float>(), loss.data_ptr<float>(),
                    count.data_ptr<int>(), blocks, stream());
  return {loss.squeeze(0), lse, count.squeeze(0)};
}

// ---- embedding -------------------------------------------------------------
// Document layout of packed sequences (the attention q_lo, the embedding's
// doc_start): int32, contiguous, on the GPU, the shape given. The values
// are not read here (that would sync): the kernels clamp them.
const int* doc_table(const c10::optional<Tensor>& t, at::IntArrayRef shape,
                     const char* name) {
  if (!t.has_value() || !t->defined() || t->numel() == 0) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kInt32 &&
                  t->is_contiguous() && t->sizes() == shape,
              name, " must be a contiguous int32 GPU tensor of shape ", shape);
  return t->data_ptr<int>();
}

// pos: optional int32 [1] device offset for the wpe row (graph decode).
// doc_start: optional int32 ids-shaped tensor; the position restarts at
// every document start (wpe row s - doc_start[b, s]).
Tensor embedding_fwd(Tensor ids, Tensor wte, Tensor wpe, Tensor pos,
                     c10::optional<Tensor> doc_start) {
  check_bf16(wte, "wte");
  TORCH_CHECK(ids.scalar_type() == torch::kInt64, "ids int64");
  const bool has_wpe = wpe.numel() > 0;
  const int dim = int(wte.size(1));
  const int seq = int(ids.size(-1));
  const int64_t n_tok = ids.numel();
  auto out_sizes = ids.sizes().vec();
  out_sizes.push_back(dim);
  auto out = torch::empty(out_sizes, wte.options());
  const int* posp = nullptr;
  if (pos.numel()) {
    TORCH_CHECK(pos.scalar_type() == torch::kInt32 && pos.is_cuda(),
                "pos must be an int32 GPU scalar");
    posp = pos.data_ptr<int>();
  }
  const int* dsp = doc_table(doc_start, ids.sizes(), "doc_start");
  if (dsp && has_wpe)
    TORCH_CHECK(ids.is_contiguous() && seq <= wpe.size(0),
                "doc_start needs contiguous ids and seq <= wpe rows");
  launch_embedding_fwd(ids.data_ptr<int64_t>(), bfp(wte),
                       has_wpe ? bfp(wpe) : nullptr, bfp_mut(out), n_tok,
                       seq, dim, has_wpe, posp, dsp, stream());
  return out;
}

// new k/v rows ([B, 1, Hk*D] strided slices of the qkv projection) into
// the caches at device row *pos; pos += 1 via i32_inc afterwards
void kv_append(Tensor kn, Tensor vn, Tensor kc, Tensor vc, Tensor pos) {
  TORCH_CHECK(kn.dim() == 3 && kn.size(1) == 1 && kn.stride(2) == 1,
              "kn must be [B,1,F] with contiguous F");
  TORCH_CHECK(vn.stride(0) == kn.stride(0) && vn.stride(2) == 1,
              "vn must share kn's layout (one qkv projection)");
  TORCH_CHECK(pos.scalar_type() == torch::kInt32 && pos.is_cuda(), "pos");
  TORCH_CHECK(kn.is_cuda() && vn.is_cuda() &&
                  kn.scalar_type() == torch::kBFloat16 &&
                  vn.scalar_type() == torch::kBFloat16,
              "kn, vn must be bf16 GPU tensors");
  // the kernel addresses row *pos of head h at h * stride(1) + pos * D
  TORCH_CHECK(kc.is_cuda() && vc.is_cuda() &&
                  kc.scalar_type() == torch::kBFloat16 &&
                  vc.scalar_type() == torch::kBFloat16,
              "kc, vc must be bf16 GPU caches");
  TORCH_CHECK(kc.dim() == 4 && kc.stride(3) == 1 &&
                  kc.stride(2) == kc.size(3),
              "kc must be [B,Hk,Lmax,D] with contiguous [Lmax,D] planes");
  TORCH_CHECK(vc.sizes() == kc.sizes() && vc.strides() == kc.strides(),
              "vc must have kc's shape and strides");
  TORCH_CHECK(kn.size(0) == kc.size(0) && vn.sizes() == kn.sizes() &&
                  kn.size(2) == kc.size(1) * kc.size(3),
              "kn, vn must be [B,1,Hk*D] of the caches' B, Hk, D");
  const int B = int(kc.size(0)), Hk = int(kc.size(1)), D = int(kc.size(3));
  launch_kv_append(bfp(kn), bfp(vn), kn.stride(0), bfp_mut(kc), bfp_mut(vc),
                   pos.data_ptr<int>(), B, Hk, D, kc.stride(0),
                   kc.stride(1), stream());
}

void i32_inc(Tensor t) {
  TORCH_CHECK(t.scalar_type() == torch::kInt32 && t.is_cuda(), "int32 gpu");
  launch_i32_inc(t.data_ptr<int>(), stream());
}

std::vector<Tensor> embedding_bwd(Tensor dy, Tensor ids, int64_t vocab,
                                  int64_t npos,
                                  c10::optional<Tensor> doc_start) {
  check_bf16(dy, "dy");
  const int dim = int(dy.size(-1));
  const int seq = int(ids.size(-1));
  const int64_t n_tok = ids.numel();
  auto f32 = dy.options().dtype(torch::kFloat32);
  auto dwte = torch::zeros({vocab, dim}, f32);
  auto dwpe = npos ? torch::zeros({npos, dim}, f32) : torch::zeros({0}, f32);
  launch_embedding_bwd(bfp(dy), ids.data_ptr<int64_t>(),
                       dwte.data_ptr<float>(), nullptr, n_tok, seq, dim,
                       false, stream());
  const int* dsp = doc_table(doc_start, ids.sizes(), "doc_start");
  if (npos && dsp) {
    // positions restart per document: dwpe[p,:] sums the tokens at offset p
    // of their document (two-phase like the column sum, no atomics)
    const int64_t B = n_tok / seq;
    TORCH_CHECK(dim % 8 == 0 && seq <= npos && ids.is_contiguous(),
                "doc_start: dim % 8 == 0, seq <= npos, contiguous ids");
    const int stripes = dta_doc_dwpe_stripes(B, seq, dim);
    auto part = torch::empty({stripes, int64_t(seq) * dim}, f32);
    launch_embedding_dwpe_doc(bfp(dy), dsp, part.data_ptr<float>(),
                              dwpe.data_ptr<float>(), B, seq, dim, stripes,
                              stream());
  } else if (npos) {
    // dwpe[s,:] = sum_b dy[b,s,:] — batch-dim column reduction over the
    // [B, seq*dim] view (B-way same-address atomics measured dominant in
    // the scatter version)
    const int64_t B = n_tok / seq;
    const int pcols = seq * dim;
    TORCH_CHECK(pcols % 8 == 0, "seq*dim must be a multiple of 8");
    const int stripes = dta_colred_stripes(B, pcols);
    auto part = torch::empty({stripes, pcols}, f32);
    // stores dwpe[:pcols] (seq <= npos); the rows past seq stay zero
    TORCH_CHECK(seq <= npos, "seq must be <= npos");
    launch_colsum(bfp(dy), part.data_ptr<float>(), dwpe.data_ptr<float>(),
                  nullptr, B, pcols, stripes, stream());
  }
  return {dwte, dwpe};  // fp32: ops layer accumulates or casts
}

// ---- serving gemv ----------------------------------------------------------
Tensor gemv(Tensor x, Tensor w, Tensor bias) {
  check_bf16(x, "x"); check_bf16(w, "w");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == w.size(1),
              "x [M,K], w [N,K]");
  const int M = int(x.size(0));
  TORCH_CHECK(M >= 1 && M <= 4, "gemv is for M <= 4");
  const int64_t N = w.size(0);
  const int K = int(x.size(1));
  TORCH_CHECK(K % 8 == 0, "gemv needs K % 8 == 0 (16 B row alignment)");
  const bf16_t* bp = nullptr;
  if (bias.numel()) {
    check_bf16(bias, "bias");
    bp = bfp(bias);
  }
  auto y = torch::empty({M, N}, x.options());
  launch_gemv(bfp(x), bfp(w), bp, bfp_mut(y), M, N, K, stream());
  return y;
}

// ---- rope ------------------------------------------------------------------
Tensor rope_apply(Tensor x, Tensor cos_t, Tensor sin_t, bool backward,
                  const Tensor& pos) {
  check_bf16(x, "x");
  // x: [B,H,S,D] or [BH,S,D]
  const int hd = int(x.size(-1));
  const int seq = int(x.size(-2));
  const int64_t bh = x.numel() / (int64_t(seq) * hd);
  const int* posp = nullptr;
  if (pos.numel()) {
    TORCH_CHECK(pos.scalar_type() == torch::kInt32 && pos.is_cuda(),
                "pos must be an int32 GPU scalar");
    posp = pos.data_ptr<int>();
  }
  auto y = torch::empty_like(x);
  auto c = cos_t.contiguous();
  auto sn = sin_t.contiguous();
  launch_rope(bfp(x), c.data_ptr<float>(), sn.data_ptr<float>(), bfp_mut(y),
              bh, seq, hd, backward, posp, stream());
  return y;
}
Tensor rope_fwd(Tensor x, Tensor c, Tensor s, Tensor pos) {
  return rope_apply(x, c, s, false, pos);
}
Tensor rope_bwd(Tensor x, Tensor c, Tensor s, Tensor pos) {
  return rope_apply(x, c, s, true, pos);
}

// ---- attention -------------------------------------------------------------
// q/k/v: [B,H(,Hk),S,D] views, innermost stride 1 (checked). Output o (and
// dq) are allocated [B,S,H,D] contiguous — the caller permutes back, so a
// transformer layer does zero transpose copies around attention.
static void check_attn_view(const Tensor& t, const char* n) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16, n,
              " must be bf16 on GPU");
  TORCH_CHECK(t.dim() == 4 && t.stride(3) == 1, n,
              " must be a [B,H,S,D] view with contiguous D");
}

// kvlen: int32 [B] valid-key prefix per batch row (empty = no mask);
// rng: int64 [1] device step counter + site/p: attention-prob dropout
// (p == 0 disables).
// q_lo / k_hi: optional int32 [B,S] document mask (dta_kernels.h AttnGeom).
using OptDoc = c10::optional<Tensor>;
static void set_mask_drop(AttnGeom& g, const Tensor& kvlen, const Tensor& rng,
                          int64_t site, double p, int64_t B,
                          const OptDoc& q_lo = c10::nullopt,
                          const OptDoc& k_hi = c10::nullopt,
                          bool need_k_hi = false) {
  g.q_lo = doc_table(q_lo, {B, int64_t(g.seq)}, "q_lo");
  g.k_hi = doc_table(k_hi, {B, int64_t(g.seq)}, "k_hi");
  TORCH_CHECK(!(need_k_hi && g.q_lo) || g.k_hi,
              "the backward needs k_hi whenever q_lo is given");
  if (!g.q_lo) g.k_hi = nullptr;
  if (kvlen.numel() > 0) {
    TORCH_CHECK(kvlen.scalar_type() == torch::kInt32 && kvlen.is_cuda() &&
                    kvlen.is_contiguous() && kvlen.numel() == B,
                "kvlen must be a contiguous int32 [B] GPU tensor");
    g.kvlen = kvlen.data_ptr<int>();
  }
  g.drop = drop_params(rng, site, p);
}

// (batch, head, seq) strides of a [B,H,S,D] view and of a [B,S,H,D] tensor
static AttnStride strides_bhsd(const Tensor& t) {
  return {t.stride(0), t.stride(1), t.stride(2)};
}
static AttnStride strides_bshd(const Tensor& t) {
  return {t.stride(0), t.stride(2), t.stride(1)};
}

// q/k/v/dout: [B,H(,Hk),S,D] views; o_bshd: [B,S,H,D]. dout may be undefined
// (forward); the backward adds its output strides itself.
static AttnGeom make_geom(const Tensor& q, const Tensor& k, const Tensor& v,
                          const Tensor& o_bshd, const Tensor& dout,
                          double scale) {
  AttnGeom g{};
  g.B = int(q.size(0)); g.H = int(q.size(1));
  g.seq = int(q.size(2)); g.hd = int(q.size(3));
  const int hk = int(k.size(1));
  TORCH_CHECK(g.H % hk == 0, "H must be a multiple of H_kv");
  g.grp = g.H / hk;
  g.scale = float(scale);
  g.q = strides_bhsd(q); g.k = strides_bhsd(k); g.v = strides_bhsd(v);
  g.o = strides_bshd(o_bshd);
  if (dout.defined()) g.dout = strides_bhsd(dout);
  return g;
}

std::vector<Tensor> attn_fwd(Tensor q, Tensor k, Tensor v, double scale,
                             Tensor kvlen, Tensor rng, int64_t site,
                             double p, OptDoc q_lo) {
  check_attn_view(q, "q"); check_attn_view(k, "k"); check_attn_view(v, "v");
  const int hd = int(q.size(3));
  TORCH_CHECK(hd == 32 || hd == 64 || hd == 128, "head dim must be 32/64/128");
  const int64_t B = q.size(0), H = q.size(1), S = q.size(2);
  auto o = torch::empty({B, S, H, hd}, q.options());
  auto lse = torch::empty({B * H, S}, q.options().dtype(torch::kFloat32));
  AttnGeom geo = make_geom(q, k, v, o, Tensor(), scale);
  set_mask_drop(geo, kvlen, rng, site, p, B, q_lo);
  launch_attn_fwd(bfp(q), bfp(k), bfp(v), bfp_mut(o),
                  lse.data_ptr<float>(), geo, stream());
  return {o, lse};  // caller views o as [B,H,S,D] via permute(0,2,1,3)
}

// Single-tile fused backward: on unless DTA_ATTN_BWD_FUSED=0, or
// attn_bwd_fused_enable() said otherwise (tests and the A/B tool run both
// paths in one process). The counter tells a caller which path a call took.
// Atomics: autograd runs the backward on its own threads.
static std::atomic<int> g_attn_bwd_fused_force{-1};   // -1: environment
static std::atomic<int64_t> g_attn_bwd_fused_calls{0};
static bool attn_bwd_fused_on() {
  const int force = g_attn_bwd_fused_force.load();
  return force < 0 ? dta_attn_bwd_fused_default() : force != 0;
}
bool attn_bwd_fused_enable(bool on) {
  const bool was = attn_bwd_fused_on();
  g_attn_bwd_fused_force.store(on ? 1 : 0);
  return was;
}
int64_t attn_bwd_fused_calls() { return g_attn_bwd_fused_calls.load(); }

// The backward both entry points share: one fused launch for a single-tile
// head, else delta alloc -> dQ -> dK/dV.
// dq_v: [B,S,H,D] destination view (contiguous D), always written.
// grp == 1: dk/dv are stored straight into the [B,S,Hk,D] views dk_v/dv_v.
// GQA: the q heads fold into zeroed fp32 [B,Hk,S,D] buffers with atomics;
// dk_v/dv_v are not touched and the buffers are handed back for the caller
// to cast into place.
static std::pair<Tensor, Tensor> attn_bwd_into(
    const Tensor& dout, const Tensor& q, const Tensor& k, const Tensor& v,
    const Tensor& o_bshd, const Tensor& lse, double scale,
    const Tensor& kvlen, const Tensor& rng, int64_t site, double p,
    Tensor dq_v, Tensor dk_v, Tensor dv_v, const OptDoc& q_lo,
    const OptDoc& k_hi) {
  check_attn_view(dout, "dout");
  TORCH_CHECK(dq_v.stride(3) == 1, "dq view needs contiguous head_dim");
  const int64_t B = q.size(0), H = q.size(1), S = q.size(2);
  AttnGeom geo = make_geom(q, k, v, o_bshd, dout, scale);
  geo.dq = strides_bshd(dq_v);
  set_mask_drop(geo, kvlen, rng, site, p, B, q_lo, k_hi, true);
  if (attn_bwd_fused_on() && dta_attn_bwd_fused_shape(geo)) {
    TORCH_CHECK(dk_v.stride(3) == 1 && dk_v.strides() == dv_v.strides(),
                "dk/dv views need contiguous head_dim and equal strides");
    geo.dkv = strides_bshd(dk_v);
    launch_attn_bwd_fused(bfp(dout), bfp(q), bfp(k), bfp(v), bfp(o_bshd),
                          lse.data_ptr<float>(), bfp_mut(dq_v), bfp_mut(dk_v),
                          bfp_mut(dv_v), geo, stream());
    ++g_attn_bwd_fused_calls;
    return {Tensor(), Tensor()};
  }
  auto delta = torch::empty({B * H, S}, lse.options());
  launch_attn_bwd_dq(bfp(dout), bfp(q), bfp(k), bfp(v), bfp(o_bshd),
                     lse.data_ptr<float>(), delta.data_ptr<float>(),
                     bfp_mut(dq_v), geo, stream());
  Tensor dk32, dv32;
  if (geo.grp == 1) {
    TORCH_CHECK(dk_v.stride(3) == 1 && dk_v.strides() == dv_v.strides(),
                "dk/dv views need contiguous head_dim and equal strides");
    geo.dkv = strides_bshd(dk_v);
  } else {
    dk32 = torch::zeros({B, k.size(1), S, q.size(3)},
                        q.options().dtype(torch::kFloat32));
    dv32 = torch::zeros_like(dk32);
  }
  launch_attn_bwd_dkv(bfp(dout), bfp(q), bfp(k), bfp(v),
                      lse.data_ptr<float>(), delta.data_ptr<float>(),
                      geo.grp == 1 ? nullptr : dk32.data_ptr<float>(),
                      geo.grp == 1 ? nullptr : dv32.data_ptr<float>(),
                      geo.grp == 1 ? bfp_mut(dk_v) : nullptr,
                      geo.grp == 1 ? bfp_mut(dv_v) : nullptr, geo, stream());
  return {dk32, dv32};
}

// Returns dq [B,S,H,D] and dk/dv as [B,Hk,S,D]: permuted views of
// [B,S,Hk,D] stores, or with GQA the contiguous cast of the fp32 buffers.
std::vector<Tensor> attn_bwd(Tensor dout, Tensor q, Tensor k, Tensor v,
                             Tensor o_bshd, Tensor lse, double scale,
                             Tensor kvlen, Tensor rng, int64_t site,
                             double p, OptDoc q_lo, OptDoc k_hi) {
  const int64_t B = q.size(0), H = q.size(1), S = q.size(2), hd = q.size(3);
  const int64_t Hk = k.size(1);
  auto dq = torch::empty({B, S, H, hd}, q.options());
  Tensor dk, dv;
  if (H == Hk) {
    dk = torch::empty({B, S, Hk, hd}, q.options());
    dv = torch::empty_like(dk);
  }
  auto [dk32, dv32] = attn_bwd_into(dout, q, k, v, o_bshd, lse, scale, kvlen,
                                    rng, site, p, dq, dk, dv, q_lo, k_hi);
  if (H == Hk) return {dq, dk.permute({0, 2, 1, 3}), dv.permute({0, 2, 1, 3})};
  return {dq, dk32.to(torch::kBFloat16), dv32.to(torch::kBFloat16)};
}

// Packed-QKV backward: dq/dk/dv are stored directly into caller-provided
// [B,S,H,D]/[B,S,Hk,D] strided views of one dqkv buffer (innermost D
// contiguous) — eliminates the split-backward cat and all transpose copies.
void attn_bwd_packed(Tensor dout, Tensor q, Tensor k, Tensor v,
                     Tensor o_bshd, Tensor lse, double scale, Tensor dq_v,
                     Tensor dk_v, Tensor dv_v, Tensor kvlen, Tensor rng,
                     int64_t site, double p, OptDoc q_lo, OptDoc k_hi) {
  TORCH_CHECK(dk_v.stride(3) == 1 && dv_v.stride(3) == 1,
              "dqkv views need contiguous head_dim");
  auto [dk32, dv32] = attn_bwd_into(dout, q, k, v, o_bshd, lse, scale, kvlen,
                                    rng, site, p, dq_v, dk_v, dv_v, q_lo,
                                    k_hi);
  if (!dk32.defined()) return;
  dk_v.copy_(dk32.permute({0, 2, 1, 3}));
  dv_v.copy_(dv32.permute({0, 2, 1, 3}));
}

// Decode attention over a KV cache: q [B,H,D], k/v caches [B,Hk,Lmax,D]
// contiguous, first kv_len positions valid -> o [B,H,D].
Tensor attn_decode(Tensor q, Tensor kc, Tensor vc, int64_t kv_len,
                   double scale, Tensor len_dev) {
  check_bf16(q, "q"); check_bf16(kc, "kcache"); check_bf16(vc, "vcache");
  TORCH_CHECK(q.dim() == 3 && kc.dim() == 4, "q [B,H,D], cache [B,Hk,L,D]");
  const int B = int(q.size(0)), H = int(q.size(1)), hd = int(q.size(2));
  const int Hk = int(kc.size(1));
  TORCH_CHECK(hd == 64 || hd == 128, "decode head dim must be 64/128");
  TORCH_CHECK(H % Hk == 0 && kv_len <= kc.size(2), "bad cache geometry");
  const int* lp = nullptr;
  if (len_dev.numel()) {
    TORCH_CHECK(len_dev.scalar_type() == torch::kInt32 && len_dev.is_cuda(),
                "len_dev must be an int32 GPU scalar");
    lp = len_dev.data_ptr<int>();
  }
  auto o = torch::empty_like(q);
  launch_attn_decode(bfp(q), bfp(kc), bfp(vc), bfp_mut(o), B, H, H / Hk,
                     int(kv_len), lp, hd, kc.stride(0), kc.stride(1),
                     float(scale), stream());
  return o;
}

// ---- mfma self-test --------------------------------------------------------
Tensor mfma_selftest_16(Tensor A, Tensor B) {
  check_bf16(A, "A"); check_bf16(B, "B");
  auto D = torch::zeros({16, 16}, A.options().dtype(torch::kFloat32));
  launch_mfma_probe_16(bfp(A), bfp(B), D.data_ptr<float>(), stream());
  return D;
}
Tensor mfma_selftest_32(Tensor A, Tensor B) {
  check_bf16(A, "A"); check_bf16(B, "B");
  auto D = torch::zeros({32, 32}, A.options().dtype(torch::kFloat32));
  launch_mfma_probe_32(bfp(A), bfp(B), D.data_ptr<float>(), stream());
  return D;
}

}  // namespace

void register_lt_fused(pybind11::module& m);  // lt_fused.cpp

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  register_lt_fused(m);
  m.def("layernorm_fwd", &layernorm_fwd);
  namespace py = pybind11;
  m.def("layernorm_bwd", &layernorm_bwd, py::arg("dy"), py::arg("ds"),
        py::arg("x"), py::arg("w"), py::arg("mean"), py::arg("rstd"),
        py::arg("rng"), py::arg("site"), py::arg("p"),
        py::arg("dw_dst") = py::none(), py::arg("db_dst") = py::none());
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("rmsnorm_bwd", &rmsnorm_bwd, py::arg("dy"), py::arg("ds"),
        py::arg("x"), py::arg("w"), py::arg("rstd"), py::arg("rng"),
        py::arg("site"), py::arg("p"), py::arg("dw_dst") = py::none());
  m.def("gelu_fwd", &gelu_fwd);
  m.def("gelu_bwd", &gelu_bwd);
  m.def("gelu_bwd_colsum", &gelu_bwd_colsum, py::arg("dy"), py::arg("x"),
        py::arg("db_dst") = py::none(), py::arg("stripes") = 0);
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("dropout_apply", &dropout_apply);
  m.def("rng_tick", &rng_tick);
  m.def("accum_f32_into_bf16", &accum_f32_into_bf16);
  m.def("delta_sub", &delta_sub);
  m.def("axpy", &axpy);
  m.def("has_nan", &has_nan);
  m.def("l2norm_sq", &l2norm_sq);
  m.def("adamw_step", &adamw_step);
  m.def("adamw_tick", &adamw_tick);
  m.def("grad_sumsq_blocks", &grad_sumsq_blocks);
  m.def("grad_sumsq_partials", &grad_sumsq_partials);
  m.def("step_control", &step_control);
  m.def("adamw_step_guarded", &adamw_step_guarded);
  m.def("colsum", &colsum, py::arg("x"), py::arg("dst") = py::none());
  // wgrad.hip: its own submodule (m.wgrad.bias, ...). Accuracy tests:
  // tests/test_wgrad_gpu.py, bound self-check tests/test_wgrad_cpu.py.
  py::module_ wg = m.def_submodule("wgrad", "split-K weight gradient");
  wg.def("bias", &wgrad_bias, py::arg("dy"), py::arg("x"), py::arg("dw"),
         py::arg("db") = py::none(), py::arg("bias_f32") = false,
         py::arg("nsplit") = 0);
  wg.def("supported", &wgrad_supported);
  wg.def("tile", &wgrad_tile);
  wg.def("nsplit", &wgrad_nsplit);
  // trimmed_merge_k: its own submodule as well. CPU definition:
  // ops.trimmed_merge; tests/test_robust_merge_gpu.py holds the kernel to it
  // bit for bit.
  py::module_ rb = m.def_submodule("robust", "trimmed-mean / median merge");
  rb.def("trimmed_merge", &trimmed_merge, py::arg("base"), py::arg("data"),
         py::arg("scales"), py::arg("block"), py::arg("trim"), py::arg("out"),
         py::arg("outside") = py::none());
  rb.def("sweep", &trimmed_sweep);
  m.def("weighted_merge", &weighted_merge);
  m.def("grad_merge_weights", &grad_merge_weights);
  m.def("weighted_merge_packed", &weighted_merge_packed);
  m.def("grad_merge_weights_packed", &grad_merge_weights_packed);
  m.def("axpy_packed", &axpy_packed);
  m.def("quantize_int8", &quantize_int8, py::arg("x"), py::arg("base"),
        py::arg("block"), py::arg("topk_k") = 0,
        py::arg("residual_in") = py::none(),
        py::arg("residual_out") = py::none());
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_bwd", &ce_bwd);
  m.def("ce_fwd_bwd", &ce_fwd_bwd, pybind11::arg("logits"),
        pybind11::arg("targets"), pybind11::arg("ignore_index"),
        pybind11::arg("inv_count_dev"), pybind11::arg("max_rows") = 0,
        pybind11::arg("lds_row") = false);
  m.def("ce_chunk", &ce_chunk);
  m.def("ce_finalize", &ce_finalize);
  m.def("head_loss_fwd", &head_loss_fwd);
  m.def("embedding_fwd", &embedding_fwd, py::arg("ids"), py::arg("wte"),
        py::arg("wpe"), py::arg("pos"), py::arg("doc_start") = py::none());
  m.def("embedding_bwd", &embedding_bwd, py::arg("dy"), py::arg("ids"),
        py::arg("vocab"), py::arg("npos"),
        py::arg("doc_start") = py::none());
  m.def("kv_append", &kv_append);
  m.def("i32_inc", &i32_inc);
  m.def("gemv", &gemv);
  m.def("rope_fwd", &rope_fwd);
  m.def("rope_bwd", &rope_bwd);
  m.def("attn_fwd", &attn_fwd, py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("scale"), py::arg("kvlen"), py::arg("rng"), py::arg("site"),
        py::arg("p"), py::arg("q_lo") = py::none());
  m.def("attn_bwd", &attn_bwd, py::arg("dout"), py::arg("q"), py::arg("k"),
        py::arg("v"), py::arg("o_bshd"), py::arg("lse"), py::arg("scale"),
        py::arg("kvlen"), py::arg("rng"), py::arg("site"), py::arg("p"),
        py::arg("q_lo") = py::none(), py::arg("k_hi") = py::none());
  m.def("attn_bwd_packed", &attn_bwd_packed, py::arg("dout"), py::arg("q"),
        py::arg("k"), py::arg("v"), py::arg("o_bshd"), py::arg("lse"),
        py::arg("scale"), py::arg("dq_v"), py::arg("dk_v"), py::arg("dv_v"),
        py::arg("kvlen"), py::arg("rng"), py::arg("site"), py::arg("p"),
        py::arg("q_lo") = py::none(), py::arg("k_hi") = py::none());
  m.def("attn_bwd_fused_enable", &attn_bwd_fused_enable);
  m.def("attn_bwd_fused_calls", &attn_bwd_fused_calls);
  m.def("attn_decode", &attn_decode);
  m.def("mfma_selftest_16", &mfma_selftest_16);
  m.def("mfma_selftest_32", &mfma_selftest_32);
}
