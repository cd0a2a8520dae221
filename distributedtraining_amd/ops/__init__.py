"""Functional op surface for the MI355X-native model stack.

Every op has exactly two execution paths:

* **CPU** — a plain fp32 PyTorch composition. This is the numerics gold the
  GPU kernels are tested against, and what CPU-only plumbing/tests run on.
* **ROCm GPU** — a hand-written gfx950 HIP kernel behind a
  ``torch.autograd.Function`` (see hip/*.hip). There is no eager fallback on
  GPU: missing extension ⇒ loud error (backend.require_ext).

Plain projection GEMMs (QKV/out/MLP/LM-head matmuls) go to hipBLASLt (via
``ops.linear``: addmm with fused bias epilogue forward, dgrad backward), per
the library-GEMM / hand-written-fused-op split; everything fused or
memory-bound is ours. One GEMM class is ours as well: the weight gradients
``dW += dyᵀ·x`` of the shapes ``_wgrad_wins`` lists run on the split-K MFMA
kernel of hip/wgrad.hip, which sums the bias gradient in the same pass over
``dy``; every other weight gradient is a library GEMM accumulated directly
into the flat plane, with the colsum kernel for its bias.

Reference behavior being reimplemented: the implicit per-step op set of
GPT-2 training in /root/reference.
"""

from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

from . import droprng
from .backend import require_ext, use_hip

__all__ = [
    "layer_norm", "rms_norm", "gelu", "swiglu", "causal_attention",
    "qkv_attention", "linear", "mlp_gelu", "add_layer_norm",
    "add_rms_norm",
    "cross_entropy_loss", "lm_head_ce", "lm_head_loss",
    "embedding_fwd", "check_q_lo", "check_doc_start", "q_lo_inverse",
    "decode_attention", "rope", "adamw_step", "delta_sub", "axpy_",
    "weighted_merge", "trimmed_merge", "median_trim",
    "grad_merge_weights", "has_nan", "l2norm",
    "grad_sumsq_blocks", "grad_sumsq_partials", "step_control",
    "adamw_step_guarded", "lr_schedule",
    "quantize_blockwise_int8", "dequantize_blockwise_int8",
    "topk_compress_blockwise",
    "dropout", "rng_tick",
]


# --------------------------------------------------------------------------
# Linear (library GEMM via hipBLASLt) with fast dbias backward
# --------------------------------------------------------------------------
import os as _os

_USE_BGRADB = _os.environ.get("DTA_LT_BGRADB", "0") == "1"

# Weight-gradient routing: "0" library GEMM + colsum everywhere (the path
# before wgrad.hip), "1" the wgrad kernel wherever its shape contract holds,
# anything else: the kernel only where _wgrad_wins measured it faster.
_WGRAD = _os.environ.get("DTA_WGRAD", "auto")
if _WGRAD not in ("0", "1"):
    _WGRAD = "auto"


def wgrad_route(mode: str) -> str:
    """Switch the weight-gradient routing ("0", "1" or "auto"; tests flip it
    in one process). Returns the previous setting."""
    global _WGRAD
    if mode not in ("0", "1", "auto"):
        raise ValueError(f"wgrad_route: {mode!r}")
    prev, _WGRAD = _WGRAD, mode
    return prev


# (T, out, in) at which tools/wgrad_ab.py measured the wgrad kernel faster than
# addmm_ + colsum by more than the library arm's own spread (MI355X,
# profiles/r10_wgrad.md). Unmeasured shapes stay on the library.
_WGRAD_WINS: frozenset = frozenset(
    (T, out, inp) for T in (65536, 32768)
    for out, inp in ((2304, 768), (768, 768), (3072, 768), (768, 3072)))


def _wgrad_wins(T: int, out: int, inp: int) -> bool:
    return (T, out, inp) in _WGRAD_WINS


def _wgrad_accum(m, dy2, x2, wgrad, bgrad, want_bias):
    """dW (+ db) of one linear into the flat plane. -> (handled, db32):
    handled False leaves everything to the library path; db32 is the fp32
    bias gradient where a bias was wanted and bgrad is None."""
    if _WGRAD == "0" or wgrad is None or dy2.dtype != torch.bfloat16:
        return False, None
    if _WGRAD == "auto" and not _wgrad_wins(
            dy2.shape[0], dy2.shape[1], x2.shape[1]):
        return False, None
    if not (wgrad.is_contiguous() and m.wgrad.supported(dy2, x2)):
        return False, None
    db32 = m.wgrad.bias(dy2, x2, wgrad, bgrad if want_bias else None,
                        want_bias and bgrad is None)
    return True, (db32 if want_bias and bgrad is None else None)


class _LinearFn(torch.autograd.Function):
    """F.linear semantics with two backward optimizations:

    * bias gradient via our vectorized colsum kernel instead of torch's
      generic reduce_kernel (~4x faster at the GPT-2 shapes),
    * weight gradient accumulated DIRECTLY into the flat-grad plane
      (w.main_grad, parallel/flat.py) with one addmm(beta=1) — skipping
      the fresh-tensor-then-autograd-add pair per weight per step."""

    @staticmethod
    def forward(ctx, x, w, b):
        x2 = x.reshape(-1, x.shape[-1])
        ctx.save_for_backward(x2, w)
        ctx.has_b = b is not None
        ctx.xshape = x.shape
        ctx.wgrad = getattr(w, "main_grad", None)
        ctx.bgrad = getattr(b, "main_grad", None) if b is not None else None
        y = torch.addmm(b, x2, w.t()) if b is not None else x2.mm(w.t())
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        if dy2.stride(-1) != 1:
            dy2 = dy2.contiguous()
        dx = dy2.mm(w).view(ctx.xshape)
        m = require_ext()
        if _USE_BGRADB and ctx.has_b and ctx.wgrad is not None:
            # one GEMM: dW accumulated into the flat plane (beta=1) with
            # the bias gradient via the BGRADB epilogue. Works at every
            # production shape BUT loses to TunableOp stream-K wgrad +
            # colsum — FINAL negative result r02: even with the FULL
            # algorithm catalog (hipblaslt_ext::getAllAlgos, 128 MiB
            # workspace) timed per shape, the best BGRADB plan measured
            # 815k vs 882k tokens/s whole-step (80.4 vs 74.3 ms). The
            # epilogue's bias reduction forces non-stream-K kernels at
            # K=65536. Kept opt-in for other shapes/batches.
            try:
                db = m.lt_wgrad_bgradb(dy2, x2, ctx.wgrad)
                return dx, None, db
            except RuntimeError:   # no epilogue kernel for this shape
                pass
        done, db32 = _wgrad_accum(m, dy2, x2, ctx.wgrad, ctx.bgrad, ctx.has_b)
        if done:                            # dW and db from one pass over dy
            return dx, None, _cast_grad(db32, w.dtype)
        if ctx.wgrad is not None:
            ctx.wgrad.addmm_(dy2.t(), x2)   # flat-plane accumulation
            dw = None
        else:
            dw = dy2.t().mm(x2)
        db = (_cast_grad(m.colsum(dy2, ctx.bgrad), w.dtype)
              if ctx.has_b else None)
        return dx, dw, db


def linear(x: torch.Tensor, w: torch.Tensor,
           b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x @ w.T (+ b). hipBLASLt GEMM with fused bias epilogue forward;
    backward: dgrad by the library; dW and the bias gradient accumulated into
    the flat-grad plane by the wgrad kernel (hip/wgrad.hip) at the shapes of
    _wgrad_wins, else by a library GEMM (beta = 1) + colsum (DTA_LT_BGRADB=1:
    one BGRADB-epilogue GEMM).

    Serving decode (inference, tiny M): LATENCY-bound projections route
    to the hand-written GEMV; the big weight-streaming shapes stay on
    tuned hipBLASLt. Per-shape A/B at M=1 (tools/gemv_ab.py, MI355X):
    gemv wins up to ~17M-element weights (q/o 4096x4096: 12.1 vs
    22.6 us), tuned hipBLASLt wins the streaming shapes (down-proj
    22.0 vs 53.3 us at 5.3 TB/s; untuned heuristics were the original
    1.7 TB/s problem — tuning/ carries the decode-shape selections)."""
    if use_hip(x):
        rows = x.numel() // x.shape[-1]
        if rows <= 4 and not torch.is_grad_enabled() and _gemv_wins(rows, w):
            x2 = x.reshape(rows, x.shape[-1])
            if not x2.is_contiguous():
                x2 = x2.contiguous()
            y = require_ext().gemv(
                x2, w, b if b is not None
                else torch.empty(0, dtype=w.dtype, device=w.device))
            return y.view(*x.shape[:-1], w.shape[0])
        return _LinearFn.apply(x, w, b)
    return F.linear(x, w, b)


def _gemv_wins(rows: int, w: torch.Tensor) -> bool:
    """Measured crossover (tools/gemv_ab.py): the hand-written GEMV beats
    tuned hipBLASLt while the weight matrix is latency- not
    bandwidth-bound."""
    if w.shape[1] % 8 != 0:      # 16 B row-alignment contract of gemv.hip
        return False
    numel = w.shape[0] * w.shape[1]
    return numel < (20_000_000 if rows == 1 else 5_000_000)


# --------------------------------------------------------------------------
# Fused MLP: linear+GELU+linear through hipBLASLt epilogues
# --------------------------------------------------------------------------
# hipBLASLt epilogue availability is SHAPE-dependent (the heuristics reject
# e.g. GELU_AUX_BIAS at M=512 N=3072 K=768) — cache the verdict per
# (M, N, K) so a serving decode shape rejected after a successful prefill
# shape falls back instead of crashing.
_lt_fused_shape_ok: dict = {}


class _FusedMLPFn(torch.autograd.Function):
    """GPT-2 MLP as one node: h = gelu(x W1ᵀ + b1); y = h W2ᵀ + b2.

    Forward fc1 uses HIPBLASLT_EPILOGUE_GELU_AUX_BIAS (gelu fused into the
    GEMM, pre-gelu aux saved); backward fuses dgelu + db1 into fc2's dgrad
    GEMM (DGELU_BGRAD) — eliminating the standalone GELU fwd/bwd kernels
    and the fc1 dbias reduction (≈5 ms/step at batch 1024). Weight grads
    accumulate into the flat plane (main_grad) like ops.linear."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        m = require_ext()
        x2 = x.reshape(-1, x.shape[-1])
        h, aux = m.lt_linear_gelu_fwd(x2.contiguous(), w1, b1)
        y = torch.addmm(b2, h, w2.t())
        ctx.save_for_backward(x2, w1, w2, h, aux)
        ctx.xshape = x.shape
        ctx.w1grad = getattr(w1, "main_grad", None)
        ctx.w2grad = getattr(w2, "main_grad", None)
        ctx.b2grad = getattr(b2, "main_grad", None)
        return y.view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        m = require_ext()
        x2, w1, w2, h, aux = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        if dy2.stride(-1) != 1:
            dy2 = dy2.contiguous()
        db2 = _cast_grad(m.colsum(dy2, ctx.b2grad), w2.dtype)
        if ctx.w2grad is not None:
            ctx.w2grad.addmm_(dy2.t(), h)
            dw2 = None
        else:
            dw2 = dy2.t().mm(h)
        dh_pre, db1 = m.lt_dgrad_dgelu_bgrad(dy2, w2, aux)
        if ctx.w1grad is not None:
            ctx.w1grad.addmm_(dh_pre.t(), x2)
            dw1 = None
        else:
            dw1 = dh_pre.t().mm(x2)
        dx = dh_pre.mm(w1).view(ctx.xshape)
        return dx, dw1, db1, dw2, db2


# DTA_MLP_NODE=0 keeps the composed path on linear -> gelu -> linear, three
# autograd nodes with a separate colsum over dh_pre for the fc bias.
_MLP_NODE = _os.environ.get("DTA_MLP_NODE", "1") != "0"


def mlp_node_enable(on: bool) -> bool:
    """Switch the one-node composed MLP (tests flip it in one process).
    Returns the previous setting."""
    global _MLP_NODE
    prev, _MLP_NODE = _MLP_NODE, bool(on)
    return prev


class _MLPGeluFn(torch.autograd.Function):
    """The composed GPT-2 MLP as one node: the GEMMs, their operands and the
    saved tensors of linear -> gelu -> linear, with the fc bias gradient
    summed by the kernel that writes dh_pre (gelu_bwd_colsum) instead of a
    second pass over it. bf16 only."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        m = require_ext()
        x2 = x.reshape(-1, x.shape[-1])
        pre = torch.addmm(b1, x2, w1.t())
        h = m.gelu_fwd(pre)
        y = torch.addmm(b2, h, w2.t())
        ctx.save_for_backward(x2, w1, w2, pre, h)
        ctx.xshape = x.shape
        ctx.grads = tuple(getattr(t, "main_grad", None)
                          for t in (w1, b1, w2, b2))
        return y.view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        m = require_ext()
        x2, w1, w2, pre, h = ctx.saved_tensors
        w1g, b1g, w2g, b2g = ctx.grads
        dy2 = dy.reshape(-1, dy.shape[-1])
        if dy2.stride(-1) != 1:
            dy2 = dy2.contiguous()
        dh = dy2.mm(w2)
        done, db32 = _wgrad_accum(m, dy2, h, w2g, b2g, True)
        if done:
            dw2, db2 = None, _cast_grad(db32, w2.dtype)
        else:
            if w2g is not None:
                w2g.addmm_(dy2.t(), h)
                dw2 = None
            else:
                dw2 = dy2.t().mm(h)
            db2 = _cast_grad(m.colsum(dy2, b2g), w2.dtype)
        dh_pre, db1 = m.gelu_bwd_colsum(dh, pre, b1g)
        del dh
        dx = dh_pre.mm(w1).view(ctx.xshape)
        # the fc bias already comes from gelu_bwd_colsum: no-bias kernel
        done, _ = _wgrad_accum(m, dh_pre, x2, w1g, None, False)
        if done:
            dw1 = None
        elif w1g is not None:
            w1g.addmm_(dh_pre.t(), x2)
            dw1 = None
        else:
            dw1 = dh_pre.t().mm(x2)
        return dx, dw1, _cast_grad(db1, w1.dtype), dw2, db2


def mlp_gelu(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor,
             w2: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """y = gelu(x W1ᵀ + b1) W2ᵀ + b2 (GPT-2 MLP). On GPU, epilogue-fused
    via hipBLASLt when available for this (M, N, K); shapes the epilogue
    heuristics reject fall back to the composed path (cached, logged
    once per shape): one autograd node for bf16 (_MLPGeluFn), else
    linear -> gelu -> linear."""
    if use_hip(x):
        rows = x.numel() // x.shape[-1]
        if rows <= 4 and not torch.is_grad_enabled():
            # serving decode: composed path over the streaming GEMV
            return linear(gelu(linear(x, w1, b1)), w2, b2)
        key = (rows, w1.shape[0], w1.shape[1])
        if _lt_fused_shape_ok.get(key, True):
            try:
                out = _FusedMLPFn.apply(x, w1, b1, w2, b2)
                _lt_fused_shape_ok[key] = True
                return out
            except RuntimeError as e:
                import logging
                logging.getLogger(__name__).warning(
                    "hipBLASLt epilogue MLP unavailable at M,N,K=%s (%s); "
                    "composed path", key, e)
                _lt_fused_shape_ok[key] = False
        if _MLP_NODE and all(t.dtype == torch.bfloat16
                             for t in (x, w1, b1, w2, b2)):
            return _MLPGeluFn.apply(x, w1, b1, w2, b2)
        return linear(gelu(linear(x, w1, b1)), w2, b2)
    return F.linear(F.gelu(F.linear(x, w1, b1), approximate="tanh"), w2, b2)


# --------------------------------------------------------------------------
# LayerNorm / RMSNorm
# --------------------------------------------------------------------------
def _empty_like0(t):
    return t.new_empty(0)


def _rng0(t: torch.Tensor) -> torch.Tensor:
    return droprng.counter(t.device)


def _grad_out(fp32_grad, main_grad, dtype):
    """Deliver a parameter gradient: accumulate the fp32 reduction into
    the flat bf16 grad plane when the param carries one (single fused
    kernel), else hand autograd a cast tensor (plain-module models).
    Only for producers without a finisher of their own (the embeddings):
    the column reductions take main_grad as their destination."""
    if main_grad is not None:
        require_ext().accum_f32_into_bf16(main_grad, fp32_grad)
        return None
    return fp32_grad.to(dtype)


def _cast_grad(fp32_grad, dtype):
    """What a column reduction hands autograd: None where it accumulated
    into main_grad itself, else the fp32 result cast to the param dtype."""
    return None if fp32_grad is None else fp32_grad.to(dtype)


def _cpu_drop(t: torch.Tensor, p: float, site: int) -> torch.Tensor:
    """Host gold of the counter-RNG dropout: t ⊙ mask / keep."""
    keep = droprng.elem_keep_mask(t.numel(), droprng.value(t.device), site, p)
    mask = torch.from_numpy(keep.astype("float32")).reshape(t.shape)
    return t * (mask * droprng.inv_keep(p)).to(t.dtype)


# The two norm Functions serve LayerNorm and RMSNorm: b is None => RMS.
def _norm_fwd(x2, res, w, b, eps, site, p):
    """-> (y, stats, sum); stats = (mean, rstd), or (rstd,) for RMS."""
    m = require_ext()
    if b is None:
        y, rstd, s = m.rmsnorm_fwd(x2, res, w, eps, _rng0(x2), site, p)
        return y, (rstd,), s
    y, mean, rstd, s = m.layernorm_fwd(x2, res, w, b, eps, _rng0(x2), site, p)
    return y, (mean, rstd), s


def _norm_bwd(dy, ds, x2, w, stats, site, p, wg=None, bg=None):
    """-> (dx, dw32, db32 or None, dres). wg/bg: main_grad views dγ/dβ are
    accumulated into by the kernel itself; that fp32 result is then None."""
    m = require_ext()
    if len(stats) == 1:
        dx, dw32, dres = m.rmsnorm_bwd(dy, ds, x2, w, *stats, _rng0(x2),
                                       site, p, wg)
        return dx, dw32, None, dres
    return m.layernorm_bwd(dy, ds, x2, w, *stats, _rng0(x2), site, p, wg, bg)


class _NormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        x2 = x.contiguous()
        y, stats, _ = _norm_fwd(x2.view(-1, x2.shape[-1]), _empty_like0(x2),
                                w, b, eps, 0, 0.0)
        ctx.save_for_backward(x2, w, *stats)
        ctx.wg = getattr(w, "main_grad", None)
        ctx.bg = getattr(b, "main_grad", None)
        return y.view_as(x2)

    @staticmethod
    def backward(ctx, dy):
        x, w, *stats = ctx.saved_tensors
        N = x.shape[-1]
        dx, dw32, db32, _ = _norm_bwd(dy.contiguous().view(-1, N),
                                      _empty_like0(x), x.view(-1, N), w,
                                      stats, 0, 0.0, ctx.wg, ctx.bg)
        return (dx.view_as(x), _cast_grad(dw32, w.dtype),
                _cast_grad(db32, w.dtype), None)


def layer_norm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor,
               eps: float = 1e-5) -> torch.Tensor:
    if use_hip(x):
        return _NormFn.apply(x, w, b, eps)
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


class _AddNormFn(torch.autograd.Function):
    """Fused residual-add + norm: (s, y) = (x+res, norm(x+res)).

    The sum is rounded to bf16 before the statistics so backward (which
    recomputes the normalized values from the saved bf16 sum) matches
    exactly; backward folds the sum-stream gradient ds into dx inside the
    dx kernel. Together this removes the separate residual add kernels
    forward AND backward (the residual joins were ~48 eager add
    launches/step). With p_drop > 0 the INCOMING branch is dropout-ed
    inside the same kernels (counter RNG): s = x + drop(res), and
    backward regenerates the mask to emit dres — the standalone dropout
    fwd+bwd HBM passes disappear entirely."""

    @staticmethod
    def forward(ctx, x, res, w, b, eps, p_drop, site):
        x2 = x.contiguous().view(-1, x.shape[-1])
        r2 = res.contiguous().view(-1, x.shape[-1])
        y, stats, s = _norm_fwd(x2, r2, w, b, eps, site, p_drop)
        ctx.save_for_backward(s, w, *stats)
        ctx.shape = x.shape
        ctx.drop = (p_drop, site)
        ctx.wg = getattr(w, "main_grad", None)
        ctx.bg = getattr(b, "main_grad", None)
        return s.view(x.shape), y.view(x.shape)

    @staticmethod
    def backward(ctx, ds, dy):
        s, w, *stats = ctx.saved_tensors
        p_drop, site = ctx.drop
        N = s.shape[-1]
        ds2 = (ds.contiguous().view(-1, N) if ds is not None
               else _empty_like0(s))
        dx, dw32, db32, dres = _norm_bwd(dy.contiguous().view(-1, N), ds2, s,
                                         w, stats, site, p_drop, ctx.wg,
                                         ctx.bg)
        dx = dx.view(ctx.shape)
        dr = dres.view(ctx.shape) if p_drop > 0.0 else dx
        return (dx, dr, _cast_grad(dw32, w.dtype), _cast_grad(db32, w.dtype),
                None, None, None)


def add_layer_norm(x: torch.Tensor, res: torch.Tensor, w: torch.Tensor,
                   b: torch.Tensor, eps: float = 1e-5, p_drop: float = 0.0,
                   site: int = 0):
    """(s, y) = (x + dropout(res), layer_norm(...)) — the transformer
    residual join fused into the norm; with p_drop > 0 the incoming
    branch additionally gets counter-RNG dropout inside the same kernel
    (transformers resid_pdrop applied at the join that consumes the
    branch)."""
    if use_hip(x):
        return _AddNormFn.apply(x, res, w, b, eps, p_drop, site)
    if p_drop > 0.0:
        res = _cpu_drop(res, p_drop, site)
    s = x + res
    return s, F.layer_norm(s, (s.shape[-1],), w, b, eps)


# --------------------------------------------------------------------------
# RMSNorm (Llama family)
# --------------------------------------------------------------------------
def add_rms_norm(x: torch.Tensor, res: torch.Tensor, w: torch.Tensor,
                 eps: float = 1e-5, p_drop: float = 0.0, site: int = 0):
    """(s, y) = (x + dropout(res), rms_norm(...))."""
    if use_hip(x):
        return _AddNormFn.apply(x, res, w, None, eps, p_drop, site)
    if p_drop > 0.0:
        res = _cpu_drop(res, p_drop, site)
    s = x + res
    sf = s.float()
    y = sf * torch.rsqrt(sf.pow(2).mean(-1, keepdim=True) + eps)
    return s, (y * w.float()).to(s.dtype)


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    if use_hip(x):
        return _NormFn.apply(x, w, None, eps)
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (y * w.float()).to(x.dtype)


# --------------------------------------------------------------------------
# Counter-based dropout (transformers GPT-2 trains with pdrop 0.1 —
# resid/embd/attn; the reference inherits those defaults via
# from_pretrained, neurons/miner.py:60-62). Masks regenerate from
# (device counter, site, index) — storage-free, hipGraph-capturable
# (ops/droprng.py documents the chain). The caller advances the stream
# once per step via rng_tick().
# --------------------------------------------------------------------------
class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, site, p):
        m = require_ext()
        c = droprng.counter(x.device)
        ctx.drop_args = (c, site, p)
        return m.dropout_apply(x.contiguous(), c, site, p)

    @staticmethod
    def backward(ctx, dy):
        # same masked scale; valid while the counter hasn't ticked again
        # (backward runs within the producing step in every training loop)
        m = require_ext()
        c, site, p = ctx.drop_args
        return m.dropout_apply(dy.contiguous(), c, site, p), None, None


def dropout(x: torch.Tensor, p: float, site: int,
            training: bool = True) -> torch.Tensor:
    """y = x ⊙ mask / (1-p) with a counter-derived mask; identity when
    p == 0 or not training. ``site`` decorrelates call sites within one
    step (fwd and bwd of one call share it)."""
    if p <= 0.0 or not training:
        return x
    if use_hip(x):
        return _DropoutFn.apply(x, site, p)
    return _cpu_drop(x, p, site)


def rng_tick(device) -> None:
    """Advance the dropout RNG one step (capturable on GPU)."""
    droprng.tick(device)


# --------------------------------------------------------------------------
# GELU (tanh approximation — GPT-2 uses gelu_new)
# --------------------------------------------------------------------------
class _GeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        m = require_ext()
        x2 = x.contiguous()
        ctx.save_for_backward(x2)
        return m.gelu_fwd(x2)

    @staticmethod
    def backward(ctx, dy):
        m = require_ext()
        (x,) = ctx.saved_tensors
        return m.gelu_bwd(dy.contiguous(), x)


def gelu(x: torch.Tensor) -> torch.Tensor:
    if use_hip(x):
        return _GeluFn.apply(x)
    return F.gelu(x, approximate="tanh")


# --------------------------------------------------------------------------
# SwiGLU (Llama MLP): silu(gate) * up
# --------------------------------------------------------------------------
class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, up):
        m = require_ext()
        gate, up = gate.contiguous(), up.contiguous()
        ctx.save_for_backward(gate, up)
        return m.swiglu_fwd(gate, up)

    @staticmethod
    def backward(ctx, dy):
        m = require_ext()
        gate, up = ctx.saved_tensors
        dgate, dup = m.swiglu_bwd(dy.contiguous(), gate, up)
        return dgate, dup


def swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    if use_hip(gate):
        return _SwiGLUFn.apply(gate, up)
    return F.silu(gate) * up


# --------------------------------------------------------------------------
# Fused causal attention (flash-style): q,k,v [B,H,S,D] -> o [B,H,S,D]
# --------------------------------------------------------------------------
def _dense_last(t: torch.Tensor) -> torch.Tensor:
    # kernel requirement: innermost head_dim contiguous; any batch/head/seq
    # strides are fine (no transpose copies)
    return t if t.stride(-1) == 1 else t.contiguous()


def check_q_lo(q_lo: torch.Tensor) -> torch.Tensor:
    """Validate a document-mask lower bound on the host: int32 [B, S] with
    0 <= q_lo[b, q] <= q, non-decreasing along q. Raises ValueError. Reads
    the values (a sync on a GPU tensor): for the CPU path, the packer and
    tests — the GPU kernels clamp instead of checking."""
    if not isinstance(q_lo, torch.Tensor) or q_lo.dtype != torch.int32:
        raise ValueError("q_lo must be an int32 tensor")
    if q_lo.dim() != 2:
        raise ValueError(f"q_lo must be [B, S], got {tuple(q_lo.shape)}")
    S = q_lo.shape[1]
    idx = torch.arange(S, dtype=torch.int32, device=q_lo.device)
    if bool((q_lo < 0).any()):
        raise ValueError("q_lo has negative entries")
    if bool((q_lo > idx).any()):
        raise ValueError("q_lo[b, q] must be <= q")
    if S > 1 and bool((q_lo[:, 1:] < q_lo[:, :-1]).any()):
        raise ValueError("q_lo must be non-decreasing along the sequence")
    return q_lo


def check_doc_start(doc_start: torch.Tensor) -> torch.Tensor:
    """:func:`check_q_lo`, and that the tensor is a document layout: every
    value names a column that starts a document (doc_start there equals the
    column). What the embedding needs; raises ValueError."""
    check_q_lo(doc_start)
    at_start = torch.gather(doc_start, 1, doc_start.long())
    if bool((at_start != doc_start).any()):
        raise ValueError("doc_start is not a document layout: "
                         "doc_start[b, doc_start[b, s]] must equal "
                         "doc_start[b, s]")
    return doc_start


def q_lo_inverse(q_lo: torch.Tensor) -> torch.Tensor:
    """k_hi[b, k] = #{q : q_lo[b, q] <= k}: one past the last query that
    sees key k, the attention backward's loop bound. q_lo is non-decreasing,
    so this is one searchsorted over the rows: on the device, no host sync,
    capturable. Derive it once per batch and hand it to every layer."""
    B, S = q_lo.shape
    keys = torch.arange(S, dtype=torch.int32, device=q_lo.device)
    return torch.searchsorted(q_lo.contiguous(), keys.expand(B, S).contiguous(),
                              right=True, out_int32=True)


def _doc_bounds(q_lo, k_hi, like: torch.Tensor):
    """(q_lo, k_hi) as the bindings take them: int32 contiguous on
    ``like``'s device, k_hi derived when the caller did not."""
    if q_lo is None:
        return None, None
    B, S = like.shape[0], like.shape[-2] if like.dim() == 4 else like.shape[1]
    if q_lo.dtype != torch.int32 or tuple(q_lo.shape) != (B, S):
        raise ValueError(f"q_lo must be int32 [{B}, {S}], got {q_lo.dtype} "
                         f"{tuple(q_lo.shape)}")
    q_lo = q_lo.contiguous()
    if k_hi is None:
        k_hi = q_lo_inverse(q_lo)
    return q_lo, k_hi


def _mask_and_counter(kvlen, like: torch.Tensor):
    """The kvlen tensor the bindings expect (empty = no mask) and the
    dropout step counter of ``like``'s device."""
    if kvlen is None:
        kvlen = torch.empty(0, dtype=torch.int32, device=like.device)
    return kvlen, droprng.counter(like.device)


class _AttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, kvlen, p_drop, site, q_lo=None,
                k_hi=None):
        m = require_ext()
        q, k, v = _dense_last(q), _dense_last(k), _dense_last(v)
        kv, rng = _mask_and_counter(kvlen, q)
        o_bshd, lse = m.attn_fwd(q, k, v, scale, kv, rng, site, p_drop,
                                 q_lo)
        ctx.save_for_backward(q, k, v, o_bshd, lse, kv, rng, q_lo, k_hi)
        ctx.attn_args = (scale, site, p_drop)
        return o_bshd.permute(0, 2, 1, 3)  # [B,H,S,D] view, zero-copy

    @staticmethod
    def backward(ctx, do):
        m = require_ext()
        q, k, v, o_bshd, lse, kv, rng, q_lo, k_hi = ctx.saved_tensors
        scale, site, p_drop = ctx.attn_args
        dq_bshd, dk, dv = m.attn_bwd(_dense_last(do), q, k, v, o_bshd, lse,
                                     scale, kv, rng, site, p_drop, q_lo, k_hi)
        return (dq_bshd.permute(0, 2, 1, 3), dk, dv, None, None, None,
                None, None, None)


def _attn_ref(q, k, v, scale, kvlen, p_drop, site, q_lo=None):
    """CPU gold: explicit masked softmax attention with the SAME padding
    and dropout semantics the HIP kernels implement (mask from the shared
    RNG chain, so GPU tests compare bit-identical masks). fp32 math;
    differentiable through plain torch ops."""
    B, H, S, D = q.shape
    Hk = k.shape[1]
    kf, vf = k.float(), v.float()
    if Hk != H:
        rep = H // Hk
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    scores = torch.einsum("bhqd,bhkd->bhqk", q.float(), kf) * scale
    idx = torch.arange(S)
    allowed = (idx[None, :] <= idx[:, None])[None, None]   # causal [1,1,q,k]
    if kvlen is not None:
        allowed = allowed & (idx[None, None, None, :]
                             < kvlen.view(B, 1, 1, 1).to(torch.long))
    if q_lo is not None:   # document mask: keys from q's document start on
        allowed = allowed & (idx[None, None, None, :]
                             >= q_lo.view(B, 1, S, 1).to(torch.long))
    A = torch.softmax(scores.masked_fill(~allowed, float("-inf")), dim=-1)
    if p_drop > 0.0:
        keep = droprng.attn_keep_mask(B * H, S, S,
                                      droprng.value(q.device), site, p_drop)
        A = A * (torch.from_numpy(keep.astype("float32")).view(B, H, S, S)
                 * droprng.inv_keep(p_drop))
    return torch.einsum("bhqk,bhkd->bhqd", A, vf).to(q.dtype)


def causal_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                     scale: Optional[float] = None,
                     kvlen: Optional[torch.Tensor] = None,
                     p_drop: float = 0.0, site: int = 0,
                     q_lo: Optional[torch.Tensor] = None,
                     k_hi: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(q kᵀ · scale + causal_mask) v over [B, H, S, D] tensors.

    GQA: k/v may have fewer heads (H_kv dividing H) — handled natively by
    the kernel (no repeat_interleave). Inputs may be permuted views of
    [B,S,H*D] projections; only the head_dim must be contiguous.

    ``kvlen`` (int32 [B]): right-padding mask — key j of row b is attended
    iff j < kvlen[b] (the reference's attention_mask semantics,
    training_manager.py:380-385). ``p_drop``/``site``: attention-prob
    dropout from the counter RNG (transformers attn_pdrop).

    ``q_lo`` (int32 [B, S]): document mask of packed sequences — key k is
    visible to query q iff q_lo[b, q] <= k as well; q_lo[b, s] is the first
    token of the document that holds s (contract: :func:`check_q_lo`; the
    GPU path does not validate, the kernels clamp). ``k_hi``: its inverse
    (:func:`q_lo_inverse`), derived here unless the caller did it once for
    all layers.
    """
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if use_hip(q):
        q_lo, k_hi = _doc_bounds(q_lo, k_hi, q)
        return _AttnFn.apply(q, k, v, scale, kvlen, p_drop, site, q_lo, k_hi)
    if kvlen is None and p_drop <= 0.0 and q_lo is None:
        return F.scaled_dot_product_attention(q, k, v, is_causal=True,
                                              scale=scale, enable_gqa=True)
    if q_lo is not None:
        check_q_lo(q_lo)
    return _attn_ref(q, k, v, scale, kvlen, p_drop, site, q_lo)


# --------------------------------------------------------------------------
# Packed-QKV causal attention: one [B,S,(H+2Hk)·D] projection in, [B,S,H·D]
# out. The kernels read q/k/v as strided views of the packed buffer and the
# backward stores dq/dk/dv directly into one dqkv buffer — no split-cat, no
# transpose copies anywhere around attention (torch's CatArrayBatchedCopy
# was 12 launches/step on GPT-2).
# --------------------------------------------------------------------------
def _qkv_views(t: torch.Tensor, H: int, Hk: int, D: int,
               bshd: bool = False):
    """q/k/v views of a packed [B,S,(H+2Hk)·D] buffer as [B,heads,S,D], or
    with ``bshd`` in the memory order [B,S,heads,D]."""
    B, S, Fdim = t.shape

    def view(heads, off):
        v = t.as_strided((B, S, heads, D), (S * Fdim, Fdim, D, 1),
                         t.storage_offset() + off)
        return v if bshd else v.permute(0, 2, 1, 3)

    return view(H, 0), view(Hk, H * D), view(Hk, (H + Hk) * D)


class _QKVAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, H, Hk, scale, kvlen, p_drop, site, q_lo=None,
                k_hi=None):
        m = require_ext()
        B, S, Fdim = qkv.shape
        D = Fdim // (H + 2 * Hk)
        q, k, v = _qkv_views(qkv, H, Hk, D)
        kv, rng = _mask_and_counter(kvlen, qkv)
        o_bshd, lse = m.attn_fwd(q, k, v, scale, kv, rng, site,
                                 p_drop, q_lo)   # [B,S,H,D] contiguous
        ctx.save_for_backward(qkv, o_bshd, lse, kv, rng, q_lo, k_hi)
        ctx.geom = (H, Hk, D, scale, site, p_drop)
        return o_bshd.view(B, S, H * D)

    @staticmethod
    def backward(ctx, do):
        m = require_ext()
        qkv, o_bshd, lse, kv, rng, q_lo, k_hi = ctx.saved_tensors
        H, Hk, D, scale, site, p_drop = ctx.geom
        B, S, Fdim = qkv.shape
        q, k, v = _qkv_views(qkv, H, Hk, D)
        do4 = do.view(B, S, H, D).permute(0, 2, 1, 3)
        if do4.stride(3) != 1:
            do4 = do.contiguous().view(B, S, H, D).permute(0, 2, 1, 3)
        dqkv = torch.empty_like(qkv)
        m.attn_bwd_packed(do4, q, k, v, o_bshd, lse, scale,
                          *_qkv_views(dqkv, H, Hk, D, bshd=True),
                          kv, rng, site, p_drop, q_lo, k_hi)
        return dqkv, None, None, None, None, None, None, None, None


def qkv_attention(qkv: torch.Tensor, n_head: int,
                  n_kv_head: Optional[int] = None,
                  scale: Optional[float] = None,
                  kvlen: Optional[torch.Tensor] = None,
                  p_drop: float = 0.0, site: int = 0,
                  q_lo: Optional[torch.Tensor] = None,
                  k_hi: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal attention over a packed qkv projection [B,S,(H+2Hk)·D] →
    [B,S,H·D]. GQA when n_kv_head < n_head. kvlen/p_drop/site/q_lo/k_hi as
    in :func:`causal_attention`."""
    Hk = n_kv_head or n_head
    B, S, Fdim = qkv.shape
    D = Fdim // (n_head + 2 * Hk)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if use_hip(qkv):
        q_lo, k_hi = _doc_bounds(q_lo, k_hi, qkv)
        return _QKVAttnFn.apply(qkv, n_head, Hk, scale, kvlen, p_drop, site,
                                q_lo, k_hi)
    E = n_head * D
    kvd = Hk * D
    q = qkv[..., :E].view(B, S, n_head, D).transpose(1, 2)
    k = qkv[..., E:E + kvd].view(B, S, Hk, D).transpose(1, 2)
    v = qkv[..., E + kvd:].view(B, S, Hk, D).transpose(1, 2)
    o = causal_attention(q, k, v, scale, kvlen, p_drop, site, q_lo, k_hi)
    return o.transpose(1, 2).reshape(B, S, E)


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, kv_len: int,
                     scale: Optional[float] = None,
                     kv_len_dev: Optional[torch.Tensor] = None
                     ) -> torch.Tensor:
    """Serving decode step: one new query per head attends the whole KV
    cache. q [B,H,D]; caches [B,Hk,Lmax,D] with the first kv_len rows
    valid. ``kv_len_dev`` (int32 [1] device counter holding the cache
    position BEFORE this token; effective length = *kv_len_dev + 1) makes
    the step hipGraph-replayable. Inference-only (no autograd)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if use_hip(q):
        return require_ext().attn_decode(
            q.contiguous(), k_cache, v_cache, kv_len, scale,
            kv_len_dev if kv_len_dev is not None
            else torch.empty(0, dtype=torch.int32, device=q.device))
    if kv_len_dev is not None:
        kv_len = int(kv_len_dev.item()) + 1
    qf = q.float().unsqueeze(2)                       # [B,H,1,D]
    B, Hk, _, D = k_cache.shape
    H = q.shape[1]
    kf = k_cache[:, :, :kv_len].float()
    vf = v_cache[:, :, :kv_len].float()
    if H != Hk:
        rep = H // Hk
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    att = torch.softmax((qf @ kf.transpose(-1, -2)) * scale, dim=-1)
    return (att @ vf).squeeze(2).to(q.dtype)


# --------------------------------------------------------------------------
# Fused log-softmax + cross entropy over the vocab dim
# --------------------------------------------------------------------------
class _CrossEntropyFn(torch.autograd.Function):
    """Sync-free on GPU: the non-ignored count stays a device scalar and the
    backward scale (dloss/count) is computed on device, so the whole loss
    path is hipGraph-capturable."""

    @staticmethod
    def forward(ctx, logits, targets, ignore_index):
        m = require_ext()
        logits = logits.contiguous()
        loss_sum, lse, count = m.ce_fwd(logits, targets, ignore_index)
        countf = count.clamp(min=1).to(torch.float32)
        ctx.save_for_backward(logits, targets, lse, countf)
        ctx.ignore_index = ignore_index
        return loss_sum / countf

    @staticmethod
    def backward(ctx, dloss):
        m = require_ext()
        logits, targets, lse, countf = ctx.saved_tensors
        scale_dev = (dloss.to(torch.float32) / countf).reshape(1)
        dlogits = m.ce_bwd(logits, targets, lse, scale_dev, 0.0,
                           ctx.ignore_index, 0, True)
        return dlogits, None, None


def cross_entropy_loss(logits: torch.Tensor, targets: torch.Tensor,
                       ignore_index: int = -100) -> torch.Tensor:
    """Mean CE over non-ignored targets. logits [T,V], targets [T]."""
    if use_hip(logits):
        return _CrossEntropyFn.apply(logits, targets, ignore_index)
    return F.cross_entropy(logits.float(), targets, ignore_index=ignore_index)


# --------------------------------------------------------------------------
# LM head + CE as one node, with a PIPELINED forward: the head GEMM runs
# tile-by-tile and each tile's online-softmax contribution is consumed on
# a side stream while the tile is still L2/Infinity-Cache resident —
# removing the 6.5 GB logits HBM re-read of the one-shot ce_fwd at the
# flagship shape AND overlapping the CE math with the next GEMM tile.
# Logits stay fully materialized (backward's ce_bwd + head GEMMs need
# them). Tile sizes keep two tiles inside the 256 MiB Infinity Cache.
# --------------------------------------------------------------------------
# NEGATIVE RESULT (r02, measured): the tiled pipeline loses 5.6 ms/step
# at the flagship shape (80.4 vs 74.9 ms) — the cache-resident tiles that
# make the CE read free also shrink the backward GEMMs to ~50-600
# workgroups (vs 256 CU x 8 slots), and the GEMM-efficiency loss dwarfs
# the ~1 ms of saved logits traffic. A strided-out variant writing tiles
# of ONE [T,V] buffer (big one-shot backward GEMMs kept) is blocked by
# TunableOp rejecting non-contiguous out (hipErrorInvalidValue at
# ld=50257). Default OFF; the machinery stays correct/tested/opt-in.
_CE_PIPE = _os.environ.get("DTA_CE_PIPELINE", "0") == "1"
_CE_TT = int(_os.environ.get("DTA_CE_TT", "8192"))
_CE_VC = int(_os.environ.get("DTA_CE_VC", "4224"))
# One-pass CE for training (no second 6.5 GB logits read, no second 6.5 GB
# buffer): tools/fused_backward_ab.py, profiles/r04_fused_backward.md.
# DTA_CE_FUSED=0 keeps ce_fwd + ce_bwd.
_CE_FUSED = _os.environ.get("DTA_CE_FUSED", "1") != "0"
# DTA_CE_FUSED=lds: the variant that holds the row in LDS (ce_fwd_bwd_lds_k),
# 0.38 ms faster but not bit-identical to ce_fwd + ce_bwd (ce.hip header)
_CE_FUSED_LDS = _os.environ.get("DTA_CE_FUSED", "1") == "lds"
_ce_stream: Optional[torch.cuda.Stream] = None


def _ce_side_stream() -> torch.cuda.Stream:
    global _ce_stream
    if _ce_stream is None:
        _ce_stream = torch.cuda.Stream()
    return _ce_stream


class _LMHeadCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, w, targets, ignore_index, allow_pipe,
                allow_fused=False):
        # NOTE: grad mode is always OFF inside Function.forward — the
        # caller decides pipe eligibility (allow_pipe) where grad state
        # is visible.
        m = require_ext()
        T, _K = x2.shape
        V = w.shape[0]
        pipe = _CE_PIPE and allow_pipe and T >= 2 * _CE_TT
        # the caller gave the logits up: one kernel reduces each row and
        # overwrites it with its gradient (ce.hip, ce_fwd_bwd_k)
        fused = _CE_FUSED and allow_fused and not pipe
        if pipe:
            # tiled: per-(token, vocab) tile CONTIGUOUS buffers — the GEMM
            # writes a tile, the side stream folds its online-softmax
            # contribution while the next GEMM runs, and backward re-walks
            # the tiles so each dlogits tile feeds its two head GEMMs
            # straight out of cache.
            mr = torch.full((T,), float("-inf"), dtype=torch.float32,
                            device=x2.device)
            sr = torch.zeros(T, dtype=torch.float32, device=x2.device)
            tl = torch.zeros(T, dtype=torch.float32, device=x2.device)
            tiles = []
            main = torch.cuda.current_stream()
            side = _ce_side_stream()
            for t0 in range(0, T, _CE_TT):
                te = min(t0 + _CE_TT, T)
                xt = x2[t0:te]
                for v0 in range(0, V, _CE_VC):
                    ve = min(v0 + _CE_VC, V)
                    tile = torch.empty(te - t0, ve - v0, dtype=x2.dtype,
                                       device=x2.device)
                    torch.mm(xt, w[v0:ve].t(), out=tile)
                    side.wait_stream(main)
                    with torch.cuda.stream(side):
                        m.ce_chunk(tile, targets[t0:te], v0, tl[t0:te],
                                   mr[t0:te], sr[t0:te])
                    tiles.append(tile)
            main.wait_stream(side)
            loss_sum, lse, count = m.ce_finalize(targets, mr, sr, tl,
                                                 ignore_index)
            logits = x2.new_empty(0)
        elif fused:
            # the logits buffer comes back holding dlogits for dloss == 1
            dlog = x2.mm(w.t())
            # the count depends on the targets alone and the kernel needs
            # its reciprocal up front: this is the one place it is computed
            count = (targets != ignore_index).sum()
            inv = count.clamp(min=1).to(torch.float32).reciprocal()
            loss_sum, lse, _ = m.ce_fwd_bwd(dlog, targets.contiguous(),
                                            ignore_index, inv.reshape(1),
                                            0, _CE_FUSED_LDS)
            tiles = [dlog]
            logits = x2.new_empty(0)
        else:
            logits = x2.mm(w.t())
            loss_sum, lse, count = m.ce_fwd(logits, targets, ignore_index)
            tiles = [logits]
        countf = count.clamp(min=1).to(torch.float32)
        ctx.save_for_backward(x2, w, targets, lse, countf, *tiles)
        ctx.ignore_index = ignore_index
        ctx.pipe = pipe
        ctx.fused = fused
        ctx.dims = (T, V)
        ctx.wgrad = getattr(w, "main_grad", None)
        ctx.mark_non_differentiable(logits)
        # without this, autograd MATERIALIZES a logits-shaped zeros as the
        # incoming grad for the non-differentiable output — a 6.5 GB
        # fill (~1.1 ms/step) that profiling caught as anonymous
        # FillFunctor kernels
        ctx.set_materialize_grads(False)
        return loss_sum / countf, logits

    @staticmethod
    def backward(ctx, dloss, _dlogits):
        m = require_ext()
        x2, w, targets, lse, countf, *tiles = ctx.saved_tensors
        ii = ctx.ignore_index
        if ctx.fused:
            # dlog was made for dloss == 1; the device scalar goes on the
            # small [T, K] side of each GEMM. PRECISION for dloss != 1:
            # dloss is rounded to the activation dtype first, so a scale
            # bf16 cannot hold (1/3, say) puts a relative error of up to
            # 2^-9 on every head-path gradient, and dx / x2*dl are rounded
            # once more. The unfused path applies fp32 dloss/count inside
            # ce_bwd before its single rounding. dloss == 1 (training, the
            # benchmark) and powers of two (loss scaling) are exact.
            dlog = tiles[0]
            dl = dloss.to(x2.dtype)
            dx = dlog.mm(w) * dl
            if ctx.wgrad is not None:
                ctx.wgrad.addmm_(dlog.t(), x2 * dl)
                dw = None
            else:
                dw = dlog.t().mm(x2 * dl)
            return dx, dw, None, None, None, None
        scale_dev = (dloss.to(torch.float32) / countf).reshape(1)
        if not ctx.pipe:
            dlog = m.ce_bwd(tiles[0], targets, lse, scale_dev, 0.0, ii,
                            0, True)
            dx = dlog.mm(w)
            if ctx.wgrad is not None:
                ctx.wgrad.addmm_(dlog.t(), x2)   # flat-plane accumulation
                dw = None
            else:
                dw = dlog.t().mm(x2)
            return dx, dw, None, None, None, None
        T, V = ctx.dims
        dx = torch.empty_like(x2)
        dw = None if ctx.wgrad is not None else torch.zeros_like(w)
        i = 0
        for t0 in range(0, T, _CE_TT):
            te = min(t0 + _CE_TT, T)
            first = True
            for v0 in range(0, V, _CE_VC):
                ve = min(v0 + _CE_VC, V)
                # no nontemporal: dlog is re-read by both GEMMs right away
                dlog = m.ce_bwd(tiles[i], targets[t0:te], lse[t0:te],
                                scale_dev, 0.0, ii, v0, False)
                i += 1
                if first:
                    torch.mm(dlog, w[v0:ve], out=dx[t0:te])
                    first = False
                else:
                    dx[t0:te].addmm_(dlog, w[v0:ve])
                if ctx.wgrad is not None:
                    ctx.wgrad[v0:ve].addmm_(dlog.t(), x2[t0:te])
                else:
                    dw[v0:ve].addmm_(dlog.t(), x2[t0:te])
        return dx, dw, None, None, None, None


def lm_head_ce(x: torch.Tensor, w: torch.Tensor, targets: torch.Tensor,
               ignore_index: int = -100, need_logits: bool = True,
               overwrite_logits: bool = False):
    """(loss, logits) = mean-CE(x @ wᵀ, targets) as one node. x [..., E]
    is flattened to [T, E]. With ``need_logits=False`` (training) the
    pipelined tiled path may engage and logits come back as ``None``.
    ``overwrite_logits=True`` with it gives the logits up for good: one
    kernel turns the buffer into its own gradient (no second [T, V] pass
    or buffer) and logits always come back as ``None``."""
    x2 = x.reshape(-1, x.shape[-1])
    if use_hip(x):
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        allow_pipe = not need_logits and torch.is_grad_enabled()
        loss, logits = _LMHeadCEFn.apply(x2, w, targets, ignore_index,
                                         allow_pipe,
                                         allow_pipe and overwrite_logits)
        return loss, (logits if logits.numel() else None)
    logits = F.linear(x2, w)
    loss = F.cross_entropy(logits.float(), targets,
                           ignore_index=ignore_index)
    return loss, logits


# --------------------------------------------------------------------------
# Fused LM-head LOSS, forward only (hip/head_loss.hip): a hand-written MFMA
# head GEMM whose accumulator tiles are folded into an online log-sum-exp
# in-register — the [T, V] logits are never written. For the no-grad
# consumers (validator scoring, cached base loss, sharded validation) that
# throw the logits away; training keeps lm_head_ce, whose backward re-reads
# them. Measured A/B: tools/head_loss_ab.py, profiles/r03_head_loss_ab.md.
# --------------------------------------------------------------------------
def _head_loss_supported(x2: torch.Tensor, w: torch.Tensor) -> bool:
    """Shapes head_loss.hip takes: bf16, K % 64 == 0, dense 16 B-aligned
    rows. Anything else keeps the library-GEMM + ce_fwd split."""
    return (x2.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
            and w.dim() == 2 and x2.shape[-1] % 64 == 0
            and w.is_contiguous()
            and x2.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0)


def lm_head_loss(x: torch.Tensor, w: torch.Tensor, targets: torch.Tensor,
                 ignore_index: int = -100, return_lse: bool = False):
    """Mean CE of ``x @ wᵀ`` against ``targets`` over non-ignored targets,
    WITHOUT materializing the logits. x [..., K] is flattened to [T, K],
    w is [V, K], targets has T elements. Returns a detached device scalar
    (0.0 when every target is ignored), or ``(loss, lse)`` with the per-row
    natural-log lse [T] (fp32) when ``return_lse`` is set.

    Forward-only: this is not an autograd node. Asking for it with grad
    enabled on inputs that require grad is an error — use ``lm_head_ce``.
    Sync-free and hipGraph-capturable on GPU."""
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad):
        raise RuntimeError(
            "ops.lm_head_loss is forward-only (it keeps no logits for a "
            "backward pass); call it under torch.no_grad(), or use "
            "ops.lm_head_ce for a differentiable head + loss")
    with torch.no_grad():
        x2 = x.detach().reshape(-1, x.shape[-1])
        w = w.detach()
        tg = targets.reshape(-1)
        if use_hip(x2):
            m = require_ext()
            if not x2.is_contiguous():
                x2 = x2.contiguous()
            if not tg.is_contiguous():
                tg = tg.contiguous()
            if not _head_loss_supported(x2, w):
                # library GEMM + our CE kernel, the same split `linear`
                # makes for GEMV
                loss, logits = lm_head_ce(x2, w, tg, ignore_index)
                if not return_lse:
                    return loss
                return loss, m.ce_fwd(logits, tg, ignore_index)[1]
            loss_sum, lse, count, _tl = m.head_loss_fwd(x2, w, tg,
                                                        ignore_index, 0)
            loss = loss_sum / count.clamp(min=1).to(torch.float32)
            return (loss, lse) if return_lse else loss
        logits = F.linear(x2.float(), w.float())
        valid = tg != ignore_index
        lse = torch.logsumexp(logits, dim=-1)
        tl = logits.gather(1, tg.clamp(min=0).unsqueeze(1)).squeeze(1)
        loss = (torch.where(valid, lse - tl, torch.zeros_like(lse)).sum()
                / valid.sum().clamp(min=1).to(torch.float32))
        return (loss, lse) if return_lse else loss


# --------------------------------------------------------------------------
# Embedding: fused token+position gather (and scatter-add backward)
# --------------------------------------------------------------------------
class _EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, wte, wpe, doc_start=None):
        m = require_ext()
        ids = ids.contiguous()
        ctx.save_for_backward(ids, doc_start)
        ctx.vocab, ctx.npos = wte.shape[0], (wpe.shape[0] if wpe is not None else 0)
        ctx.dim = wte.shape[1]
        ctx.dtype = wte.dtype
        ctx.wteg = getattr(wte, "main_grad", None)
        ctx.wpeg = (getattr(wpe, "main_grad", None)
                    if wpe is not None else None)
        return m.embedding_fwd(ids, wte, wpe if wpe is not None else torch.empty(0, dtype=wte.dtype, device=wte.device), torch.empty(0, dtype=torch.int32, device=wte.device), doc_start)

    @staticmethod
    def backward(ctx, dy):
        m = require_ext()
        ids, doc_start = ctx.saved_tensors
        dwte32, dwpe32 = m.embedding_bwd(dy.contiguous(), ids, ctx.vocab,
                                         ctx.npos, doc_start)
        dwte = _grad_out(dwte32, ctx.wteg, ctx.dtype)
        dwpe = (_grad_out(dwpe32, ctx.wpeg, ctx.dtype) if ctx.npos
                else None)
        return None, dwte, dwpe, None


def embedding_fwd(ids: torch.Tensor, wte: torch.Tensor,
                  wpe: Optional[torch.Tensor] = None,
                  pos: Optional[torch.Tensor] = None,
                  doc_start: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x[b,s,:] = wte[ids[b,s]] (+ wpe[pos + s] if given). ``pos``: int32
    [1] DEVICE offset — graph-replayable decode (inference-only path).
    ``doc_start`` (int32, ids-shaped; packed sequences, the attention
    q_lo): positions restart per document, wpe[s - doc_start[b,s]]. Not
    combined with ``pos``. It must be a DOCUMENT LAYOUT, which is more than
    the q_lo contract: every value is the index of a column that starts a
    document, doc_start[b, doc_start[b,s]] == doc_start[b,s] (what
    ``packed_text_batches`` produces; :func:`check_doc_start` checks it on
    the host). The GPU backward finds the documents as the columns with
    doc_start[b,s] == s; for a q_lo that is no document layout (a sliding
    window) its dwpe would not be the gradient of the forward."""
    if doc_start is not None:
        if pos is not None:
            raise ValueError("doc_start and pos cannot be combined")
        if (doc_start.dtype != torch.int32
                or doc_start.shape != ids.shape):
            raise ValueError("doc_start must be int32 and shaped like ids")
        if wpe is None:
            doc_start = None   # no position table: nothing restarts
    if use_hip(wte):
        if pos is not None:   # serving decode: no autograd needed
            return require_ext().embedding_fwd(
                ids.contiguous(), wte,
                wpe if wpe is not None else torch.empty(
                    0, dtype=wte.dtype, device=wte.device), pos)
        return _EmbeddingFn.apply(
            ids, wte, wpe,
            doc_start.contiguous() if doc_start is not None else None)
    x = F.embedding(ids, wte)
    if doc_start is not None:
        check_doc_start(doc_start.view(-1, ids.shape[-1]))
        posn = torch.arange(ids.shape[-1], device=ids.device) - doc_start.long()
        return x + wpe[posn]
    if wpe is not None:
        off = int(pos.item()) if pos is not None else 0
        x = x + wpe[off:off + ids.shape[-1]].unsqueeze(0)
    return x


# --------------------------------------------------------------------------
# RoPE (Llama): rotate q,k in-place-free
# --------------------------------------------------------------------------
class _RopeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin):
        m = require_ext()
        ctx.save_for_backward(cos, sin)
        e = torch.empty(0, dtype=torch.int32, device=x.device)
        ctx.e = e
        return m.rope_fwd(x.contiguous(), cos, sin, e)

    @staticmethod
    def backward(ctx, dy):
        m = require_ext()
        cos, sin = ctx.saved_tensors
        return m.rope_bwd(dy.contiguous(), cos, sin, ctx.e), None, None


def rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
         pos: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Apply rotary embedding to x [B,H,S,D] with cos/sin [S,D/2] (fp32;
    other dtypes are upcast — Module.to(bf16) casts registered buffers).
    ``pos``: int32 [1] DEVICE offset into the tables (graph-replayable
    decode; inference-only path)."""
    if cos.dtype != torch.float32:
        cos = cos.float()
        sin = sin.float()
    if use_hip(x):
        if pos is not None:   # serving decode: no autograd needed
            return require_ext().rope_fwd(x.contiguous(), cos, sin, pos)
        return _RopeFn.apply(x, cos, sin)
    off = int(pos.item()) if pos is not None else 0
    xf = x.float()
    d2 = x.shape[-1] // 2
    x1, x2 = xf[..., :d2], xf[..., d2:]
    c = cos[off:off + x.shape[-2]].view(1, 1, x.shape[-2], d2)
    s = sin[off:off + x.shape[-2]].view(1, 1, x.shape[-2], d2)
    out = torch.cat([x1 * c - x2 * s, x1 * s + x2 * c], dim=-1)
    return out.to(x.dtype)


# --------------------------------------------------------------------------
# Fused AdamW over flat buffers (reference: optimizer.step(),
# training_manager.py:391 — torch AdamW; here one kernel over one buffer)
# --------------------------------------------------------------------------
def adamw_step(master: torch.Tensor, grad: torch.Tensor, m: torch.Tensor,
               v: torch.Tensor, out_bf16: Optional[torch.Tensor], step: int,
               lr: float, beta1: float = 0.9, beta2: float = 0.999,
               eps: float = 1e-8, weight_decay: float = 0.01,
               bc: Optional[torch.Tensor] = None) -> None:
    """Decoupled AdamW (torch semantics): in-place update of fp32 master,
    m, v; optionally writes the bf16 working copy. ``bc`` (fp32[2] device
    buffer from adamw_tick) replaces host bias correction for the
    hipGraph-capturable path."""
    if use_hip(master):
        require_ext().adamw_step(master, grad, m, v,
                                 out_bf16 if out_bf16 is not None else master.new_empty(0).to(torch.bfloat16),
                                 step, lr, beta1, beta2, eps, weight_decay,
                                 bc if bc is not None else master.new_empty(0))
        return
    g = grad.float()
    master.mul_(1.0 - lr * weight_decay)
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (v / bc2).sqrt_().add_(eps)
    master.addcdiv_(m, denom, value=-lr / bc1)
    if out_bf16 is not None:
        out_bf16.copy_(master.to(out_bf16.dtype))


def adamw_tick(t_dev: torch.Tensor, bc_dev: torch.Tensor,
               beta1: float, beta2: float) -> None:
    """Advance the device-side AdamW step counter and refresh the bias
    correction buffer (graph-capturable; see adamw_step's ``bc``)."""
    require_ext().adamw_tick(t_dev, bc_dev, beta1, beta2)


# --------------------------------------------------------------------------
# Guarded step: gradient clipping, non-finite skip and the LR schedule with
# no host round-trip. grad_sumsq_partials -> step_control ->
# adamw_step_guarded talk through a device control block
#   ctl_f fp32[6]  {lr, coef, grad_norm, bc1, bc2, unused}
#   ctl_i int32[4] {t, sched_step, skip_now, skipped_total}
# (hip/adamw.hip). The CPU paths keep the block in host tensors and have the
# same semantics.
# --------------------------------------------------------------------------
LR_SCHEDULES = ("constant", "linear", "cosine")
CTL_LR, CTL_COEF, CTL_NORM, CTL_BC1, CTL_BC2 = range(5)
CTL_T, CTL_SCHED, CTL_SKIP_NOW, CTL_SKIPPED = range(4)


def lr_schedule(schedule: str, s: int, lr_max: float, min_lr: float = 0.0,
                warmup_steps: int = 0, total_steps: int = 0) -> float:
    """The schedule's value at step ``s`` (counted from 1), in double: linear
    warmup to ``lr_max``, then constant, or linear / cosine decay to
    ``min_lr`` at ``total_steps`` and flat after it."""
    if s <= warmup_steps:
        return lr_max * s / warmup_steps
    if schedule == "constant":
        return lr_max
    p = min(1.0, (s - warmup_steps) / max(1, total_steps - warmup_steps))
    if schedule == "linear":
        return lr_max + (min_lr - lr_max) * p
    assert schedule == "cosine", schedule
    return min_lr + 0.5 * (lr_max - min_lr) * (1.0 + math.cos(math.pi * p))


def grad_sumsq_blocks(n: int, dtype: torch.dtype,
                      device: torch.device) -> int:
    """Length of the partial buffer grad_sumsq_partials fills for a plane of
    ``n`` elements: a fixed function of n and dtype."""
    if torch.device(device).type == "cuda":
        return int(require_ext().grad_sumsq_blocks(
            n, dtype == torch.bfloat16))
    return 1


def grad_sumsq_partials(flat: torch.Tensor, out: torch.Tensor) -> None:
    """out[b] = partial sum of squares of ``flat`` (bf16 or fp32); the
    partials add up to |flat|^2. Every element of ``out`` is stored, with no
    atomics, so the values repeat bit for bit. A bf16 value whose square
    overflows fp32 gives an infinite partial."""
    if use_hip(flat):
        require_ext().grad_sumsq_partials(flat, out)
        return
    out.zero_()
    out[0] = flat.double().pow(2).sum().to(torch.float32)


def step_control(partials: Optional[torch.Tensor], ctl_f: torch.Tensor,
                 ctl_i: torch.Tensor, beta1: float, beta2: float,
                 max_norm: float = 0.0, skip_nonfinite: bool = False,
                 schedule: str = "constant", lr_max: float = 5e-4,
                 min_lr: float = 0.0, warmup_steps: int = 0,
                 total_steps: int = 0) -> None:
    """The tick of a guarded step. Folds ``partials`` (None: no norm taken)
    in double, then writes the control block: grad_norm, the clip factor
    coef = min(1, max_norm / (norm + 1e-6)) (1 when max_norm <= 0), skip_now
    = skip_nonfinite and the sum is not finite, sched_step += 1, lr =
    lr_schedule(sched_step), and, unless skipping, t += 1 with the bias
    corrections of t. With skip_nonfinite off a non-finite norm is not
    special-cased: coef is whatever the formula gives, as in
    torch.nn.utils.clip_grad_norm_."""
    sched = LR_SCHEDULES.index(schedule)
    if use_hip(ctl_f):
        require_ext().step_control(
            partials if partials is not None else ctl_f.new_empty(0), ctl_f,
            ctl_i, beta1, beta2, max_norm, skip_nonfinite, sched, lr_max,
            min_lr, warmup_steps, total_steps)
        return
    import numpy as np
    if partials is None and (max_norm > 0 or skip_nonfinite):
        raise ValueError("clipping and the non-finite skip need the norm "
                         "partials")
    total = float(partials.double().sum()) if partials is not None else 0.0
    with np.errstate(all="ignore"):
        norm = np.float32(np.sqrt(np.float64(total)))
        coef = np.float32(1.0)
        if max_norm > 0:
            c = np.float32(max_norm) / (norm + np.float32(1e-6))
            coef = np.float32(1.0) if c > 1.0 else c
    skip = bool(skip_nonfinite and not math.isfinite(total))
    s = int(ctl_i[CTL_SCHED]) + 1
    ctl_i[CTL_SCHED] = s
    if not skip:
        t = int(ctl_i[CTL_T]) + 1
        ctl_i[CTL_T] = t
        ctl_f[CTL_BC1] = 1.0 - beta1 ** t
        ctl_f[CTL_BC2] = 1.0 - beta2 ** t
    ctl_f[CTL_LR] = lr_schedule(schedule, s, lr_max, min_lr, warmup_steps,
                                total_steps)
    ctl_f[CTL_COEF] = float(coef)
    ctl_f[CTL_NORM] = float(norm)
    ctl_i[CTL_SKIP_NOW] = int(skip)
    ctl_i[CTL_SKIPPED] += int(skip)


def adamw_step_guarded(master: torch.Tensor, grad: torch.Tensor,
                       m: torch.Tensor, v: torch.Tensor,
                       out_bf16: Optional[torch.Tensor], ctl_f: torch.Tensor,
                       ctl_i: torch.Tensor, beta1: float = 0.9,
                       beta2: float = 0.999, eps: float = 1e-8,
                       weight_decay: float = 0.01) -> None:
    """adamw_step with lr, the bias corrections and the clip factor read
    from the control block step_control wrote. skip_now set: nothing is
    touched. The clip factor scales the gradient in registers; ``grad``
    itself is never modified."""
    if use_hip(master):
        require_ext().adamw_step_guarded(
            master, grad, m, v,
            out_bf16 if out_bf16 is not None
            else master.new_empty(0).to(torch.bfloat16),
            ctl_f, ctl_i, beta1, beta2, eps, weight_decay)
        return
    if int(ctl_i[CTL_SKIP_NOW]):
        return
    lr, coef, _, bc1, bc2, _ = ctl_f.tolist()
    g = grad.float() * coef
    master.mul_(1.0 - lr * weight_decay)
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    denom = (v / bc2).sqrt_().add_(eps)
    master.addcdiv_(m, denom, value=-lr / bc1)
    if out_bf16 is not None:
        out_bf16.copy_(master.to(out_bf16.dtype))


# --------------------------------------------------------------------------
# Delta / merge primitives over flat buffers
# --------------------------------------------------------------------------
def delta_sub(w: torch.Tensor, base: torch.Tensor,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """delta = w − base (reference: training_manager.py:417-421)."""
    if out is None:
        out = torch.empty_like(base)
    if use_hip(w):
        require_ext().delta_sub(w, base, out)
        return out
    torch.sub(w.float(), base.float(), out=out)
    return out


def _packed(x) -> bool:
    """A parallel.comm.PackedDeltas (named by shape: comm imports ops)."""
    return not isinstance(x, torch.Tensor) and hasattr(x, "kind")


def _packed_args(pd):
    """(data, scales, block) as the packed bindings take them."""
    scales = (pd.scales if pd.scales is not None
              else torch.empty(0, dtype=torch.float32, device=pd.data.device))
    return pd.data, scales, pd.block


def quantize_blockwise_int8(flat: torch.Tensor, block: int = 4096,
                            base: Optional[torch.Tensor] = None):
    """(int8 codes [nb*block], fp32 scales [nb]) of ``flat``, or of
    ``flat - base``. The definition is parallel.comm.quantize_blockwise_int8
    (the CPU path); the GPU kernel equals it bit for bit, reads both planes
    once and never writes the fp32 difference."""
    if use_hip(flat):
        def plane(t):
            # the kernel reads 16 B vectors: a row of an odd-width stack
            # is copied to an allocation of its own
            t = t.contiguous()
            return t if t.data_ptr() % 16 == 0 else t.clone()
        q, scale = require_ext().quantize_int8(
            plane(flat), flat.new_empty(0) if base is None else plane(base),
            block)
        return q, scale
    from ..parallel.comm import quantize_blockwise_int8 as _q
    return _q(flat if base is None else flat.float() - base.float(), block)


def _plane16(t: torch.Tensor) -> torch.Tensor:
    """Contiguous and 16 B aligned, as the kernels' vector loads need."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def topk_compress_blockwise(flat: torch.Tensor, k: int = 128,
                            block: int = 4096,
                            base: Optional[torch.Tensor] = None,
                            residual: Optional[torch.Tensor] = None,
                            update_residual: bool = True):
    """Blockwise top-k entries of ``d = (flat - base) + residual`` (``base``
    and ``residual`` optional): ``(entries int32 [nb*k], residual)``.

    The definition is parallel.comm.topk_compress_blockwise (the CPU path);
    the GPU kernel equals it bit for bit, reads every plane once and never
    writes ``d``. With ``update_residual`` the fp32 [P] ``residual`` tensor
    is overwritten in place with the error-feedback remainder and returned
    (a fresh one is made when ``residual`` is None); without it ``residual``
    is left untouched and returned as it came."""
    from ..parallel.comm import check_topk_format, \
        topk_compress_blockwise as _t
    check_topk_format(k, block)
    if residual is not None and (residual.dtype != torch.float32
                                 or residual.numel() != flat.numel()
                                 or not residual.is_contiguous()):
        raise ValueError("residual must be a contiguous fp32 [P] tensor")
    if use_hip(flat):
        e = flat.new_empty(0)
        if residual is not None and residual.data_ptr() % 16 != 0:
            raise ValueError("residual must be 16-byte aligned")
        out = e
        if update_residual:
            out = residual if residual is not None else torch.empty(
                flat.numel(), dtype=torch.float32, device=flat.device)
        # the top-k form of the extension's delta compressor (topk_k > 0)
        ent, = require_ext().quantize_int8(
            _plane16(flat), e if base is None else _plane16(base), block,
            topk_k=k, residual_in=residual,
            residual_out=out if update_residual else None)
        return ent, (out if update_residual else residual)
    d = flat.float() if base is None else flat.float() - base.float()
    ent, res = _t(d.reshape(-1), k, block, residual)
    if not update_residual:
        return ent, residual
    if residual is not None:
        residual.copy_(res)
        res = residual
    return ent, res


def dequantize_blockwise_int8(q: torch.Tensor, scale: torch.Tensor,
                              numel: int, block: int = 4096) -> torch.Tensor:
    """fp32 [numel] of one quantised row: float(q) * scale per block."""
    if use_hip(q):
        out = torch.zeros(numel, dtype=torch.float32, device=q.device)
        # 1.0 * d + 0.0 is d
        require_ext().axpy_packed(out, q.view(1, -1), scale.view(1, -1),
                                  block, 0, 1.0)
        return out
    from ..parallel.comm import dequantize_blockwise_int8 as _dq
    return _dq(q, scale, numel, block)


def axpy_(w: torch.Tensor, x, alpha: float = 1.0) -> torch.Tensor:
    """w += alpha·x (reference delta apply: validation_logic.py:252-259).
    ``x``: a tensor, or ``(PackedDeltas, i)`` for row ``i`` of a packed
    gather — dequantised in registers, no fp32 copy of the delta.

    A "topk" row is a pure scatter, ``w[e] = fma(alpha, v, w[e])`` over its
    in-range entries. For finite ``alpha`` that equals the dense kernel on
    the densified row as numbers; elements off the support are not touched,
    so a ``-0.0`` in ``w`` that the dense kernel would turn into ``+0.0``
    may stay ``-0.0``."""
    if isinstance(x, tuple):
        pd, i = x
        if pd.kind == "fp32":
            return axpy_(w, pd.data[i], alpha)
        if use_hip(w):
            require_ext().axpy_packed(w, *_packed_args(pd), i, alpha)
            return w
        return w.add_(pd.row(i).to(w.dtype), alpha=alpha)
    if use_hip(w):
        require_ext().axpy(w, x, alpha)
        return w
    return w.add_(x.to(w.dtype), alpha=alpha)


def weighted_merge(base: torch.Tensor, deltas,
                   W: torch.Tensor, offsets: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """merged[e] = Σ_i W[i, seg(e)] · (base[e] + deltas[i,e]).

    ``W`` is [N, S] per-(miner, parameter-tensor) merge weights; ``offsets``
    [S+1] the flat-buffer segment boundaries. Reference semantics:
    averaging_logic.py:422-470 (get_averaged_params over per-param weights).
    ``deltas``: [N, P] fp32, or a PackedDeltas (bf16 / int8 / topk stay
    compressed in memory; the result equals this call on
    ``deltas.dequantize()``).
    """
    if _packed(deltas) and deltas.kind == "fp32":
        deltas = deltas.data
    N, P = deltas.shape
    if out is None:
        out = torch.empty_like(base)
    if use_hip(base):
        if _packed(deltas):
            require_ext().weighted_merge_packed(
                base, *_packed_args(deltas), W, offsets.to(base.device), out)
            return out
        require_ext().weighted_merge(base, deltas, W, offsets.to(base.device), out)
        return out
    seg = _seg_ids(offsets, P)
    acc = torch.zeros(P, dtype=torch.float32)
    for i in range(N):
        di = deltas.row(i) if _packed(deltas) else deltas[i].float()
        acc += W[i].float()[seg] * (base.float() + di)
    out.copy_(acc.to(out.dtype))
    return out


# --------------------------------------------------------------------------
# Robust merge: coordinate-wise trimmed mean / median
# --------------------------------------------------------------------------
MERGE_MAX_MODELS = 32    # DTA_MERGE_MAX_MODELS of the kernels
_KEY_NAN = 0xFFFFFFFF
_TRIM_CHUNK = 1 << 20    # elements per slice of the CPU path (int64 keys)


def median_trim(n: int) -> int:
    """The ``trim`` that makes :func:`trimmed_merge` a coordinate-wise
    median: the middle value for odd ``n``, the mean of the two middle
    values for even ``n``."""
    return (n - 1) // 2


def _order_keys(v: torch.Tensor) -> torch.Tensor:
    """int64 order keys (values in [0, 2^32)) of an fp32 tensor: the bit
    pattern with every bit flipped where the sign bit is set and only the
    sign bit flipped elsewhere, so integer order is
    -inf < .. < -0.0 < +0.0 < .. < +inf; every NaN is 0xFFFFFFFF."""
    b = v.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    key = torch.where(b >= 0x80000000, b ^ 0xFFFFFFFF, b ^ 0x80000000)
    return torch.where(torch.isnan(v), torch.full_like(key, _KEY_NAN), key)


def _key_values(key: torch.Tensor) -> torch.Tensor:
    """The fp32 values of int64 order keys; the NaN key is 0x7FC00000."""
    b = torch.where(key >= 0x80000000, key ^ 0x80000000, key ^ 0xFFFFFFFF)
    b = torch.where(key == _KEY_NAN, torch.full_like(b, 0x7FC00000), b)
    b = torch.where(b >= 0x80000000, b - (1 << 32), b)   # as signed 32 bit
    return b.to(torch.int32).view(torch.float32)


def _trimmed_merge_cpu(base, rows, trim, out, outside):
    """The definition. rows(lo, hi) -> [N, hi - lo] fp32 of the deltas."""
    N = outside.numel()
    m = torch.tensor(float(N - 2 * trim), dtype=torch.float32)
    canon = torch.tensor(0x7FC00000, dtype=torch.int32).view(torch.float32)
    P = base.numel()
    for lo in range(0, P, _TRIM_CHUNK):
        hi = min(lo + _TRIM_CHUNK, P)
        keys = _order_keys(rows(lo, hi))
        srt, _ = torch.sort(keys, dim=0)
        vals = _key_values(srt[trim:N - trim])
        acc = vals[0].clone()            # starts FROM the first kept value
        for j in range(1, N - 2 * trim):
            acc = acc + vals[j]
        o = base[lo:hi] + acc / m
        # inf - inf has no one NaN across machines: every NaN is 0x7FC00000
        out[lo:hi] = torch.where(torch.isnan(o), canon, o)
        outside += ((keys < srt[trim]) | (keys > srt[N - 1 - trim])).sum(dim=1)


def trimmed_merge(base: torch.Tensor, deltas, trim: int,
                  out: Optional[torch.Tensor] = None,
                  outside: Optional[torch.Tensor] = None):
    """Coordinate-wise trimmed mean of N deltas on top of ``base``:
    ``(out fp32 [P], outside int64 [N])``.

    For every element e on its own the N values ``deltas[i, e]`` are put in
    the total order -inf < .. < -0.0 < +0.0 < .. < +inf < NaN, the ``trim``
    smallest and the ``trim`` largest are dropped, and the ``m = N - 2 trim``
    kept ones are summed in ascending order starting from the first of them
    (plain fp32 adds); ``out[e] = base[e] + sum / m`` with one IEEE division
    and one add. A NaN result is always 0x7FC00000. ``outside[i]`` counts the
    elements at which miner i lies strictly outside the kept interval (a tie
    with its boundary counts for nobody), so it does not depend on the row
    order; neither does any bit of ``out``. ``trim = median_trim(N)`` is the
    median; ``trim = 0`` a mean that, unlike ``weighted_merge``, does not
    depend on the order of the miners. A NaN or an infinity sent by at most
    ``trim`` miners at an element is trimmed there like any other outlier.

    ``base`` fp32 [P]; ``deltas`` [N, P] fp32 or a PackedDeltas of kind
    fp32 / bf16 / int8 (dequantised as in ``weighted_merge``), 1 <= N <= 32,
    0 <= 2 trim < N. A "topk" PackedDeltas is refused: most coordinates are
    sent by fewer than half of the miners, so a coordinate-wise median would
    zero almost everything. ``out`` / ``outside``, where given, are
    overwritten. Both results live on ``base``'s device; the op does not
    sync. The CPU path is the definition, the GPU kernel equals it bit for
    bit (hip/merge.hip, trimmed_merge_k)."""
    if _packed(deltas):
        if deltas.kind == "topk":
            raise ValueError(
                "trimmed_merge: top-k deltas are refused. Most coordinates "
                "are sent by fewer than half of the miners, so a "
                "coordinate-wise median would zero almost every element; "
                "exchange fp32, bf16 or int8 deltas for the robust merge")
        if deltas.kind == "fp32":
            deltas = deltas.data
    if not _packed(deltas) and (deltas.dim() != 2
                                or deltas.dtype != torch.float32):
        raise ValueError("trimmed_merge: deltas must be an fp32 [N, P] "
                         "tensor or a PackedDeltas")
    N, P = deltas.shape
    trim = int(trim)
    if not 1 <= N <= MERGE_MAX_MODELS:
        raise ValueError(f"trimmed_merge: 1 <= N <= {MERGE_MAX_MODELS}, "
                         f"got {N}")
    if trim < 0 or 2 * trim >= N:
        raise ValueError(f"trimmed_merge: need 0 <= 2 * trim < N, got trim "
                         f"{trim} for {N} deltas")
    if base.dtype != torch.float32 or base.dim() != 1 or base.numel() != P:
        raise ValueError("trimmed_merge: base must be fp32 [P]")
    if out is None:
        out = torch.empty_like(base)
    elif out.dtype != torch.float32 or tuple(out.shape) != (P,):
        raise ValueError("trimmed_merge: out must be fp32 [P]")
    if outside is None:
        outside = torch.zeros(N, dtype=torch.int64, device=base.device)
    elif outside.dtype != torch.int64 or tuple(outside.shape) != (N,):
        raise ValueError("trimmed_merge: outside must be int64 [N]")
    else:
        outside.zero_()
    if use_hip(base):
        if _packed(deltas):
            data, scales, block = _packed_args(deltas)
        else:
            data, scales, block = deltas, base.new_empty(0), 0
        require_ext().robust.trimmed_merge(base, data, scales, block, trim,
                                           out, outside)
        return out, outside
    if _packed(deltas):
        if deltas.kind == "bf16":
            def rows(lo, hi):
                return deltas.data[:, lo:hi].to(torch.float32)
        else:
            full = deltas.dequantize()

            def rows(lo, hi):
                return full[:, lo:hi]
    else:
        def rows(lo, hi):
            return deltas[:, lo:hi]
    _trimmed_merge_cpu(base, rows, trim, out, outside)
    return out, outside


def grad_merge_weights(g: torch.Tensor, base: torch.Tensor,
                       deltas, merged: torch.Tensor,
                       offsets: torch.Tensor) -> torch.Tensor:
    """grad_W[i,j] = Σ_{e∈seg j} g[e] · (base[e]+deltas[i,e] − merged[e]).

    The averager's manual meta-gradient (averaging_logic.py:512-522).
    ``deltas``: [N, P] fp32 or a PackedDeltas, as in weighted_merge."""
    if _packed(deltas) and deltas.kind == "fp32":
        deltas = deltas.data
    N, P = deltas.shape
    S = offsets.numel() - 1
    if use_hip(g):
        if _packed(deltas):
            return require_ext().grad_merge_weights_packed(
                g, base, *_packed_args(deltas), merged, offsets.to(g.device))
        return require_ext().grad_merge_weights(g, base, deltas, merged,
                                                offsets.to(g.device))
    seg = _seg_ids(offsets, P)
    gw = torch.zeros(N, S, dtype=torch.float32)
    diff_base = base.float() - merged.float()
    gf = g.float()
    for i in range(N):
        di = deltas.row(i) if _packed(deltas) else deltas[i].float()
        contrib = gf * (diff_base + di)
        gw[i] = torch.zeros(S).index_add_(0, seg, contrib)
    return gw


def _seg_ids(offsets: torch.Tensor, P: int) -> torch.Tensor:
    seg = torch.zeros(P, dtype=torch.long)
    off = offsets.tolist()
    for j in range(len(off) - 1):
        seg[off[j]:off[j + 1]] = j
    return seg


def has_nan(flat: torch.Tensor) -> bool:
    """Reference: have_nans, averaging_logic.py:121-127."""
    if use_hip(flat):
        return bool(require_ext().has_nan(flat))
    return bool(torch.isnan(flat).any().item())


def l2norm(flat: torch.Tensor) -> float:
    """Norm of an fp32 plane as a host float (reference:
    training_manager.py:181-196). Syncs; the train step's clipping takes its
    norm with grad_sumsq_partials + step_control instead."""
    if use_hip(flat):
        return float(require_ext().l2norm_sq(flat)) ** 0.5
    return float(flat.float().pow(2).sum().item()) ** 0.5
