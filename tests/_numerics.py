"""fp64 references of the HIP kernels and the one error measure the accuracy
tests use (tests/test_numerics_selfcheck.py on the CPU,
tests/test_kernel_accuracy_gpu.py on the GPU). A plain helper module.

Every reference takes the EXACT bf16 (or fp32) input values as fp64 CPU
tensors and has two modes:

* ``exact``   -- fp64 throughout; the truth every error is measured against.
* ``rounded`` -- fp64 arithmetic, rounded to bf16 where the kernel rounds; the
  error of this result against ``exact`` is the floor no bf16 kernel can beat,
  and the kernel is held to a small multiple of it (``BF16_FACTOR``). For an
  fp32-output quantity ``rounded`` is the same formula evaluated in fp32 torch
  on the CPU, and the kernel is held to ``FP32_FACTOR`` times that error, never
  to less than ``FP32_ULPS`` fp32 ulp of the value.

Rounding points modelled in ``rounded`` (kernel file: where):

attention (hip/attention.hip)
  * P before P.V: attn_fwd_k packs exp2(s - m_run) * dropout into bf16
    (scores_to_afrag) with m_run the running max after the CURRENT 32-key
    tile; the rescale of the accumulator and the final 1/l stay fp32.
  * o: store_acc_tile rounds acc / l to bf16.
  * delta = rowsum(dO * o) reads the bf16 o (attn_bwd_dq_k prologue).
  * P in the backward is exp2(s - lse) with the fp32 lse of the forward.
  * dO.V (MFMA) and delta (fmaf chain) are two fp32 sums of D products in
    different orders, so their difference carries an fp32 error even where
    it is zero in exact arithmetic (one visible key: dq and dk are exactly
    zero). Modelled as one fp32 ulp of sum |dO||V| added to dO.V - delta;
    it matters in that degenerate case only.
  * dS before dS.K and dS^T.Q: scores_to_afrag in attn_bwd_dq_k / _dkv_k.
  * dropped P before P^T.dO (dv): scores_to_afrag in attn_bwd_dkv_k.
  * dq, dk, dv: one bf16 rounding each; with GQA dk/dv fold the q heads in
    fp32 (atomics) and round once after (bindings.cpp attn_bwd).
  * attn_bwd_fused_k runs the same arithmetic: same points.
decode attention (attn_decode_k): p and the accumulators stay fp32; only the
  output is rounded.
cross entropy (hip/ce.hip): dlogits = bf16(scale * (softmax - onehot)) is the
  only bf16 rounding (ce_row_grad); lse / loss_sum are fp32 quantities.
  loss_sum is an fp32 atomicAdd over rows: its fp32 baseline accumulates the
  rows serially in fp32. Each row's term is lse - target logit with lse
  ALREADY rounded to fp32 (ce_fwd_k, ``l - bf2f(xr[tgt])``): with logits
  near +-80 the term is 10 to 100 times smaller than the lse whose rounding
  it inherits, so the 4-ulp floor of loss_sum is taken from the lse values
  of the summed rows (``ulp_of``), as it is for head_loss_fwd.
norms (hip/norms.hip): the residual sum s = bf16(x + dropout(res)) is rounded
  BEFORE the statistics (norm_fwd_k, ``f2bf(f + rf)``); y, dx, dres are
  rounded once (dres from the unrounded dx: ``f2bf(g * inv_keep)``); dw/db are
  fp32 sums cast to the parameter dtype by ops._grad_out. The backward
  recomputes xhat from the rounded s.
GELU / SwiGLU (hip/elementwise.hip): the whole map is evaluated in fp32 and
  rounded once; ``rounded`` is therefore the formula in fp32 torch, then bf16
  (this models the fp32 cancellation in 1 + tanh(u), gelu_f, for x << 0).
RoPE (hip/rope.hip), embedding forward (hip/embedding.hip): fp32 arithmetic,
  outputs rounded once. Embedding dwte/dwpe are fp32 sums.
AdamW (hip/adamw.hip): master/m/v fp32; the working copy is bf16(master).
serving GEMV (hip/gemv.hip): fp32 fmaf accumulators over the whole K (the
  chunks of the x panel share them), fp32 wave and block fold, bias added in
  fp32, ONE bf16 rounding at the store (gemv_k, emit): ``rounded`` is
  bf16(exact).
weighted_merge (hip/merge.hip): fp32 throughout, base + d rounded, then an
  fmaf per model; the fp32 baseline is the CPU path of ops.weighted_merge.
grad_W (hip/merge.hip, grad_w_k): terms g * ((base - merged) + d) in fp32;
  lane t of 256 sums elements start + t, + 256, ... of a chunk of <= 2^20
  serially in fp32, the 256 partials and then the chunks of a segment are
  folded in fp32 (atomicAdd). The fp32 baseline (``lane_sum32``) sums in
  exactly that order: a serial sum of 2e5 terms costs 6e-6 to 8e-6 on its
  own and would hide the order of the two adds inside the term.
ce_chunk + ce_finalize (hip/ce.hip): the running (m, s) of a row is fp32 in
  exp2 units, rescaled once per tile; lse and loss_sum are the fp32
  quantities of ce_fwd and use its references; the target logit is the bf16
  input converted to fp32, exact.
kv_append, delta_sub: no rounding of their own (a copy; one fp32 subtract).
accum_f32_into_bf16: bf16(dst + src) with the sum in fp32, one rounding;
  ``rounded`` is bf16 of the fp64 sum.
"""

from __future__ import annotations

import json
import math
import os
from typing import Dict, Optional

import numpy as np
import torch

F64 = torch.float64
BF16_FACTOR = 3.0     # kernel <= 3 x rounded-reference error (bf16 outputs)
FP32_FACTOR = 16.0    # kernel <= 16 x fp32-torch error (fp32 outputs)
FP32_ULPS = 4.0       # ... and the bound is never below 4 fp32 ulp


def d(t: torch.Tensor) -> torch.Tensor:
    """Exact value of a bf16/fp32 tensor as an fp64 CPU tensor."""
    return t.detach().to("cpu").to(F64)


def bf16(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (nearest even), back in fp64."""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def f32(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(F64)


def _rnd(mode: str):
    assert mode in ("exact", "rounded"), mode
    return bf16 if mode == "rounded" else (lambda t: t)


# ---------------------------------------------------------------------------
# The measure
# ---------------------------------------------------------------------------
def errors(got: torch.Tensor, exact: torch.Tensor, row_dim=-1, live=None):
    """(rel_l2, worst_row) of ``got`` against ``exact``.

    rel_l2    = ||got - exact|| / ||exact|| over the tensor.
    worst_row = max_r ||e_r|| / max(||exact_r||, rms_r ||exact_r||): rows that
    are zero or nearly so in exact arithmetic are judged against the typical
    row. ``row_dim``: the dimension a row extends along; None makes every
    element its own row. ``live``: optional bool mask over the rows (shape of
    the tensor without ``row_dim``); rows outside it are outside the kernel's
    contract and are the only thing left out. A non-finite ``got`` is
    infinitely wrong. Where ``exact`` is identically zero both numbers are
    absolute errors.
    """
    g, e = d(got), d(exact)
    assert g.shape == e.shape, (g.shape, e.shape)
    if row_dim is None:
        g, e = g.reshape(-1, 1), e.reshape(-1, 1)
    else:
        g = g.movedim(row_dim, -1)
        e = e.movedim(row_dim, -1)
        g, e = g.reshape(-1, g.shape[-1]), e.reshape(-1, e.shape[-1])
    if live is not None:
        keep = live.reshape(-1).to(torch.bool)
        assert keep.numel() == g.shape[0], (keep.shape, g.shape)
        g, e = g[keep], e[keep]
    if not bool(torch.isfinite(g).all()):
        return float("inf"), float("inf")
    err = (g - e).norm(dim=-1)
    ref = e.norm(dim=-1)
    tot_err, tot_ref = float(err.norm()), float(ref.norm())
    if tot_ref == 0.0:
        # exact is identically zero (dq of a one-key softmax): no relative
        # error exists, both numbers are the absolute errors instead
        return tot_err, float(err.max())
    rms = tot_ref / math.sqrt(ref.numel())
    worst = float((err / torch.clamp(ref, min=rms)).max())
    return tot_err / tot_ref, worst


def _ulp32(e: torch.Tensor) -> torch.Tensor:
    """fp32 spacing at |e| (fp64 tensor)."""
    a = e.abs().to(torch.float32)
    tiny = torch.finfo(torch.float32).tiny
    a = torch.clamp(a, min=tiny)
    nxt = torch.nextafter(a, torch.full_like(a, float("inf")))
    return (nxt - a).to(F64)


def bounds(exact, rounded, row_dim=-1, live=None, fp32_out=False,
           ulp_of=None):
    """((base_l2, base_worst), (bound_l2, bound_worst)) for one tensor.
    ``ulp_of``: for an fp32 quantity that is a sum of differences of fp32
    values much larger than itself (loss_sum = sum of lse - target logit),
    those values: the floor is then 4 ulp of THEM, root-sum-squared, since
    each is rounded to fp32 before the difference is formed."""
    base = errors(rounded, exact, row_dim, live)
    if not fp32_out:
        return base, tuple(BF16_FACTOR * b for b in base)
    e = d(exact)
    if ulp_of is None:
        floor = errors(e + FP32_ULPS * _ulp32(e), e, row_dim, live)
    else:
        assert e.numel() == 1
        fl = float((FP32_ULPS * _ulp32(d(ulp_of))).norm())
        floor = errors(e + fl, e, row_dim, live)
    return base, tuple(max(FP32_FACTOR * b, f) for b, f in zip(base, floor))


# measured rows of the accuracy table (docs/test_accuracy.md); written out
# by the GPU test module when DTA_ACCURACY_REPORT names a file
REPORT = []


def check(op: str, case: str, tensor: str, got, exact, rounded, row_dim=-1,
          live=None, fp32_out=False, ulp_of=None):
    """Measure, record, print, then assert both bounds. Returns the row."""
    base, bound = bounds(exact, rounded, row_dim, live, fp32_out, ulp_of)
    kern = errors(got, exact, row_dim, live)
    row = dict(op=op, case=case, tensor=tensor, fp32=bool(fp32_out),
               base_l2=base[0], base_worst=base[1], kern_l2=kern[0],
               kern_worst=kern[1], bound_l2=bound[0], bound_worst=bound[1])
    REPORT.append(row)
    print(f"[acc] {op} {case} {tensor}: base {base[0]:.3e}/{base[1]:.3e} "
          f"kernel {kern[0]:.3e}/{kern[1]:.3e} "
          f"bound {bound[0]:.3e}/{bound[1]:.3e}")
    assert kern[0] <= bound[0], (
        f"{op} {case} {tensor}: rel_l2 {kern[0]:.3e} > bound {bound[0]:.3e} "
        f"(baseline {base[0]:.3e})")
    assert kern[1] <= bound[1], (
        f"{op} {case} {tensor}: worst_row {kern[1]:.3e} > bound "
        f"{bound[1]:.3e} (baseline {base[1]:.3e})")
    return row


def passes(got, exact, rounded, row_dim=-1, live=None, fp32_out=False,
           ulp_of=None):
    """True iff ``got`` is within both bounds (the self-check's predicate)."""
    _, bound = bounds(exact, rounded, row_dim, live, fp32_out, ulp_of)
    kern = errors(got, exact, row_dim, live)
    return kern[0] <= bound[0] and kern[1] <= bound[1]


def dump_report(path: Optional[str] = None) -> None:
    path = path or os.environ.get("DTA_ACCURACY_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f)


# ---------------------------------------------------------------------------
# Causal attention, forward + backward
# ---------------------------------------------------------------------------
def attention(q, k, v, do, scale, kvlen=None, keep=None, inv_keep=1.0,
              mode="exact", mut: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """q, do [B,H,S,D]; k, v [B,Hk,S,D] (fp64). kvlen: int tensor [B] or None.
    keep: bool [B,H,S,S] dropout keep-mask (ops.droprng.attn_keep_mask) or
    None; inv_keep its rescale. Returns o, lse, dq, dk, dv.

    ``mut`` (mutants, exact mode only): zero_prob=(b,h,q,k) zeroes one
    probability; dv_no_inv_keep drops the 1/keep factor in dv only; gqa_mod
    folds q head h onto kv head h % Hk instead of h // group.
    """
    mut = mut or {}
    rounded = mode == "rounded"
    rnd = _rnd(mode)
    assert not (mut and rounded)
    B, H, S, D = q.shape
    Hk = k.shape[1]
    grp = H // Hk
    head = torch.arange(H) % Hk if mut.get("gqa_mod") else torch.arange(H) // grp
    ke, ve = k[:, head], v[:, head]
    s = torch.einsum("bhqd,bhkd->bhqk", q, ke) * scale
    idx = torch.arange(S)
    vis = (idx[None, :] <= idx[:, None])[None, None]
    if kvlen is not None:
        vis = vis & (idx[None, None, None, :]
                     < kvlen.to(torch.long).view(B, 1, 1, 1))
    s = s.masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    A = e / l
    if "zero_prob" in mut:
        A = A.clone()
        A[mut["zero_prob"]] = 0.0
    lse = (m + torch.log(l)).squeeze(-1)
    drop = (keep.to(F64) * inv_keep if keep is not None
            else torch.ones_like(A))

    if rounded:
        # running max after each 32-key tile, spread back over the keys
        nt = (S + 31) // 32
        sp = torch.nn.functional.pad(s, (0, nt * 32 - S), value=float("-inf"))
        mt = sp.view(B, H, S, nt, 32).amax(-1).cummax(-1).values
        mt = mt.repeat_interleave(32, dim=-1)[..., :S]
        pt = bf16(torch.exp(s - mt) * drop)
        o = torch.einsum("bhqk,bhkd->bhqd", pt * torch.exp(mt - m), ve) / l
        o = bf16(o)
        lse_b = f32(lse)
        P = torch.exp(s - lse_b.unsqueeze(-1))
    else:
        o = torch.einsum("bhqk,bhkd->bhqd", A * drop, ve)
        P = A

    dp = torch.einsum("bhqd,bhkd->bhqk", do, ve)
    delta = (do * o).sum(-1, keepdim=True)
    resid = 0.0
    if rounded:
        resid = _ulp32(torch.einsum("bhqd,bhkd->bhqk", do.abs(), ve.abs()))
    dS = rnd(P * (dp * drop - delta + resid))
    dq = rnd(torch.einsum("bhqk,bhkd->bhqd", dS, ke) * scale)
    drop_v = drop
    if mut.get("dv_no_inv_keep") and keep is not None:
        drop_v = keep.to(F64)
    dk_h = torch.einsum("bhqk,bhqd->bhkd", dS, q) * scale
    dv_h = torch.einsum("bhqk,bhqd->bhkd", rnd(P * drop_v), do)
    dk = torch.zeros(B, Hk, S, D, dtype=F64).index_add_(1, head, dk_h)
    dv = torch.zeros(B, Hk, S, D, dtype=F64).index_add_(1, head, dv_h)
    return dict(o=o, lse=f32(lse) if rounded else lse, dq=dq, dk=rnd(dk),
                dv=rnd(dv))


def decode_attention(q, kc, vc, L, scale, mode="exact"):
    """q [B,H,D]; caches [B,Hk,Lmax,D]; the first L cache rows are valid."""
    B, H, D = q.shape
    Hk = kc.shape[1]
    head = torch.arange(H) // (H // Hk)
    ke, ve = kc[:, head, :L], vc[:, head, :L]
    s = torch.einsum("bhd,bhkd->bhk", q, ke) * scale
    A = torch.softmax(s, dim=-1)
    return _rnd(mode)(torch.einsum("bhk,bhkd->bhd", A, ve))


# ---------------------------------------------------------------------------
# Cross entropy
# ---------------------------------------------------------------------------
def _serial_sum32(t32: torch.Tensor) -> torch.Tensor:
    """fp32 sum accumulated one term at a time (what an atomicAdd chain does,
    in some order). numpy keeps the running sum in fp32; torch.cumsum on the
    CPU accumulates fp32 data in double."""
    if t32.numel() == 0:
        return torch.zeros((), dtype=torch.float32)
    a = t32.reshape(-1).numpy().astype(np.float32)
    return torch.tensor(np.cumsum(a, dtype=np.float32)[-1],
                        dtype=torch.float32)


def cross_entropy(logits, targets, ignore_index, scale, mode="exact",
                  mut: Optional[dict] = None):
    """logits [T,V] fp64, targets int64 [T], scale the fp32 value the kernel
    multiplies (softmax - onehot) with. Returns lse [T], loss_sum, count,
    dlogits [T,V]. Mutants: grad_mul, lse_add, grad_ignored, count_all."""
    mut = mut or {}
    valid = targets != ignore_index
    tg = targets.clamp(min=0)
    count = int(valid.sum())
    if mode == "rounded":
        x32 = logits.to(torch.float32)
        lse32 = torch.logsumexp(x32, dim=-1)
        per = (lse32 - x32.gather(1, tg[:, None])[:, 0])[valid]
        loss_sum = _serial_sum32(per).to(F64)
        lse = lse32.to(F64)
        lse_x = torch.logsumexp(logits, dim=-1)
    else:
        lse = torch.logsumexp(logits, dim=-1) + mut.get("lse_add", 0.0)
        loss_sum = (lse - logits.gather(1, tg[:, None])[:, 0])[valid].sum()
        lse_x = lse
    p = torch.exp(logits - lse_x[:, None])
    onehot = torch.zeros_like(p).scatter_(1, tg[:, None], 1.0)
    sc = scale
    if mut.get("count_all"):
        sc = scale * max(count, 1) / targets.numel()
    rowsc = valid.to(F64) * sc
    if mut.get("grad_ignored"):
        rowsc = torch.full_like(rowsc, sc)
    dl = rowsc[:, None] * (p - onehot) * mut.get("grad_mul", 1.0)
    return dict(lse=lse, loss_sum=loss_sum, count=count,
                dlogits=_rnd(mode)(dl))


def head_loss(x, w, targets, ignore_index, mode="exact"):
    """lse [T] and loss_sum of x @ w^T without rounding the logits (the
    kernel folds fp32 accumulator tiles straight into the lse)."""
    valid = targets != ignore_index
    tg = targets.clamp(min=0)
    if mode == "rounded":
        lg = x.to(torch.float32) @ w.to(torch.float32).t()
        lse = torch.logsumexp(lg, dim=-1)
        per = (lse - lg.gather(1, tg[:, None])[:, 0])[valid]
        return dict(lse=lse.to(F64), loss_sum=_serial_sum32(per).to(F64),
                    count=int(valid.sum()))
    lg = x @ w.t()
    lse = torch.logsumexp(lg, dim=-1)
    return dict(lse=lse,
                loss_sum=(lse - lg.gather(1, tg[:, None])[:, 0])[valid].sum(),
                count=int(valid.sum()))


# ---------------------------------------------------------------------------
# LayerNorm / RMSNorm, optional fused residual add (+ dropout on the branch)
# ---------------------------------------------------------------------------
def norm(x, w, b, eps, dy, res=None, ds=None, keep=None, inv_keep=1.0,
         mode="exact", mut: Optional[dict] = None):
    """x, dy [R,C]; w [C]; b [C] or None (RMSNorm). res: branch added to x
    (fused residual), keep: bool [R,C] dropout keep-mask on it. ds: gradient
    arriving on the sum. Returns y, s, dx, dres, dw, db.
    Mutants: no_mean_term (dx without the projection on the mean, for RMS
    without the projection on xhat), dw_skip_last_row, no_eps."""
    mut = mut or {}
    rnd = _rnd(mode)
    rms = b is None
    s = x
    if res is not None:
        r = res if keep is None else res * keep.to(F64) * inv_keep
        s = rnd(x + r)
    mu = torch.zeros_like(s[:, :1]) if rms else s.mean(-1, keepdim=True)
    var = ((s - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + (0.0 if mut.get("no_eps") else eps))
    xh = (s - mu) * rstd
    y = xh * w
    if not rms:
        y = y + b
    dyw = dy * w
    c1 = dyw.mean(-1, keepdim=True)
    c2 = (dyw * xh).mean(-1, keepdim=True)
    if rms:
        g = rstd * (dyw if mut.get("no_mean_term") else dyw - xh * c2)
    else:
        g = rstd * (dyw - (0.0 if mut.get("no_mean_term") else c1) - xh * c2)
    if ds is not None:
        g = g + ds
    dres = None
    if res is not None:
        dres = g if keep is None else g * keep.to(F64) * inv_keep
        dres = rnd(dres)
    rows = slice(None, -1) if mut.get("dw_skip_last_row") else slice(None)
    dw = (dy * xh)[rows].sum(0)
    db = None if rms else dy[rows].sum(0)
    return dict(y=rnd(y), s=s, dx=rnd(g), dres=dres, dw=rnd(dw),
                db=None if db is None else rnd(db))


# ---------------------------------------------------------------------------
# GELU (tanh form) / SwiGLU
# ---------------------------------------------------------------------------
_GELU_C = math.sqrt(2.0 / math.pi)
_GELU_A = 0.044715


def _gelu_parts(x):
    u = _GELU_C * (x + _GELU_A * x * x * x)
    t = torch.tanh(u)
    y = 0.5 * x * (1.0 + t)
    dy = 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * _GELU_C * (
        1.0 + 3.0 * _GELU_A * x * x)
    return y, dy


def gelu(x, dy, mode="exact", mut: Optional[dict] = None):
    """Returns y, dx. Mutant: erf (the erf form where the tanh form belongs)."""
    mut = mut or {}
    if mut.get("erf"):
        phi = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
        pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        return dict(y=x * phi, dx=dy * (phi + x * pdf))
    if mode == "rounded":
        y, g = _gelu_parts(x.to(torch.float32))
        return dict(y=bf16(y), dx=bf16(dy.to(torch.float32) * g))
    y, g = _gelu_parts(x)
    return dict(y=y, dx=dy * g)


def swiglu(gate, up, dy, mode="exact"):
    """Returns y, dgate, dup."""
    if mode == "rounded":
        gate, up, dy = (t.to(torch.float32) for t in (gate, up, dy))
    sg = torch.sigmoid(gate)
    silu = gate * sg
    dsilu = sg * (1.0 + gate * (1.0 - sg))
    out = dict(y=silu * up, dgate=dy * up * dsilu, dup=dy * silu)
    if mode == "rounded":
        out = {k_: bf16(v_) for k_, v_ in out.items()}
    return out


# ---------------------------------------------------------------------------
# RoPE (half-split convention), embedding, AdamW
# ---------------------------------------------------------------------------
def rope(x, cos, sin, pos=0, backward=False, mode="exact",
         mut: Optional[dict] = None):
    """x [...,S,D]; cos/sin [rows,D/2] tables; row of position s is pos + s.
    backward: the explicit inverse rotation. Mutants: bwd_fwd_sign (backward
    with the forward's sign), row_off (table row off by this much)."""
    mut = mut or {}
    S, D = x.shape[-2], x.shape[-1]
    d2 = D // 2
    p0 = pos + mut.get("row_off", 0)
    c, sn = cos[p0:p0 + S], sin[p0:p0 + S]
    if backward and not mut.get("bwd_fwd_sign"):
        sn = -sn
    x1, x2 = x[..., :d2], x[..., d2:]
    return _rnd(mode)(torch.cat([x1 * c - x2 * sn, x1 * sn + x2 * c], dim=-1))


def embedding(ids, wte, wpe, dy, pos=0, mode="exact"):
    """ids [B,S]; returns y [B,S,E], dwte [V,E], dwpe [P,E] (fp32-output
    sums; the backward has no position offset)."""
    B, S = ids.shape
    y = wte[ids]
    if wpe is not None:
        y = y + wpe[pos:pos + S][None]
    if mode == "rounded":
        dy32 = dy.to(torch.float32)
        dwte = torch.zeros(wte.shape, dtype=torch.float32).index_add_(
            0, ids.reshape(-1), dy32.reshape(-1, dy.shape[-1])).to(F64)
        dwpe = None
        if wpe is not None:
            dwpe = torch.zeros(wpe.shape, dtype=torch.float32)
            dwpe[:S] = dy32.sum(0)
            dwpe = dwpe.to(F64)
        return dict(y=bf16(y), dwte=dwte, dwpe=dwpe)
    dwte = torch.zeros_like(wte).index_add_(0, ids.reshape(-1),
                                            dy.reshape(-1, dy.shape[-1]))
    dwpe = None
    if wpe is not None:
        dwpe = torch.zeros_like(wpe)
        dwpe[:S] = dy.sum(0)
    return dict(y=y, dwte=dwte, dwpe=dwpe)


def adamw(master, grads, lr, beta1, beta2, eps, wd, mode="exact",
          mut: Optional[dict] = None):
    """Decoupled AdamW from zero moments over len(grads) steps. master fp64
    (fp32 values), grads: list of fp64 tensors holding the bf16 gradient
    values the kernel reads. Returns master, m, v, work (bf16 copy).
    Mutants: bc_prev_step (bias correction of step t-1, from step 2 on),
    coupled (weight decay added to the gradient)."""
    mut = mut or {}
    dt = torch.float32 if mode == "rounded" else F64
    w = master.to(dt).clone()
    m = torch.zeros_like(w)
    v = torch.zeros_like(w)
    for t, g in enumerate(grads, start=1):
        g = g.to(dt)
        tb = max(t - 1, 1) if mut.get("bc_prev_step") else t
        bc1, bc2 = 1.0 - beta1 ** tb, 1.0 - beta2 ** tb
        if mut.get("coupled"):
            g = g + wd * w
        else:
            w = w * (1.0 - lr * wd)
        m = beta1 * m + (1.0 - beta1) * g
        v = beta2 * v + (1.0 - beta2) * g * g
        w = w - (lr / bc1) * m / (torch.sqrt(v / bc2) + eps)
    return dict(master=w.to(F64), m=m.to(F64), v=v.to(F64),
                work=bf16(w.to(F64)) if mode == "rounded" else w.to(F64))


def l2norm_sq(x, mode="exact"):
    """x fp64 (fp32 values). fp32 baseline: 1024-element partials, then a
    serial fp32 accumulation (the kernel's block sums + atomicAdd chain)."""
    if mode == "exact":
        return (x * x).sum()
    sq = x.to(torch.float32) ** 2
    n = sq.numel()
    pad = (-n) % 1024
    part = torch.nn.functional.pad(sq, (0, pad)).view(-1, 1024).sum(1)
    return _serial_sum32(part).to(F64)


def colsum(x, mode="exact"):
    if mode == "exact":
        return x.sum(0)
    return x.to(torch.float32).sum(0).to(F64)


def axpy(w, x, alpha, mode="exact"):
    if mode == "exact":
        return w + float(np.float32(alpha)) * x
    return (w.to(torch.float32) + float(np.float32(alpha))
            * x.to(torch.float32)).to(F64)


# ---------------------------------------------------------------------------
# Shared input builders (the self-check and the GPU tests draw the SAME
# inputs, so a regime in which a mutant hides shows up on the CPU)
# ---------------------------------------------------------------------------
def randn_bf16(*shape, seed=0, scale=1.0) -> torch.Tensor:
    """CPU bf16 tensor, the generator convention of tests/test_ops_gpu.py."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


ATTN_REGIMES = ("diffuse", "peaked", "rising", "large")


def attn_inputs(B, H, Hk, S, D, regime, seed=100):
    """q [B,H,S,D], k, v [B,Hk,S,D], do [B,H,S,D] as CPU bf16.
    diffuse: randn. peaked: q x 4. rising: the keys of the last 16 positions
    x 4, so the row max moves in the final key tile (online rescale).
    large: q and k x 8, scores reach tens (exp2 range)."""
    q = randn_bf16(B, H, S, D, seed=seed).float()
    k = randn_bf16(B, Hk, S, D, seed=seed + 1).float()
    v = randn_bf16(B, Hk, S, D, seed=seed + 2)
    do = randn_bf16(B, H, S, D, seed=seed + 3)
    if regime == "peaked":
        q = q * 4
    elif regime == "rising":
        k[:, :, max(S - 16, 0):] *= 4
    elif regime == "large":
        q, k = q * 8, k * 8
    else:
        assert regime == "diffuse", regime
    return q.to(torch.bfloat16), k.to(torch.bfloat16), v, do


def live_rows(kvlen, B, S):
    """bool [B,S]: query rows inside the contract (row < kvlen[b])."""
    if kvlen is None:
        return torch.ones(B, S, dtype=torch.bool)
    return torch.arange(S)[None, :] < kvlen.to(torch.long)[:, None]


CE_REGIMES = {"randn3": 0.0, "plus80": 80.0, "minus80": -80.0}


def ce_inputs(rows, vocab, regime, seed=200):
    """logits (CPU bf16) and targets. randn x 3 shifted by the regime; rows
    0, 4, 8, ... ignored; row 1 has its target logit 30 above the rest of
    the row, row 2 has all-equal logits."""
    x = randn_bf16(rows, vocab, seed=seed, scale=3.0).float() \
        + CE_REGIMES[regime]
    g = torch.Generator().manual_seed(seed + 1)
    tg = torch.randint(0, vocab, (rows,), generator=g)
    x = x.to(torch.bfloat16).float()
    x[1, tg[1]] = x[1].max() + 30.0
    x[2] = x[2, 0]
    tg[::4] = -100
    return x.to(torch.bfloat16), tg


NORM_REGIMES = ("randn", "offset100", "lowvar")


def norm_inputs(rows, cols, regime, seed=300):
    """x, res, w, b, dy, ds as CPU bf16. offset100: x = 100 + 0.5 randn (one
    bf16 step at 100: the smallest noise the format holds there), the
    cancellation probe for a one-pass variance. lowvar: row 0 is 1 with one
    entry in ten a bf16 step higher, so its variance is of the size of eps;
    row 1 is 2^-9 randn, so its mean square is too (the RMSNorm probe). dy
    of those two rows is scaled by 2^-8 (their rstd is ~260), or their dx
    would be the whole norm of the tensor and hide every other row."""
    x = randn_bf16(rows, cols, seed=seed).float()
    if regime == "offset100":
        x = 100.0 + 0.5 * x
    elif regime == "lowvar":
        g = torch.Generator().manual_seed(seed + 9)
        x[0] = 1.0 + (torch.rand(cols, generator=g) < 0.1).float() * 2.0 ** -7
        x[1] = x[1] * 2.0 ** -9
    else:
        assert regime == "randn", regime
    dy = randn_bf16(rows, cols, seed=seed + 4)
    if regime == "lowvar":
        dy[:2] = (dy[:2].float() * 2.0 ** -8).to(torch.bfloat16)
    return dict(x=x.to(torch.bfloat16),
                res=randn_bf16(rows, cols, seed=seed + 1, scale=0.25),
                w=randn_bf16(cols, seed=seed + 2, scale=0.5),
                b=randn_bf16(cols, seed=seed + 3, scale=0.5),
                dy=dy,
                ds=randn_bf16(rows, cols, seed=seed + 5))


EW_FIXED = (0.0, 1e-3, -1e-3, 8.0, -8.0, 30.0, -30.0, 1e4, -1e4)
# the fixed values are measured in groups of one magnitude: in one vector
# the 1e4 entries would be the whole norm
EW_FIXED_GROUPS = (slice(0, 3), slice(3, 7), slice(7, 9))


def ew_inputs(n, regime="randn2", seed=400):
    """x, up, dy (CPU bf16, length n). randn2: randn x 2, and for n >= 64
    the last 9 entries are EW_FIXED. tail: x in [-4, -2.5], where GELU is
    small and the erf and tanh forms differ by 3% and more."""
    x = randn_bf16(n, seed=seed, scale=2.0).float()
    if regime == "tail":
        g = torch.Generator().manual_seed(seed + 9)
        x = -2.5 - 1.5 * torch.rand(n, generator=g)
    elif n >= 64:
        x[-len(EW_FIXED):] = torch.tensor(EW_FIXED)
    return (x.to(torch.bfloat16), randn_bf16(n, seed=seed + 1),
            randn_bf16(n, seed=seed + 2))


def rope_tables(rows, D, theta=10000.0):
    """cos, sin [rows, D/2] fp32 (the models' table formula)."""
    inv = 1.0 / (theta ** (torch.arange(0, D // 2, dtype=torch.float64)
                           / (D // 2)))
    ang = torch.arange(rows, dtype=torch.float64)[:, None] * inv[None]
    return ang.cos().float(), ang.sin().float()


# ---------------------------------------------------------------------------
# The cases. Both test modules iterate these lists; a case builds its inputs
# and both references once (cached) and is never modified afterwards.
# ---------------------------------------------------------------------------
import functools  # noqa: E402

DROP_CTR, DROP_SITE = 42, 7

# (B, H, Hkv, S, D). Fused backward (one 64-row tile, no GQA, D <= 64):
# the first two; two-kernel path with a ragged last block: the next two;
# GQA; one row; one partly filled wave.
ATTN_SHAPES = [(2, 2, 2, 64, 64), (1, 2, 2, 48, 32), (1, 2, 2, 70, 32),
               (1, 2, 2, 130, 128), (1, 4, 2, 96, 64), (1, 1, 1, 1, 64),
               (1, 1, 1, 17, 64)]
ATTN_FUSED_SHAPES = [(2, 2, 2, 64, 64), (1, 2, 2, 48, 32)]


def attn_fused_expected(shape) -> bool:
    """dta_attn_bwd_fused_shape: one tile, no GQA fold, head dim 32 or 64."""
    _B, H, Hk, S, D = shape
    return S <= 64 and H == Hk and D in (32, 64)


# (shape, regime, kvlen or None, p)
ATTN_PLAIN = [(s, r, None, 0.0) for s in ATTN_SHAPES for r in ATTN_REGIMES]
# kvlen values from {1, 16, 17, 64, 65, S}; at least half the query rows of
# every case are live (65 at S = 64 is clamped to S by the kernels)
ATTN_KVLEN = [(s, r, kv, 0.0)
              for s, kv in [((4, 2, 2, 64, 64), (64, 17, 16, 65)),
                            ((4, 2, 2, 64, 64), (64, 1, 64, 64)),
                            ((4, 2, 2, 130, 64), (130, 65, 64, 130)),
                            ((4, 2, 2, 130, 128), (130, 17, 130, 1)),
                            ((4, 2, 2, 130, 64), (16, 130, 130, 130))]
              for r in ("diffuse", "rising")]
ATTN_DROP = [(s, r, kv, p)
             for s, kv, p in [((2, 2, 2, 64, 64), None, 0.1),
                              ((2, 2, 2, 64, 64), (64, 17), 0.25),
                              ((1, 2, 2, 70, 32), None, 0.25),
                              ((2, 2, 2, 130, 64), (130, 65), 0.1),
                              ((1, 4, 2, 96, 64), None, 0.1),
                              ((2, 4, 2, 96, 64), (96, 64), 0.25)]
             for r in ("diffuse", "peaked")]
ATTN_CASES = ATTN_PLAIN + ATTN_KVLEN + ATTN_DROP
ATTN_TENSORS = ("o", "dq", "dk", "dv")


def case_id(case) -> str:
    shape, regime, kv, p = case
    s = "x".join(map(str, shape)) + "-" + regime
    if kv is not None:
        s += "-kv" + "_".join(map(str, kv))
    if p:
        s += f"-p{p}"
    return s


def attn_mask(case):
    """(keep bool [B,H,S,S] or None, inv_keep) from the host-gold chain."""
    from distributedtraining_amd.ops import droprng
    (B, H, _Hk, S, _D), _r, _kv, p = case
    if not p:
        return None, 1.0
    keep = droprng.attn_keep_mask(B * H, S, S, DROP_CTR, DROP_SITE, p)
    return (torch.from_numpy(keep).view(B, H, S, S),
            float(np.float32(droprng.inv_keep(p))))


@functools.lru_cache(maxsize=None)
def attn_case(case):
    """inputs (CPU bf16; dO zero on rows outside the contract), kvlen, keep,
    live [B,H,S] and both references."""
    (B, H, Hk, S, D), regime, kv, p = case
    q, k, v, do = attn_inputs(B, H, Hk, S, D, regime)
    kvlen = None if kv is None else torch.tensor(kv, dtype=torch.int32)
    live = live_rows(None if kvlen is None else kvlen.clamp(max=S), B, S)
    do = (do.float() * live[:, None, :, None]).to(torch.bfloat16)
    keep, inv_keep = attn_mask(case)
    scale = 1.0 / math.sqrt(D)
    args = (d(q), d(k), d(v), d(do), scale, kvlen, keep, inv_keep)
    return dict(q=q, k=k, v=v, do=do, kvlen=kvlen, keep=keep,
                inv_keep=inv_keep, scale=scale, args=args,
                live=live[:, None, :].expand(B, H, S),
                exact=attention(*args, mode="exact"),
                rounded=attention(*args, mode="rounded"))


def attn_live(c, name):
    """Rows of tensor ``name`` inside the contract: query rows below kvlen
    for o and dq; every key row for dk and dv."""
    return c["live"] if name in ("o", "dq") else None


# decode: (B, H, Hkv, L, D, regime); the cache is 7 rows longer than L
DECODE_CASES = [(2, 4, 4, L, D, r) for L in (1, 63, 64, 65, 257)
                for D in (64, 128) for r in ("diffuse", "rising")] \
    + [(2, 8, 2, 257, 64, "diffuse"), (2, 8, 2, 65, 128, "rising")]


@functools.lru_cache(maxsize=None)
def decode_case(case):
    B, H, Hk, L, D, regime = case
    q = randn_bf16(B, H, D, seed=500)
    kc = randn_bf16(B, Hk, L + 7, D, seed=501).float()
    vc = randn_bf16(B, Hk, L + 7, D, seed=502)
    if regime == "rising":
        kc[:, :, max(L - 16, 0):L] *= 4
    kc = kc.to(torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    args = (d(q), d(kc), d(vc), L, scale)
    return dict(q=q, kc=kc, vc=vc, scale=scale,
                exact=decode_attention(*args, mode="exact"),
                rounded=decode_attention(*args, mode="rounded"))


CE_SHAPES = [(8, 50257), (33, 1000), (5, 7), (16, 520)]
CE_CASES = [(r, v, g) for r, v in CE_SHAPES for g in CE_REGIMES]


@functools.lru_cache(maxsize=None)
def ce_case(case):
    rows, vocab, regime = case
    x, tg = ce_inputs(rows, vocab, regime)
    n_valid = int((tg != -100).sum())
    scale = float(np.float32(1.0) / np.float32(max(n_valid, 1)))
    args = (d(x), tg, -100, scale)
    return dict(x=x, tg=tg, scale=scale, n_valid=n_valid, args=args,
                exact=cross_entropy(*args, mode="exact"),
                rounded=cross_entropy(*args, mode="rounded"))


def ce_valid_lse(c):
    """The lse values loss_sum is made of (``ulp_of`` of its check)."""
    return c["exact"]["lse"][c["tg"] != -100]


def ce_target_entries(dlogits, tg):
    """The target-column entries of the non-ignored rows, as a vector."""
    valid = tg != -100
    return d(dlogits)[valid].gather(1, tg[valid][:, None])[:, 0]


NORM_SHAPES = [(33, 8), (33, 520), (5, 768), (33, 4096)]
NORM_DROP = (0.2, 9, 31)    # p, site, counter of the residual-dropout case
# (rows, cols, kind, regime, form); form: plain | residual | dropout
NORM_CASES = [(r, c, kind, regime, form) for r, c in NORM_SHAPES
              for kind in ("layer", "rms") for regime in NORM_REGIMES
              for form in ("plain", "residual")] \
    + [(33, 520, "layer", "randn", "dropout"),
       (33, 520, "rms", "randn", "dropout")]
NORM_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def norm_case(case):
    from distributedtraining_amd.ops import droprng
    rows, cols, kind, regime, form = case
    t = norm_inputs(rows, cols, regime)
    keep, inv_keep = None, 1.0
    if form == "dropout":
        p, site, ctr = NORM_DROP
        keep = torch.from_numpy(
            droprng.elem_keep_mask(rows * cols, ctr, site, p)).view(rows, cols)
        inv_keep = float(np.float32(droprng.inv_keep(p)))
    kw = dict(x=d(t["x"]), w=d(t["w"]),
              b=d(t["b"]) if kind == "layer" else None, eps=NORM_EPS,
              dy=d(t["dy"]))
    if form != "plain":
        kw.update(res=d(t["res"]), ds=d(t["ds"]), keep=keep,
                  inv_keep=inv_keep)
    return dict(t=t, kw=kw, keep=keep, exact=norm(**kw, mode="exact"),
                rounded=norm(**kw, mode="rounded"))


def norm_tensors(case):
    """(name, row_dim) of the tensors a norm case asserts."""
    _r, _c, kind, _g, form = case
    names = [("y", -1), ("dx", -1), ("dw", None)]
    if kind == "layer":
        names.append(("db", None))
    if form != "plain":
        names += [("s", -1), ("dres", -1)]
    return names


# elementwise lengths: scalar tails, one vector, several blocks; EW_LOOP_N
# makes the capped grid (MAX_RESIDENT_BLOCKS blocks of 256 threads, 16
# elements per thread and iteration in the GELU map) go round a second time
EW_NS = [1, 15, 17, 1000, 4099]
EW_CASES = [(n, "randn2") for n in EW_NS] + [(4099, "tail")]


def ew_loop_n(max_resident_blocks: int) -> int:
    return max_resident_blocks * 256 * 16 + 4099


@functools.lru_cache(maxsize=None)
def ew_case(case):
    n, regime = case
    x, up, dy = ew_inputs(n, regime)
    return dict(x=x, up=up, dy=dy,
                gelu_exact=gelu(d(x), d(dy)),
                gelu_rounded=gelu(d(x), d(dy), mode="rounded"),
                swiglu_exact=swiglu(d(x), d(up), d(dy)),
                swiglu_rounded=swiglu(d(x), d(up), d(dy), mode="rounded"))


def ew_parts(case):
    """(label, slice) pieces an elementwise tensor is measured in."""
    n, regime = case
    if regime == "randn2" and n >= 64:
        nf = len(EW_FIXED)
        return [("body", slice(0, n - nf))] + [
            (f"fixed{i}", slice(n - nf + g.start, n - nf + g.stop))
            for i, g in enumerate(EW_FIXED_GROUPS)]
    return [("body", slice(0, n))]


# RoPE: (BH, S, D, pos). 4096 blocks of 4 row-waves cover 16384 rows: the
# (260, 64, 64) case has 16640 and loops once. D = 6: odd half-dim tail;
# D = 512: second lane iteration.
ROPE_CASES = [(4, 32, 64, 0), (260, 64, 64, 0), (3, 5, 6, 0), (2, 7, 512, 0),
              (4, 1, 64, 37), (3, 5, 6, 3)]


@functools.lru_cache(maxsize=None)
def rope_case(case):
    bh, S, D, pos = case
    x = randn_bf16(bh, S, D, seed=600)
    cos, sin = rope_tables(pos + S + 2, D)
    out = dict(x=x, cos=cos, sin=sin)
    for name, bwd in (("fwd", False), ("bwd", True)):
        for mode in ("exact", "rounded"):
            out[f"{name}_{mode}"] = rope(d(x), d(cos), d(sin), pos, bwd, mode)
    return out


# embedding: (V, P, E, B, S, ids, pos)
EMB_CASES = [(64, 48, 64, 4, 32, "same", 0), (512, 48, 64, 4, 32, "random", 0),
             (512, 48, 72, 3, 1, "random", 11), (64, 48, 64, 2, 8, "same", 5)]


@functools.lru_cache(maxsize=None)
def emb_case(case):
    V, P, E, B, S, kind, pos = case
    wte = randn_bf16(V, E, seed=700)
    wpe = randn_bf16(P, E, seed=701)
    dy = randn_bf16(B, S, E, seed=702)
    if kind == "same":
        ids = torch.full((B, S), 3, dtype=torch.int64)
    else:
        ids = torch.randint(0, V, (B, S),
                            generator=torch.Generator().manual_seed(703))
    a = (ids, d(wte), d(wpe), d(dy), pos)
    return dict(wte=wte, wpe=wpe, dy=dy, ids=ids,
                exact=embedding(*a, mode="exact"),
                rounded=embedding(*a, mode="rounded"))


ADAMW_HP = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.05)
ADAMW_N = 4099      # odd tail on purpose


@functools.lru_cache(maxsize=None)
def adamw_case():
    g0 = torch.Generator().manual_seed(21)
    master = torch.randn(ADAMW_N, generator=g0)
    grads = [torch.randn(ADAMW_N, generator=g0).to(torch.bfloat16)
             for _ in range(3)]
    a = (d(master), [d(g) for g in grads])
    return dict(master=master, grads=grads,
                exact=adamw(*a, **ADAMW_HP, mode="exact"),
                rounded=adamw(*a, **ADAMW_HP, mode="rounded"))


ADAMW_TENSORS = (("master", True), ("m", True), ("v", True), ("work", False))


def attention_probs(q, k, scale, kvlen=None):
    """Exact softmax probabilities [B,H,S,S] (what a mutant perturbs)."""
    B, H, S, _ = q.shape
    head = torch.arange(H) // (H // k.shape[1])
    s = torch.einsum("bhqd,bhkd->bhqk", q, k[:, head]) * scale
    idx = torch.arange(S)
    vis = (idx[None, :] <= idx[:, None])[None, None]
    if kvlen is not None:
        vis = vis & (idx[None, None, None, :]
                     < kvlen.to(torch.long).view(B, 1, 1, 1))
    return torch.softmax(s.masked_fill(~vis, float("-inf")), dim=-1)


HEAD_LOSS_SHAPE = (17, 64, 517)     # T, K, V: ragged row block and vocab tile


@functools.lru_cache(maxsize=None)
def head_loss_case():
    T, K, V = HEAD_LOSS_SHAPE
    x = randn_bf16(T, K, seed=800, scale=0.5)
    w = randn_bf16(V, K, seed=801, scale=0.5)
    tg = torch.randint(0, V, (T,), generator=torch.Generator().manual_seed(802))
    tg[::5] = -100
    a = (d(x), d(w), tg, -100)
    return dict(x=x, w=w, tg=tg, exact=head_loss(*a, mode="exact"),
                rounded=head_loss(*a, mode="rounded"))


# ---------------------------------------------------------------------------
# Serving GEMV
# ---------------------------------------------------------------------------
def gemv_kc(M: int) -> int:
    """K chunk of the staged x panel: 8192 / MT, MT = 1, 2 or 4 rows."""
    return 8192 // (1 if M == 1 else 2 if M == 2 else 4)


def gemv(x, w, bias, mode="exact", mut: Optional[dict] = None):
    """x [M,K], w [N,K], bias [N] or None (fp64). y [M,N] = x w^T + bias.
    Mutants: drop_last_chunk (the last K chunk of gemv_kc(M) elements),
    drop_last8, no_bias, bf16_between_chunks (the accumulator rounded to bf16
    at every chunk boundary), row_shift (row m reads x row m - 1),
    skip_last_col (column N - 1 left at zero)."""
    mut = mut or {}
    M, K = x.shape
    kc = gemv_kc(M)
    xs = x.roll(1, 0) if mut.get("row_shift") else x
    hi = K
    if mut.get("drop_last_chunk"):
        hi = ((K - 1) // kc) * kc
    if mut.get("drop_last8"):
        hi = K - 8
    if mut.get("bf16_between_chunks"):
        acc = torch.zeros(M, w.shape[0], dtype=F64)
        for k0 in range(0, K, kc):
            if k0:
                acc = bf16(acc)
            acc = acc + xs[:, k0:k0 + kc] @ w[:, k0:k0 + kc].t()
    else:
        acc = xs[:, :hi] @ w[:, :hi].t()
    if bias is not None and not mut.get("no_bias"):
        acc = acc + bias
    if mut.get("skip_last_col"):
        acc = acc.clone()
        acc[:, -1] = 0.0
    return _rnd(mode)(acc)


def gemv_inputs(M, N, K, bias, regime, seed=900):
    """x [M,K], w [N,K], bias [N] or None as CPU bf16. randn: x = 0.5 randn,
    w = 0.05 randn. cancel: row m of x is (1 + m/4) x0 and w[n] = a_n s_k x0,
    s_k = +1 on the first half of K and -0.98 S+/S- on the second, so the two
    halves of every dot product are 50 x the result with opposite signs.
    bias: none | bf16 (randn, as the serving models') | x100 (100 x the rms
    of the product)."""
    x = randn_bf16(M, K, seed=seed, scale=0.5)
    w = randn_bf16(N, K, seed=seed + 1, scale=0.05)
    if regime == "cancel":
        x0 = x[0].to(F64)
        h = K // 2
        s = torch.ones(K, dtype=F64)
        s[h:] = -0.98 * float((x0[:h] ** 2).sum() / (x0[h:] ** 2).sum())
        a = 0.05 * (1.0 + 0.1 * torch.arange(N, dtype=F64)) \
            * (1.0 - 2.0 * (torch.arange(N) % 2))
        x = (x0[None] * (1.0 + 0.25 * torch.arange(M, dtype=F64))[:, None]
             ).to(torch.float32).to(torch.bfloat16)
        w = (a[:, None] * (s * x0)[None]).to(torch.float32).to(torch.bfloat16)
    else:
        assert regime == "randn", regime
    b = None
    if bias != "none":
        sc = {"bf16": 1.0, "x100": 100.0 * 0.025 * math.sqrt(K)}[bias]
        b = randn_bf16(N, seed=seed + 2, scale=sc)
    return x, w, b


# KC = 8192 / MT and a sweep of the 256 lanes covers 2048 elements: one
# sweep, one sweep + a vector, one chunk, one chunk + a vector, the Llama
# down projection (M = 1); the same around KC = 4096 (M = 2) and 2048 (M = 3
# runs the MT = 4 kernel with a padded row)
GEMV_K = {1: (8, 2048, 2056, 8192, 8200, 14336), 2: (4096, 4104),
          3: (2048, 2056, 4104), 4: (2048, 2056, 4104)}
# (M, N, K, bias, regime)
GEMV_CASES = [(M, N, K, b, "randn") for M, Ks in GEMV_K.items() for K in Ks
              for N in (1, 5) for b in ("none", "bf16")] \
    + [(1, 2051, 64, "bf16", "randn"), (4, 2051, 64, "bf16", "randn"),
       (1, 5, 2048, "x100", "randn"), (4, 5, 4104, "x100", "randn"),
       (1, 5, 14336, "none", "cancel"), (2, 5, 4104, "none", "cancel"),
       (4, 5, 4104, "none", "cancel"), (3, 5, 2056, "none", "cancel")]


@functools.lru_cache(maxsize=None)
def gemv_case(case):
    x, w, b = gemv_inputs(*case)
    a = (d(x), d(w), None if b is None else d(b))
    return dict(x=x, w=w, b=b, args=a, exact=gemv(*a, mode="exact"),
                rounded=gemv(*a, mode="rounded"))


# ---------------------------------------------------------------------------
# Merge plane: weighted_merge and grad_W on fp32 deltas
# ---------------------------------------------------------------------------
def seg_ids(offsets, P):
    return torch.repeat_interleave(torch.arange(len(offsets) - 1),
                                   offsets[1:] - offsets[:-1],
                                   output_size=P)


def weighted_merge(base, deltas, W, offsets, mode="exact",
                   mut: Optional[dict] = None):
    """merged[e] = sum_i W[i, seg(e)] (base[e] + deltas[i, e]); base [P],
    deltas [N,P], W [N,S] fp64 (fp32 values), offsets int64 [S+1].
    Mutants: boundary_prev_weight (the first element of segment j > 0 takes
    segment j - 1's weight), drop_last_model, w_transposed (W read as
    [seg, i]), base_once (base added once, not once per model)."""
    mut = mut or {}
    N, P = deltas.shape
    S = W.shape[1]
    if mode == "rounded":
        from distributedtraining_amd import ops
        return ops.weighted_merge(base.float(), deltas.float(), W.float(),
                                  offsets).to(F64)
    seg = seg_ids(offsets, P)
    if mut.get("boundary_prev_weight"):
        seg = seg.clone()
        first = offsets[1:-1][offsets[1:-1] < offsets[2:]]
        seg[first] = seg[first - 1]
    if mut.get("w_transposed"):
        W = W.reshape(-1).view(S, N).t()
    n = N - 1 if mut.get("drop_last_model") else N
    Ws = W[:n][:, seg]
    if mut.get("base_once"):
        return base + (Ws * deltas[:n]).sum(0)
    return (Ws * (base[None] + deltas[:n])).sum(0)


GW_LANES, GW_CHUNK = 256, 1 << 20


def lane_sum32(t: np.ndarray) -> np.float32:
    """fp32 sum of a chunk in grad_w_k's order: lane l of 256 adds elements
    l, l + 256, ... one at a time, then the 256 partials are folded one at a
    time (numpy keeps the running sums in fp32, see _serial_sum32)."""
    t = np.asarray(t, dtype=np.float32)
    if t.size == 0:
        return np.float32(0.0)
    pad = (-t.size) % GW_LANES
    a = np.concatenate([t, np.zeros(pad, np.float32)]).reshape(-1, GW_LANES)
    part = np.cumsum(a, axis=0, dtype=np.float32)[-1]
    return np.cumsum(part, dtype=np.float32)[-1]


def grad_w_fp32(g, base, deltas, merged, offsets, order="cpu"):
    """[N,S] fp32 grad_W from fp32 numpy planes, chunked and summed as the
    kernel does. order: cpu = g ((base - merged) + d), the CPU path's and
    the kernel's; parent = g ((base + d) - merged), the kernel's before."""
    N = deltas.shape[0]
    off = [int(o) for o in offsets]
    out = np.zeros((N, len(off) - 1), np.float32)
    bm = base - merged
    for i in range(N):
        t = g * ((bm + deltas[i]) if order == "cpu"
                 else ((base + deltas[i]) - merged))
        for j in range(len(off) - 1):
            acc = np.float32(0.0)
            for s0 in range(off[j], off[j + 1], GW_CHUNK):
                acc = np.float32(
                    acc + lane_sum32(t[s0:min(s0 + GW_CHUNK, off[j + 1])]))
            out[i, j] = acc
    return out


def grad_merge_weights(g, base, deltas, merged, offsets, mode="exact",
                       mut: Optional[dict] = None):
    """grad_W[i,j] = sum_{e in seg j} g[e] (base[e] + deltas[i,e] -
    merged[e]) on fp64 tensors holding the values the kernel reads.
    Mutants: no_merged, drop_seg_last (the last element of every segment),
    next_seg (a chunk's sum credited to segment j + 1)."""
    mut = mut or {}
    N, P = deltas.shape
    S = len(offsets) - 1
    if mode == "rounded":
        f = lambda t: t.to(torch.float32).numpy()   # noqa: E731
        return torch.from_numpy(grad_w_fp32(
            f(g), f(base), f(deltas), f(merged), offsets)).to(F64)
    seg = seg_ids(offsets, P)
    keep = torch.ones(P, dtype=F64)
    if mut.get("drop_seg_last"):
        last = offsets[1:][offsets[1:] > offsets[:-1]] - 1
        keep[last] = 0.0
    mg = torch.zeros_like(merged) if mut.get("no_merged") else merged
    out = torch.zeros(N, S, dtype=F64)
    for i in range(N):
        out[i].index_add_(0, seg, keep * g * (base + deltas[i] - mg))
    if mut.get("next_seg"):
        out = out.roll(1, 1)
    return out


def _odd_sizes(n):
    return tuple(1 + (7 * j * j + 3 * j) % 97 for j in range(n))


# segment tables: boundaries inside 16 B vectors; one-element segments; an
# empty segment (two equal offsets); a single segment; 291 segments of mixed
# odd sizes (the tensor count of Llama-3-8B); big: three chunks in one
# segment, so one output receives three atomic adds (grad_W only)
MERGE_TABLES = {"four": (1000, 37, 4096, 123), "ones": (1, 1, 1, 5),
                "empty": (300, 0, 41, 7), "single": (4099,),
                "t291": _odd_sizes(291),
                "big": (37, 2 * GW_CHUNK + 5, 123)}
MERGE_W = ("uniform", "rand", "signed")
# (table, N, W kind); "loop" is built from MAX_RESIDENT_BLOCKS by the caller
MERGE_CASES = [(t, n, wk) for t in ("four", "ones", "empty", "single", "t291")
               for n in (1, 3, 32) for wk in MERGE_W]


def max_resident_blocks() -> int:
    """MAX_RESIDENT_BLOCKS, the cap of the elementwise grids, from the
    header."""
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "distributedtraining_amd", "ops", "hip",
        "dta_common.h")
    with open(path) as f:
        return int(re.search(r"MAX_RESIDENT_BLOCKS\s*=\s*(\d+)",
                             f.read()).group(1))


def merge_loop_table(max_resident_blocks: int):
    """A plane past MAX_RESIDENT_BLOCKS x 256 elements: the capped grid of
    weighted_merge_k (one element per lane) goes round a second time."""
    return (max_resident_blocks * 256 - 40, 37, 4099 + 3)


def merge_inputs(table, N, wkind, dscale=1e-3, seed=1000):
    """base [P] randn, deltas [N,P] = dscale randn, g [P] randn (fp32), W
    [N,S]: uniform = 1/N (the averager's start); rand in [0, 1]; signed =
    randn shifted so that every column sums to 1 (N = 1: ones)."""
    gen = torch.Generator().manual_seed(seed + N)
    P, S = sum(table), len(table)
    base = torch.randn(P, generator=gen)
    deltas = torch.randn(N, P, generator=gen) * dscale
    grad = torch.randn(P, generator=gen)
    if wkind == "uniform":
        W = torch.full((N, S), 1.0 / N)
    elif wkind == "rand":
        W = torch.rand(N, S, generator=gen)
    else:
        assert wkind == "signed", wkind
        r = torch.randn(N, S, generator=gen)
        W = r - r.mean(0, keepdim=True) + 1.0 / N
    offsets = torch.tensor([0] + list(np.cumsum(table)), dtype=torch.int64)
    return dict(P=P, base=base, deltas=deltas, W=W, g=grad, offsets=offsets)


def merge_case_uncached(table, N, wkind):
    t = merge_inputs(table, N, wkind)
    a = (d(t["base"]), d(t["deltas"]), d(t["W"]), t["offsets"])
    t.update(args=a, exact=weighted_merge(*a, mode="exact"),
             rounded=weighted_merge(*a, mode="rounded"))
    return t


@functools.lru_cache(maxsize=None)
def merge_case(case):
    table, N, wkind = case
    return merge_case_uncached(MERGE_TABLES[table], N, wkind)


# grad_W: (table, N, regime, g dtype). d1e-3 / d1e-5: deltas of that scale
# under W = 1/N, where merged = base + mean delta and the term cancels (the
# production regime); wrand: W rand, columns not summing to 1, no
# cancellation. The 2^21-element table keeps to three cases.
GRADW_REGIMES = {"d1e-3": (1e-3, "uniform"), "d1e-5": (1e-5, "uniform"),
                 "wrand": (1e-3, "rand")}
GRADW_CASES = [(t, 3, r, gd) for t in ("four", "ones", "empty", "single",
                                       "t291")
               for r in GRADW_REGIMES for gd in ("fp32", "bf16")] \
    + [("four", 32, r, "fp32") for r in GRADW_REGIMES] \
    + [("big", 3, "d1e-5", "fp32"), ("big", 3, "d1e-5", "bf16"),
       ("big", 3, "wrand", "fp32")]


def gradw_case_uncached(case):
    """merged is the fp64 merge rounded to fp32: an input that does not come
    from the kernel under test. g_src: the fp32 plane a bf16 g was rounded
    from."""
    table, N, regime, gd = case
    dscale, wkind = GRADW_REGIMES[regime]
    t = merge_inputs(MERGE_TABLES[table], N, wkind, dscale)
    merged = weighted_merge(d(t["base"]), d(t["deltas"]), d(t["W"]),
                            t["offsets"]).to(torch.float32)
    g = t["g"] if gd == "fp32" else t["g"].to(torch.bfloat16)
    a = (d(g), d(t["base"]), d(t["deltas"]), d(merged), t["offsets"])
    t.update(merged=merged, g_in=g, g_src=t["g"], args=a,
             exact=grad_merge_weights(*a, mode="exact"),
             rounded=grad_merge_weights(*a, mode="rounded"))
    return t


@functools.lru_cache(maxsize=None)
def gradw_case(case):
    return gradw_case_uncached(case)


# ---------------------------------------------------------------------------
# ce_chunk + ce_finalize: the logits of a CE case consumed in column tiles
# ---------------------------------------------------------------------------
def ce_tiles(logits, targets, tiles, ignore_index,
             mut: Optional[dict] = None):
    """fp64 model of ce_chunk over the column tiles (widths ``tiles``)
    followed by ce_finalize, from the state m = -inf, s = 0, tlogit = 0.
    Returns lse, loss_sum, count, tlogit. Mutants: no_rescale (a tile is
    added without rescaling the running sum), v0_off (v0 off by one in the
    target lookup), drop_tail (the scalar tail of a tile whose width is no
    multiple of 8), count_ignored."""
    mut = mut or {}
    T = logits.shape[0]
    m = torch.full((T,), float("-inf"), dtype=F64)
    s = torch.zeros(T, dtype=F64)
    tl = torch.zeros(T, dtype=F64)
    ninf = torch.full((T,), float("-inf"), dtype=F64)
    v0 = 0
    for wd in tiles:
        x = logits[:, v0:v0 + wd]
        if mut.get("drop_tail"):
            x = x[:, :wd - wd % 8]
        M = x.amax(1) if x.shape[1] else ninf
        mn = torch.maximum(m, M)
        fin = torch.isfinite(mn)
        safe = torch.where(fin, mn, torch.zeros_like(mn))
        S = torch.exp(x - safe[:, None]).sum(1)      # = S_tile exp(M - mn)
        keep = torch.ones_like(s) if mut.get("no_rescale") \
            else torch.exp(m - safe)
        s = torch.where(fin, s * keep + S, s)
        m = mn
        tc = targets - v0 - (1 if mut.get("v0_off") else 0)
        hit = (tc >= 0) & (tc < wd)
        tl[hit] = logits[hit, (v0 + tc)[hit]]
        v0 += wd
    assert v0 == logits.shape[1]
    lse = m + torch.log(s)
    valid = torch.ones(T, dtype=torch.bool) if mut.get("count_ignored") \
        else targets != ignore_index
    return dict(lse=lse, loss_sum=(lse - tl)[valid].sum(),
                count=int(valid.sum()), tlogit=tl)


# the CE shapes split into column tiles: odd widths (3 + 4; 505), a tail of
# fewer than 8 columns, v0 no multiple of 8 (8 + 505), one tile, the GPT-2
# vocabulary with its odd last tile, and 4099 rows (the 4096-block grid of
# ce_chunk_k loops)
CE_TILINGS = [((5, 7), (3, 4)), ((33, 1000), (640, 360)),
              ((33, 1000), (1000,)), ((16, 520), (8, 505, 7)),
              ((8, 50257), (16384, 16384, 50257 - 2 * 16384)),
              ((4099, 24), (9, 15))]
# (rows, vocab, regime, tiles, peak); peak first / last: one column of the
# first / last tile raised by 12 in every row, so the row maximum arrives
# with the first tile and never moves, or moves in the last
CE_TILE_CASES = [(r, v, g, t, None) for (r, v), t in CE_TILINGS
                 for g in CE_REGIMES] \
    + [(r, v, "randn3", t, p) for (r, v), t in CE_TILINGS if len(t) > 1
       for p in ("first", "last")]


@functools.lru_cache(maxsize=None)
def ce_tile_case(case):
    """ce_inputs of the shape, with the target of row 3 on the first column
    of the second tile and that of row 2 on the last column of the first
    (one tile: columns 0 and V - 1)."""
    rows, vocab, regime, tiles, peak = case
    x, tg = ce_inputs(rows, vocab, regime)
    x, tg = x.float(), tg.clone()
    if peak is not None:
        x[:, 1 if peak == "first" else vocab - 2] += 12.0
    first = tiles[0] if len(tiles) > 1 else 0
    tg[3], tg[2] = first, (first - 1) % vocab
    x = x.to(torch.bfloat16)
    a = (d(x), tg, -100, 1.0)
    ex = cross_entropy(*a, mode="exact")
    rd = cross_entropy(*a, mode="rounded")
    keys = ("lse", "loss_sum", "count")
    return dict(x=x, tg=tg, tiles=tiles, exact={k: ex[k] for k in keys},
                rounded={k: rd[k] for k in keys})


# ---------------------------------------------------------------------------
# Every name the extension exports, and where its reference lives: a test
# module, or the reason why the export computes nothing to hold against one
# (tests/test_numerics_selfcheck.py::test_every_export_has_a_reference)
# ---------------------------------------------------------------------------
_ACC = "tests/test_kernel_accuracy_gpu.py"
_OPS = "tests/test_ops_gpu.py"
_BIAS = "tests/test_bias_grad_gpu.py"
_GUARD = "tests/test_guarded_step_gpu.py"
_PACKED = "tests/test_packed_merge_gpu.py"
EXPORTS = {
    "layernorm_fwd": _ACC, "layernorm_bwd": _ACC, "rmsnorm_fwd": _ACC,
    "rmsnorm_bwd": _ACC, "gelu_fwd": _ACC, "gelu_bwd": _ACC,
    "gelu_bwd_colsum": _BIAS, "swiglu_fwd": _ACC, "swiglu_bwd": _ACC,
    "dropout_apply": _OPS,
    "rng_tick": "not numeric: increments the int64 dropout step counter",
    "accum_f32_into_bf16": _ACC, "delta_sub": _ACC, "axpy": _ACC,
    "has_nan": _ACC, "l2norm_sq": _ACC, "adamw_step": _ACC,
    "adamw_tick": _ACC,
    "grad_sumsq_blocks": "not numeric: the number of partials the norm "
                         "pass writes for a length",
    "grad_sumsq_partials": _GUARD, "step_control": _GUARD,
    "adamw_step_guarded": _GUARD, "colsum": _ACC, "weighted_merge": _ACC,
    "grad_merge_weights": _ACC, "weighted_merge_packed": _PACKED,
    "grad_merge_weights_packed": _PACKED, "axpy_packed": _PACKED,
    "quantize_int8": _PACKED, "ce_fwd": _ACC, "ce_bwd": _ACC,
    "ce_fwd_bwd": _ACC, "ce_chunk": _ACC, "ce_finalize": _ACC,
    "head_loss_fwd": _ACC, "embedding_fwd": _ACC, "embedding_bwd": _ACC,
    "kv_append": _ACC,
    "i32_inc": _ACC, "gemv": _ACC, "rope_fwd": _ACC, "rope_bwd": _ACC,
    "attn_fwd": _ACC, "attn_bwd": _ACC, "attn_bwd_packed": _ACC,
    "attn_bwd_fused_enable": "not numeric: switches the single-tile fused "
                             "backward on or off",
    "attn_bwd_fused_calls": "not numeric: counts launches of the fused "
                            "backward",
    "attn_decode": _ACC,
    "mfma_selftest_16": "not numeric: dumps the MFMA fragment layout "
                        "(test_mfma_layout_16x16x32)",
    "mfma_selftest_32": "not numeric: dumps the MFMA fragment layout "
                        "(test_mfma_layout_32x32x16)",
    "lt_linear_gelu_fwd": _OPS, "lt_dgrad_dgelu_bgrad": _OPS,
    "lt_wgrad_bgradb": _OPS,
}
