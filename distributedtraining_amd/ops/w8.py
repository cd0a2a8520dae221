"""Int8 weight-only serving format (W8A16) and its projection.

A ``QuantWeight`` stands where a bf16 ``[N, K]`` projection weight stood:
int8 codes with one fp32 scale per (row, group of 128 along K), prepacked
once, offline, in the order the kernel of hip/w8_gemv.hip streams them.

Definition (group g of row n covers columns 128 g .. 128 g + 127):

* ``scale[n, g] = amax(|w[n, group]|) / 127`` in fp32; an all-zero group
  takes scale 1;
* ``q = clamp(rint(w / scale), -127, 127)`` as int8;
* the represented weight is ``float(q) * scale``, an fp32 product.

Packing: rows padded with zero codes to ``Np = ceil16(N)``; codes
``int8 [Np/16][K/64][64][16]``: the 1 KB of a (16-row tile, 64-wide K-step)
in lane order, lane ``l`` holding row ``l % 16`` and the 16 columns
``16 (l // 16) ..`` of the step; scales ``fp32 [Np/16][K/128][16]``.
Quantising and packing are plain torch ops on either device, a one-off at
load. Inference only.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from .backend import require_ext, use_hip

GROUP = 128      # K columns per scale
MAX_ROWS = 16    # activation rows the streaming kernel takes


class QuantWeight:
    """Packed int8 weight of a ``[N, K]`` projection (see module docstring).
    Not a Parameter: it carries no gradient and is not part of a state dict
    or of the flat training plane."""

    def __init__(self, codes: torch.Tensor, scales: torch.Tensor, N: int,
                 K: int):
        self.codes, self.scales, self.N, self.K = codes, scales, N, K

    @property
    def shape(self):
        return (self.N, self.K)

    @property
    def device(self):
        return self.codes.device

    def nbytes(self) -> int:
        return (self.codes.numel() * self.codes.element_size()
                + self.scales.numel() * self.scales.element_size())

    def to(self, device) -> "QuantWeight":
        return QuantWeight(self.codes.to(device), self.scales.to(device),
                           self.N, self.K)

    def __repr__(self):
        return f"QuantWeight(N={self.N}, K={self.K}, device={self.device})"


def quantize_weight_int8(w: torch.Tensor) -> QuantWeight:
    """bf16 / fp32 ``[N, K]`` weight -> packed ``QuantWeight``. Raises on
    ``K % 128 != 0`` and on a non-finite weight."""
    if w.dim() != 2 or w.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("quantize_weight_int8 takes a bf16 or fp32 [N, K] "
                         f"weight, got {w.dtype} {tuple(w.shape)}")
    N, K = w.shape
    if N < 1 or K < GROUP or K % GROUP != 0:
        raise ValueError(f"K must be a multiple of {GROUP}, got K = {K}")
    wf = w.detach().to(torch.float32)
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_weight_int8: non-finite weight")
    g = wf.view(N, K // GROUP, GROUP)
    scale = g.abs().amax(dim=-1) / 127.0
    scale = torch.where(scale == 0, torch.ones_like(scale), scale)
    q = torch.clamp(torch.round(g / scale[..., None]), -127, 127) \
        .to(torch.int8).view(N, K)
    Np = (N + 15) // 16 * 16
    if Np != N:
        q = torch.cat([q, q.new_zeros(Np - N, K)])
        scale = torch.cat([scale, scale.new_ones(Np - N, K // GROUP)])
    # [tile, row, step, quarter, byte] -> [tile, step, quarter * 16 + row, byte]
    codes = q.view(Np // 16, 16, K // 64, 4, 16).permute(0, 2, 3, 1, 4) \
        .reshape(Np // 16, K // 64, 64, 16).contiguous()
    scales = scale.view(Np // 16, 16, K // GROUP).permute(0, 2, 1).contiguous()
    return QuantWeight(codes, scales, N, K)


def unpack_weight(qw: QuantWeight):
    """(codes int8 [N, K], scales fp32 [N, K/128]) in row-major order: the
    inverse of the packing, without the padded rows."""
    Np, K = qw.codes.shape[0] * 16, qw.K
    q = qw.codes.view(Np // 16, K // 64, 4, 16, 16).permute(0, 3, 1, 2, 4) \
        .reshape(Np, K)
    s = qw.scales.permute(0, 2, 1).reshape(Np, K // GROUP)
    return q[:qw.N], s[:qw.N]


def dequantize_weight(qw: QuantWeight,
                      dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Dense ``[N, K]`` weight: ``float(q) * scale`` rounded once to
    ``dtype``."""
    q, s = unpack_weight(qw)
    w = q.to(torch.float32).view(qw.N, qw.K // GROUP, GROUP) * s[..., None]
    return w.view(qw.N, qw.K).to(dtype)


def linear_w8(x: torch.Tensor, qw: QuantWeight,
              b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``ops.linear`` with a ``QuantWeight``. GPU: up to 16 rows stream the
    packed weight through w8_gemv; more rows (prefill) dequantise it into a
    scratch bf16 weight for the library GEMM. CPU: F.linear on the
    dequantised weight."""
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError("a QuantWeight projection is inference-only: run "
                           "it under torch.no_grad()")
    if x.shape[-1] != qw.K:
        raise ValueError(f"x has {x.shape[-1]} columns, the weight K = {qw.K}")
    if not use_hip(x):
        return F.linear(x, dequantize_weight(qw, x.dtype), b)
    m = require_ext()
    rows = x.numel() // qw.K
    if 1 <= rows <= MAX_ROWS:
        x2 = x.reshape(rows, qw.K)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        y = m.w8_gemv(x2, qw.codes, qw.scales, b, qw.N)
        return y.view(*x.shape[:-1], qw.N)
    from . import linear
    with torch.no_grad():
        return linear(x, m.w8_dequant(qw.codes, qw.scales, qw.N), b)
