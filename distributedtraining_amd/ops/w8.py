"""Weight-only serving formats (W8A16, W4A16) and their projection.

A ``QuantWeight`` stands where a bf16 ``[N, K]`` projection weight stood:
int8 (``bits == 8``) or int4 (``bits == 4``) codes with one fp32 scale per
(row, group of 128 along K), prepacked once, offline, in the order the
kernels of hip/w8_gemv.hip and hip/w4_gemv.hip stream them.

Int8
----

Definition (group g of row n covers columns 128 g .. 128 g + 127):

* ``scale[n, g] = amax(|w[n, group]|) / 127`` in fp32; an all-zero group
  takes scale 1;
* ``q = clamp(rint(w / scale), -127, 127)`` as int8;
* the represented weight is ``float(q) * scale``, an fp32 product.

Packing: rows padded with zero codes to ``Np = ceil16(N)``; codes
``int8 [Np/16][K/64][64][16]``: the 1 KB of a (16-row tile, 64-wide K-step)
in lane order, lane ``l`` holding row ``l % 16`` and the 16 columns
``16 (l // 16) ..`` of the step; scales ``fp32 [Np/16][K/128][16]``.

Int4
----
* ``scale[n, g] = amax(|w[n, group]|) / 7`` in fp32; an all-zero group takes
  scale 1;
* ``q = clamp(rint(w / scale), -7, 7)``, the divide in fp32, round-half-even;
  the stored nibble is ``u = q + 8`` in 1 .. 15;
* the represented weight is ``float(u - 8) * scale``, an fp32 product.

Packing: rows padded with the zero code (nibble 8) to ``Np``; codes
``uint8 [Np/16][K/128][64][16]``: the 1 KB of a (16-row tile, group) in lane
order, lane ``l`` holding row ``l % 16`` and the 32 columns ``32 (l // 16) ..``
of the group as four little-endian dwords. Dword ``d`` holds columns
``32 (l // 16) + 8 d + e``, ``e = 0 .. 7``: nibble ``s`` (bits ``4 s ..``) is
``e = 2 s`` and nibble ``s + 4`` is ``e = 2 s + 1``, so that
``(dword >> 4 s) & 0x000F000F`` is the pair ``(2 s, 2 s + 1)``. Scales as int8.

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
    """Packed int8 or int4 weight of a ``[N, K]`` projection (see module
    docstring); ``bits`` says which. Not a Parameter: it carries no gradient
    and is not part of a state dict or of the flat training plane."""

    def __init__(self, codes: torch.Tensor, scales: torch.Tensor, N: int,
                 K: int, bits: int = 8):
        if bits not in (4, 8):
            raise ValueError(f"bits must be 4 or 8, got {bits}")
        self.codes, self.scales, self.N, self.K = codes, scales, N, K
        self.bits = bits

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
                           self.N, self.K, self.bits)

    def __repr__(self):
        return (f"QuantWeight(N={self.N}, K={self.K}, bits={self.bits}, "
                f"device={self.device})")


def _quantize_groups(w: torch.Tensor, qmax: int, who: str):
    """(codes int8 [Np, K], scales fp32 [Np, K/128], N, K) by the group rule
    of the module docstring with ``|q| <= qmax``; rows padded to ``Np`` with
    zero codes and unit scales."""
    if w.dim() != 2 or w.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"{who} takes a bf16 or fp32 [N, K] "
                         f"weight, got {w.dtype} {tuple(w.shape)}")
    N, K = w.shape
    if N < 1 or K < GROUP or K % GROUP != 0:
        raise ValueError(f"K must be a multiple of {GROUP}, got K = {K}")
    wf = w.detach().to(torch.float32)
    if not bool(torch.isfinite(wf).all()):
        raise ValueError(f"{who}: non-finite weight")
    g = wf.view(N, K // GROUP, GROUP)
    scale = g.abs().amax(dim=-1) / float(qmax)
    scale = torch.where(scale == 0, torch.ones_like(scale), scale)
    q = torch.clamp(torch.round(g / scale[..., None]), -qmax, qmax) \
        .to(torch.int8).view(N, K)
    Np = (N + 15) // 16 * 16
    if Np != N:
        q = torch.cat([q, q.new_zeros(Np - N, K)])
        scale = torch.cat([scale, scale.new_ones(Np - N, K // GROUP)])
    return q, scale, N, K


def quantize_weight_int8(w: torch.Tensor) -> QuantWeight:
    """bf16 / fp32 ``[N, K]`` weight -> packed ``QuantWeight``. Raises on
    ``K % 128 != 0`` and on a non-finite weight."""
    q, scale, N, K = _quantize_groups(w, 127, "quantize_weight_int8")
    Np = q.shape[0]
    # [tile, row, step, quarter, byte] -> [tile, step, quarter * 16 + row, byte]
    codes = q.view(Np // 16, 16, K // 64, 4, 16).permute(0, 2, 3, 1, 4) \
        .reshape(Np // 16, K // 64, 64, 16).contiguous()
    scales = scale.view(Np // 16, 16, K // GROUP).permute(0, 2, 1).contiguous()
    return QuantWeight(codes, scales, N, K)


# byte b of an int4 dword: its low nibble is fragment element _W4_LO[b], its
# high nibble element _W4_HI[b] (nibble s = element 2 s, s + 4 = 2 s + 1)
_W4_LO = (0, 4, 1, 5)
_W4_HI = (2, 6, 3, 7)


def quantize_weight_int4(w: torch.Tensor) -> QuantWeight:
    """bf16 / fp32 ``[N, K]`` weight -> packed int4 ``QuantWeight`` (g128,
    ``|q| <= 7``). Raises on ``K % 128 != 0`` and on a non-finite weight."""
    q, scale, N, K = _quantize_groups(w, 7, "quantize_weight_int4")
    Np = q.shape[0]
    u = (q + 8).to(torch.uint8)
    # [tile, row, group, quarter, dword, element]
    u = u.view(Np // 16, 16, K // GROUP, 4, 4, 8)
    byts = u[..., list(_W4_LO)] | (u[..., list(_W4_HI)] << 4)
    # -> [tile, group, quarter * 16 + row, dword * 4 + byte]
    codes = byts.permute(0, 2, 3, 1, 4, 5) \
        .reshape(Np // 16, K // GROUP, 64, 16).contiguous()
    scales = scale.view(Np // 16, 16, K // GROUP).permute(0, 2, 1).contiguous()
    return QuantWeight(codes, scales, N, K, bits=4)


def unpack_weight(qw: QuantWeight):
    """(codes int8 [N, K], scales fp32 [N, K/128]) in row-major order: the
    inverse of the packing, without the padded rows. Int4 codes come back as
    ``q = u - 8`` in -7 .. 7."""
    Np, K = qw.codes.shape[0] * 16, qw.K
    s = qw.scales.permute(0, 2, 1).reshape(Np, K // GROUP)
    if qw.bits == 4:
        byts = qw.codes.view(Np // 16, K // GROUP, 4, 16, 4, 4)
        el = byts.new_empty(*byts.shape[:-1], 8)
        el[..., list(_W4_LO)] = byts & 15
        el[..., list(_W4_HI)] = byts >> 4
        q = el.permute(0, 3, 1, 2, 4, 5).reshape(Np, K).to(torch.int8) - 8
        return q[:qw.N], s[:qw.N]
    q = qw.codes.view(Np // 16, K // 64, 4, 16, 16).permute(0, 3, 1, 2, 4) \
        .reshape(Np, K)
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
    """``ops.linear`` with a ``QuantWeight`` of either width. GPU: up to 16
    rows stream the packed weight through w8_gemv / w4_gemv; more rows
    (prefill) dequantise it into a scratch bf16 weight for the library GEMM.
    CPU: F.linear on the dequantised weight."""
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError("a QuantWeight projection is inference-only: run "
                           "it under torch.no_grad()")
    if x.shape[-1] != qw.K:
        raise ValueError(f"x has {x.shape[-1]} columns, the weight K = {qw.K}")
    if not use_hip(x):
        return F.linear(x, dequantize_weight(qw, x.dtype), b)
    m = require_ext()
    gemv, dequant = ((m.w4_gemv, m.w4_dequant) if qw.bits == 4
                     else (m.w8_gemv, m.w8_dequant))
    rows = x.numel() // qw.K
    if 1 <= rows <= MAX_ROWS:
        x2 = x.reshape(rows, qw.K)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        y = gemv(x2, qw.codes, qw.scales, b, qw.N)
        return y.view(*x.shape[:-1], qw.N)
    from . import linear
    with torch.no_grad():
        return linear(x, dequant(qw.codes, qw.scales, qw.N), b)
