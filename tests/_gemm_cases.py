"""Inputs, fp64 reference and the case list of the forward projection GEMM
(hip/gemm.hip) for tests/test_gemm_gpu.py. A plain helper module.

    y = x w^T (+ b)        pre = x w^T + b, h = gelu(pre)

``exact`` is fp64 throughout. The kernel accumulates in fp32, adds the bias in
fp32 and rounds ONCE, so ``rounded`` is bf16(exact); h is checked bit for bit
against gelu_fwd of the stored pre and needs no reference of its own.
"""

from __future__ import annotations

import functools

import torch

import _numerics as N

# the kernel's tile (tokens x features) and K granule; the GPU test asserts
# these against the extension's own constants
BM, BN, BK = 256, 128, 64

# (T, N, K, pad): one row; a ragged row tile; an odd K-step count (stage
# parity) behind a padded row stride; tile indexing both ways; 12 blocks, so
# the XCD remap wraps. pad: extra row stride of x in elements.
CASES = [
    (1, BN, BK, 0),
    (BM - 1, 2 * BN, 2 * BK, 0),
    (BM + 5, BN, 3 * BK, 8),
    (2 * BM, 3 * BN, BK, 0),
    (3 * BM + 1, 3 * BN, 2 * BK, 0),
]
# (case, regime, epilogue): every epilogue meets both regimes, the ragged
# cases and the pad case
PARAMS = [
    (0, "randn", "none"), (0, "randn", "bias_gelu"),
    (1, "cancel", "none"), (1, "randn", "bias"), (1, "cancel", "bias_gelu"),
    (2, "randn", "none"), (2, "cancel", "bias"), (2, "randn", "bias_gelu"),
    (2, "cancel", "bias_gelu"),
    (3, "cancel", "none"), (3, "randn", "bias"), (3, "cancel", "bias_gelu"),
    (4, "randn", "none"), (4, "cancel", "bias"), (4, "randn", "bias"),
    (4, "randn", "bias_gelu"),
]


def param_id(p) -> str:
    (T, Nf, K, pad), regime, epi = CASES[p[0]], p[1], p[2]
    return f"T{T}-{Nf}x{K}-pad{pad}-{regime}-{epi}"


def gemm_inputs(T, Nf, K, regime, seed=1400):
    """x [T, K], w [N, K], b [N] as CPU bf16. randn: x = 0.5 randn, w = 0.05
    randn, b = 0.1 randn. cancel: with h = K // 2, columns h.. of x repeat
    columns ..h and those of w are -0.98 x the first half's, so the two halves
    of every dot product cancel to 2 % of their size."""
    x = N.randn_bf16(T, K, seed=seed, scale=0.5)
    w = N.randn_bf16(Nf, K, seed=seed + 1, scale=0.05)
    if regime == "cancel":
        h = K // 2
        x[:, h:2 * h] = x[:, :h]
        w[:, h:2 * h] = (-0.98 * w[:, :h].double()).to(torch.float32) \
            .to(torch.bfloat16)
    else:
        assert regime == "randn", regime
    return x, w, N.randn_bf16(Nf, seed=seed + 2, scale=0.1)


@functools.lru_cache(maxsize=None)
def case(i, regime):
    """Inputs and the exact products of one case, without and with the bias;
    never modified afterwards."""
    T, Nf, K, pad = CASES[i]
    x, w, b = gemm_inputs(T, Nf, K, regime, seed=1400 + 10 * i)
    prod = N.d(x) @ N.d(w).t()
    return dict(x=x, w=w, b=b, pad=pad, none=prod, bias=prod + N.d(b))
