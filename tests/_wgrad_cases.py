"""Inputs, fp64 references and the case list of the weight-gradient kernel
(hip/wgrad.hip), shared by tests/test_wgrad_cpu.py (the bound rejects this
kernel's possible mistakes) and tests/test_wgrad_gpu.py. A plain helper module.

    dW = dst_w + dy^T x          db = dst_b + sum_t dy

``exact`` is fp64 throughout. The kernel accumulates in fp32 and rounds ONCE,
at the fold (dst = bf16(float(dst) + sum)), so ``rounded`` is bf16(exact); the
fp32 bias store has no bf16 rounding and its baseline is the fp32 torch sum
(_numerics.colsum).
"""

from __future__ import annotations

import functools

import torch

import _numerics as N

# the kernel's tile (rows of dW x columns of dW) and K-step; the GPU test
# asserts these against the extension's own constants
BM, BN, BK = 256, 128, 32

REGIMES = ("randn", "cancel")


def wgrad_inputs(T, out, inp, regime, seed=1100):
    """dy [T, out], x [T, in], dst_w [out, in], dst_b [out] as CPU bf16, the
    regimes of _numerics.gemv_inputs carried over to a sum over t.
    randn: dy = 0.05 randn, x = 0.5 randn. cancel: with h = T // 2, row h + t
    of x repeats row t and row h + t of dy is -0.98 x row t, so the two halves
    of the t range cancel to 2 % of their size, in dW and in db alike; an odd
    last row of dy is random at 1/8 of the scale (one full-size row would be
    several times what the halves leave). The destinations are non-zero
    (0.1 randn)."""
    dy = N.randn_bf16(T, out, seed=seed, scale=0.05)
    x = N.randn_bf16(T, inp, seed=seed + 1, scale=0.5)
    if regime == "cancel":
        h = T // 2
        assert h >= 1
        x[h:2 * h] = x[:h]
        dy[h:2 * h] = (-0.98 * dy[:h].double()).to(torch.float32) \
            .to(torch.bfloat16)
        dy[2 * h:] = (dy[2 * h:].float() / 8).to(torch.bfloat16)
    else:
        assert regime == "randn", regime
    return (dy, x, N.randn_bf16(out, inp, seed=seed + 2, scale=0.1),
            N.randn_bf16(out, seed=seed + 3, scale=0.1))


def reference(dy, x, dst_w, dst_b, mut=None):
    """exact dW and db (fp64). Mutants, each a mistake this kernel can make:
    drop_last_row (the last t row), drop_slice=(lo, hi) (the rows of one K
    slice), garbage_tail=(g_dy, g_x) (the zero padding of the ragged last
    K-step read as those rows instead), bias_next_tile (db of row tile i
    taken from tile i + 1), overwrite (dst not accumulated)."""
    mut = mut or {}
    dy, x = N.d(dy), N.d(x)
    if mut.get("drop_last_row"):
        dy, x = dy[:-1], x[:-1]
    if "drop_slice" in mut:
        lo, hi = mut["drop_slice"]
        keep = torch.ones(dy.shape[0], dtype=torch.bool)
        keep[lo:hi] = False
        dy, x = dy[keep], x[keep]
    if "garbage_tail" in mut:
        g_dy, g_x = mut["garbage_tail"]
        dy, x = torch.cat([dy, N.d(g_dy)]), torch.cat([x, N.d(g_x)])
    dw = dy.t() @ x
    db = dy.sum(0)
    if mut.get("bias_next_tile"):
        db = db.roll(-BM)
    if not mut.get("overwrite"):
        dw = dw + N.d(dst_w)
        db = db + N.d(dst_b)
    return dict(dw=dw, db=db)


def slice_rows(T, nsplit, s):
    """Rows [lo, hi) of K slice s: whole K-steps, dta_wgrad's partition."""
    ksteps = (T + BK - 1) // BK
    return (min(T, ksteps * s // nsplit * BK),
            min(T, ksteps * (s + 1) // nsplit * BK))


# T, out, in, forced nsplit (0: automatic), bias ("dst": accumulated into a
# bf16 view, "f32": fp32 store, "none"), off: destination views start this
# many elements into their buffers (1: 2 B aligned only), pad: extra row
# stride of dy / x in elements (the packed-qkv views).
#   T = BK - 1: one ragged K-step; 2 BK + 5; 1; 6 BK + 17 in 3 slices (the
#   last one ragged); BK in 4 slices (three of them empty).
#   2 BM x BN and BM x 3 BN: tile indexing in both directions.
CASES = [
    dict(T=BK - 1, out=2 * BM, inp=BN, ns=1, bias="dst", off=1, pad=0),
    dict(T=2 * BK + 5, out=BM, inp=3 * BN, ns=1, bias="f32", off=0, pad=64),
    dict(T=1, out=2 * BM, inp=BN, ns=1, bias="dst", off=0, pad=0),
    dict(T=6 * BK + 17, out=2 * BM, inp=BN, ns=3, bias="dst", off=1, pad=8),
    dict(T=6 * BK + 17, out=BM, inp=3 * BN, ns=3, bias="f32", off=1, pad=0),
    dict(T=BK, out=BM, inp=3 * BN, ns=4, bias="dst", off=0, pad=0),
    dict(T=2 * BK + 5, out=2 * BM, inp=BN, ns=1, bias="none", off=1, pad=0),
    dict(T=6 * BK + 17, out=BM, inp=3 * BN, ns=0, bias="none", off=0, pad=8),
]
CASE_REGIMES = [(i, r) for i in range(len(CASES)) for r in REGIMES
                if not (r == "cancel" and CASES[i]["T"] < 2)]


def case_id(cr) -> str:
    c, r = CASES[cr[0]], cr[1]
    return (f"T{c['T']}-{c['out']}x{c['inp']}-ns{c['ns']}-{c['bias']}"
            f"-off{c['off']}-pad{c['pad']}-{r}")


@functools.lru_cache(maxsize=None)
def case(i, regime):
    """Inputs and both references of one case; never modified afterwards."""
    c = CASES[i]
    dy, x, dst_w, dst_b = wgrad_inputs(c["T"], c["out"], c["inp"], regime,
                                       seed=1100 + 10 * i)
    exact = reference(dy, x, dst_w, dst_b)
    rounded = dict(dw=N.bf16(exact["dw"]), db=N.bf16(exact["db"]))
    # the fp32 store has no destination: plain column sums
    db32_exact = N.colsum(N.d(dy))
    db32_rounded = N.colsum(N.d(dy), mode="rounded")
    return dict(c=c, dy=dy, x=x, dst_w=dst_w, dst_b=dst_b, exact=exact,
                rounded=rounded, db32_exact=db32_exact,
                db32_rounded=db32_rounded)
