#!/usr/bin/env python3
"""SHA-256 of every output of the norm, dropout, attention and decode entry
points on seeded inputs with the dropout counter pinned — a bit-for-bit
fingerprint for refactors that must not change arithmetic.

Each case runs twice; an output whose bytes differ between the two runs
(atomically reduced dγ/dβ, GQA dk/dv) is listed as ``unstable`` and left out
of comparisons.

    python tools/op_digest.py > new.txt
    python tools/op_digest.py --root <other checkout> > old.txt
    python tools/op_digest.py --against old.txt   # exit 1 on any mismatch
"""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), help="checkout whose built package to load")
ap.add_argument("--against", help="listing to compare the digests with")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402
from distributedtraining_amd.ops.backend import require_ext  # noqa: E402

m = require_ext()
DEV = "cuda:0"
CTR, SITE, P = 20240607, 5, 0.1
rng = torch.full((1,), CTR, dtype=torch.int64, device=DEV)
empty = torch.empty(0, dtype=torch.bfloat16, device=DEV)
_gen = torch.Generator(device="cpu")


def rand(*shape, seed, scale=1.0):
    _gen.manual_seed(seed)
    return (torch.randn(*shape, generator=_gen) * scale).to(DEV,
                                                            torch.bfloat16)


def norm_case(rows, cols, fused):
    x, w, b = (rand(rows, cols, seed=1), rand(cols, seed=2, scale=0.5),
               rand(cols, seed=3, scale=0.5))
    res = rand(rows, cols, seed=4) if fused else empty
    ds = rand(rows, cols, seed=5) if fused else empty
    dy = rand(rows, cols, seed=6)
    site, p = (SITE, P) if fused else (0, 0.0)
    out = {}
    y, mean, rstd, s = m.layernorm_fwd(x, res, w, b, 1e-5, rng, site, p)
    out.update({"layernorm_fwd.y": y, "layernorm_fwd.mean": mean,
                "layernorm_fwd.rstd": rstd, "layernorm_fwd.sum": s})
    dx, dw, db, dres = m.layernorm_bwd(dy, ds, s if fused else x, w, mean,
                                       rstd, rng, site, p)
    out.update({"layernorm_bwd.dx": dx, "layernorm_bwd.dw": dw,
                "layernorm_bwd.db": db, "layernorm_bwd.dres": dres})
    y, rstd, s = m.rmsnorm_fwd(x, res, w, 1e-5, rng, site, p)
    out.update({"rmsnorm_fwd.y": y, "rmsnorm_fwd.rstd": rstd,
                "rmsnorm_fwd.sum": s})
    dx, dw, dres = m.rmsnorm_bwd(dy, ds, s if fused else x, w, rstd, rng,
                                 site, p)
    out.update({"rmsnorm_bwd.dx": dx, "rmsnorm_bwd.dw": dw,
                "rmsnorm_bwd.dres": dres})
    return out


def dropout_case(n):
    return {"dropout_apply.y": m.dropout_apply(rand(n, seed=7), rng, SITE, P)}


def attn_case(B, H, Hk, S, D):
    F = (H + 2 * Hk) * D
    qkv = rand(B, S, F, seed=8)

    def views(t):   # packed [B,S,(H+2Hk)D] -> q/k/v [B,heads,S,D] views
        return (t.as_strided((B, H, S, D), (S * F, D, F, 1), 0),
                t.as_strided((B, Hk, S, D), (S * F, D, F, 1), H * D),
                t.as_strided((B, Hk, S, D), (S * F, D, F, 1), (H + Hk) * D))

    q, k, v = views(qkv)
    kvlen = torch.tensor([S - 29 * i for i in range(B)], dtype=torch.int32,
                         device=DEV)
    dout = rand(B, S, H, D, seed=9).permute(0, 2, 1, 3)
    scale = D ** -0.5
    o, lse = m.attn_fwd(q, k, v, scale, kvlen, rng, SITE, P)
    dq, dk, dv = m.attn_bwd(dout, q, k, v, o, lse, scale, kvlen, rng, SITE, P)
    dqkv = torch.zeros_like(qkv)
    pq, pk, pv = (t.permute(0, 2, 1, 3) for t in views(dqkv))
    m.attn_bwd_packed(dout, q, k, v, o, lse, scale, pq, pk, pv, kvlen, rng,
                      SITE, P)
    return {"attn_fwd.o": o, "attn_fwd.lse": lse, "attn_bwd.dq": dq,
            "attn_bwd.dk": dk, "attn_bwd.dv": dv, "attn_bwd_packed.dq": pq,
            "attn_bwd_packed.dk": pk, "attn_bwd_packed.dv": pv}


def decode_case(B, H, Hk, L, D):
    q = rand(B, H, D, seed=10)
    kc, vc = rand(B, Hk, L + 7, D, seed=11), rand(B, Hk, L + 7, D, seed=12)
    return {"attn_decode.o": m.attn_decode(
        q, kc, vc, L, D ** -0.5,
        torch.empty(0, dtype=torch.int32, device=DEV))}


CASES = [(f"norm[{r}x{c},{'res+drop' if f else 'plain'}]", norm_case,
          (r, c, f)) for r, c in ((128, 768), (33, 2560)) for f in (0, 1)]
CASES.append(("dropout[100003]", dropout_case, (100_003,)))
CASES += [(f"attn[{'x'.join(map(str, g))}]", attn_case, g)
          for g in ((2, 4, 4, 96, 64), (2, 8, 2, 96, 64),
                    # S = 70: a second 64-row block, one wave partly live;
                    # all three head dims, direct and atomic dk/dv at 128
                    (2, 2, 2, 70, 32), (2, 4, 1, 70, 128), (2, 3, 3, 70, 64))]
CASES += [(f"decode[{'x'.join(map(str, g))}]", decode_case, g)
          for g in ((2, 4, 2, 130, 64), (1, 4, 4, 130, 128))]


def digests(fn, a):
    return {k: hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy()
                              .tobytes()).hexdigest()
            for k, t in fn(*a).items() if t.numel()}


listing = {}
for name, fn, a in CASES:
    first, second = digests(fn, a), digests(fn, a)
    for k in first:
        listing[f"{name} {k}"] = (first[k] if first[k] == second[k]
                                  else "unstable")
for k, d in listing.items():
    print(k, d)

if args.against:
    with open(args.against) as f:
        other = dict(line.rstrip("\n").rsplit(" ", 1) for line in f
                     if line.strip() and not line.startswith("#"))
    assert other.keys() == listing.keys(), "listings cover different outputs"
    skipped = [k for k in listing
               if "unstable" in (listing[k], other[k])]
    bad = [k for k in listing if k not in skipped and listing[k] != other[k]]
    print(f"# compared {len(listing) - len(skipped)} outputs, "
          f"{len(skipped)} unstable excluded, {len(bad)} mismatched")
    for k in skipped:
        print("# excluded:", k)
    for k in bad:
        print("# MISMATCH:", k)
    sys.exit(1 if bad else 0)
