"""Shared pieces of the packed-sequence tests (CPU and GPU).

The fp64 references are composed, not rewritten: a document-masked row is
exactly the independent attention of each of its documents, so ``exact`` and
``rounded`` come from ``_numerics.attention`` on each document's slice of
q, k, v, dO (with the slice of the dropout keep-mask and kvlen clipped to the
slice) written back into [B, H, S, D]. The bounds are then ``_numerics.check``'s
measured bf16-floor bounds; nothing here sets a tolerance.
"""

import functools
import math

import torch

import _numerics as N


def q_lo_of(starts, S):
    """int32 [B, S] from per-row document starts (each a sorted tuple that
    begins with 0): the start of the document holding each token."""
    rows = []
    for st in starts:
        assert st[0] == 0 and list(st) == sorted(set(st)) and st[-1] < S
        row = torch.zeros(S, dtype=torch.int32)
        for s0 in st:
            row[s0:] = s0
        rows.append(row)
    return torch.stack(rows)


def doc_slices(st, S):
    """[(s0, s1)] of one row's documents."""
    ends = list(st[1:]) + [S]
    return list(zip(st, ends))


# (B, H, Hkv, S, D), starts per row, kvlen or None, p — the issue's table
ATTN_DOC_CASES = [
    ((2, 2, 2, 64, 64), ((0, 17, 48), (0,)), None, 0.0),
    ((1, 2, 2, 48, 32), ((0, 1, 33),), None, 0.0),
    ((1, 2, 2, 130, 128), ((0, 31, 32, 65, 129),), None, 0.0),
    ((1, 4, 2, 96, 64), ((0, 40, 64),), None, 0.0),
    ((2, 2, 2, 130, 64), ((0, 64, 100), (0, 64, 100)), (130, 65), 0.1),
]
# diffuse: plain randn. rising: the keys of the row's last 16 positions x 4,
# so the running max moves in the last key tile after leading tiles were
# skipped (the online rescale from the (-inf, 0, 0) state).
ATTN_DOC_REGIMES = ("diffuse", "rising")


def doc_case_id(case) -> str:
    shape, starts, kv, p = case
    s = "x".join(map(str, shape)) + "-d" + "_".join(
        ".".join(map(str, st)) for st in starts)
    if kv is not None:
        s += "-kv" + "_".join(map(str, kv))
    if p:
        s += f"-p{p}"
    return s


@functools.lru_cache(maxsize=None)
def attn_doc_case(case, regime):
    """Inputs (CPU bf16; dO zero on rows outside the contract), q_lo, kvlen,
    live [B,H,S] and both composed references, computed once per case."""
    from distributedtraining_amd.ops import droprng
    (B, H, Hk, S, D), starts, kv, p = case
    q, k, v, do = N.attn_inputs(B, H, Hk, S, D, regime)
    kvlen = None if kv is None else torch.tensor(kv, dtype=torch.int32)
    live = N.live_rows(None if kvlen is None else kvlen.clamp(max=S), B, S)
    do = (do.float() * live[:, None, :, None]).to(torch.bfloat16)
    keep, inv_keep = None, 1.0
    if p:
        keep = torch.from_numpy(droprng.attn_keep_mask(
            B * H, S, S, N.DROP_CTR, N.DROP_SITE, p)).view(B, H, S, S)
        import numpy as np
        inv_keep = float(np.float32(droprng.inv_keep(p)))
    scale = 1.0 / math.sqrt(D)
    qd, kd, vd, dod = N.d(q), N.d(k), N.d(v), N.d(do)
    out = {}
    for mode in ("exact", "rounded"):
        ref = dict(o=torch.zeros(B, H, S, D, dtype=N.F64),
                   dq=torch.zeros(B, H, S, D, dtype=N.F64),
                   dk=torch.zeros(B, Hk, S, D, dtype=N.F64),
                   dv=torch.zeros(B, Hk, S, D, dtype=N.F64))
        for b in range(B):
            for s0, s1 in doc_slices(starts[b], S):
                kvl = None
                if kvlen is not None:
                    n_live = min(max(int(kvlen[b]) - s0, 0), s1 - s0)
                    if n_live == 0:
                        # no live key: every row of the document is outside
                        # the contract (dO is zero there) and its keys are
                        # padding, so all four tensors stay zero
                        continue
                    kvl = torch.tensor([n_live], dtype=torch.int32)
                sl = slice(s0, s1)
                r = N.attention(
                    qd[b:b + 1, :, sl], kd[b:b + 1, :, sl], vd[b:b + 1, :, sl],
                    dod[b:b + 1, :, sl], scale, kvl,
                    None if keep is None else keep[b:b + 1, :, sl, sl],
                    inv_keep, mode=mode)
                for name in ref:
                    ref[name][b:b + 1, :, sl] = r[name]
        out[mode] = ref
    return dict(q=q, k=k, v=v, do=do, kvlen=kvlen, scale=scale,
                q_lo=q_lo_of(starts, S),
                live=live[:, None, :].expand(B, H, S),
                exact=out["exact"], rounded=out["rounded"])


# ---- embedding: (B, S, dim, V, P), starts (the same in every row) ----------
EMB_DOC_CASES = [((4, 48, 64, 64, 64), (0, 1, 20)),
                 ((3, 70, 32, 50, 128), (0, 69))]


@functools.lru_cache(maxsize=None)
def emb_doc_case(case):
    (B, S, E, V, P), st = case
    wte = N.randn_bf16(V, E, seed=700)
    wpe = N.randn_bf16(P, E, seed=701)
    dy = N.randn_bf16(B, S, E, seed=702)
    ids = torch.randint(0, V, (B, S),
                        generator=torch.Generator().manual_seed(703))
    doc_start = q_lo_of((st,) * B, S)
    pos = torch.arange(S)[None, :] - doc_start.long()          # [B, S]
    # forward as N.embedding models it: the fp32 sum, rounded to bf16 once
    y = N.bf16(N.d(wte)[ids] + N.d(wpe)[pos])
    flat = pos.reshape(-1)
    dwpe_exact = torch.zeros(P, E, dtype=N.F64).index_add_(
        0, flat, N.d(dy).reshape(-1, E))
    dwpe_f32 = torch.zeros(P, E, dtype=torch.float32).index_add_(
        0, flat, dy.float().reshape(-1, E)).to(N.F64)
    used = torch.zeros(P, dtype=torch.bool)
    used[flat] = True
    return dict(wte=wte, wpe=wpe, dy=dy, ids=ids, doc_start=doc_start, y=y,
                dwpe_exact=dwpe_exact, dwpe_f32=dwpe_f32, used=used)


# ---- the model-equivalence layout: three documents in one row of 16 --------
EQUIV_LENS = (5, 1, 10)


def equiv_batch(vocab, seed=0):
    """(ids [1,16], doc_start [1,16] int32, [(s0, s1)])."""
    S = sum(EQUIV_LENS)
    ids = torch.randint(0, vocab, (1, S),
                        generator=torch.Generator().manual_seed(seed))
    st, s0 = [], 0
    for n in EQUIV_LENS:
        st.append(s0)
        s0 += n
    return ids, q_lo_of((tuple(st),), S), doc_slices(tuple(st), S)
