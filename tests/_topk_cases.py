"""Crafted inputs for the top-k delta tests (CPU and GPU files share them).

``crafted(P, block, k)`` is ``randn * 1e-3`` with, block by block as far as
there are blocks:

  block 0  a tie group: equal magnitudes 5.0 of both signs at offsets 5, 6,
           70, 300, 1029, 1029 + 257, ... (different lanes and, from 1029
           on, different waves of the compressor), above ``k - keep`` larger
           distinct values, so that exactly ``keep`` members (all but the
           last two) fit under the cut and index order must decide
  block 1  2k values 1 + j * 2^-23, j < 256, of both signs: their keys share
           the top 24 bits, only the last radix pass separates them, and
           values repeat, so the cut also falls inside a tie
  block 2  all zeros
  block 3  fewer than k non-zeros, among them one NaN, one +inf, a denormal
           and a -0.0
The last block is the ragged one whenever P is no multiple of ``block``.
"""

import functools
import struct

import torch

SHAPES = [(3 * 4096 + 37, 4096, 128), (1000, 4096, 128),
          (5 * 1024 + 1, 1024, 8), (2 * 8192, 8192, 2048)]
TIE = 5.0
DENORMAL = 1e-40


def tie_members(P, block):
    n0 = min(block, P)
    offs = [5, 6, 70, 300] + list(range(1029, n0, 257))
    return [o for o in offs if o < n0]


@functools.lru_cache(maxsize=None)
def crafted(P, block, k):
    """(x fp32 [P], info) — treat both as read-only."""
    g = torch.Generator().manual_seed(P * 31 + block + k)
    x = torch.randn(P, generator=g) * 1e-3
    nb = (P + block - 1) // block
    n0 = min(block, P)
    members = tie_members(P, block)
    keep = len(members) - 2
    n_big = k - keep
    assert keep >= 2 and n_big >= 1
    free = [o for o in torch.randperm(n0, generator=g).tolist()
            if o not in set(members)]
    big = sorted(free[:n_big])
    for r, o in enumerate(big):
        x[o] = (10.0 + r) * (-1.0 if r % 3 == 0 else 1.0)
    for r, o in enumerate(members):
        x[o] = TIE if r % 2 == 0 else -TIE
    info = {"members": members, "keep": keep, "big": big, "special": None}
    if nb > 1:
        n1 = min(block, P - block)
        pos = torch.randperm(n1, generator=g)[:min(2 * k, n1)] + block
        j = (torch.arange(pos.numel()) * 7) % 256
        one = torch.tensor(1.0).view(torch.int32)
        v = (one + j.to(torch.int32)).view(torch.float32)
        x[pos] = torch.where(torch.arange(pos.numel()) % 2 == 0, v, -v)
        info["near"] = sorted(pos.tolist())
    if nb > 2:
        x[2 * block:min(3 * block, P)] = 0.0
    if nb > 3:
        lo, hi = 3 * block, min(4 * block, P)
        x[lo:hi] = 0.0
        n3 = hi - lo
        assert n3 >= 8
        cnt = min(k // 2, n3 // 2)
        pos = torch.randperm(n3, generator=g)[:cnt] + lo
        x[pos[4:]] = torch.randn(cnt - 4, generator=g) * 1e-3
        x[pos[0]] = float("nan")
        x[pos[1]] = float("inf")
        x[pos[2]] = DENORMAL
        x[pos[3]] = -0.0
        info["special"] = {"nan": int(pos[0]), "inf": int(pos[1]),
                           "denormal": int(pos[2]), "negzero": int(pos[3]),
                           "nonzero": sorted(pos[4:].tolist()
                                             + pos[:3].tolist())}
    return x, info


@functools.lru_cache(maxsize=None)
def crafted_base_residual(P, block, k):
    """(base, residual) that leave the tie group of ``crafted`` a tie:
    base is a multiple of 0.25 (w = base + x is exact at the members) and
    the residual is 0 there."""
    g = torch.Generator().manual_seed(P + 7 * block + k)
    base = torch.randint(-8, 9, (P,), generator=g).to(torch.float32) * 0.25
    residual = torch.randn(P, generator=g) * 1e-4
    residual[tie_members(P, block)] = 0.0
    return base, residual


def entry_index(entries, k, block):
    """Global element index of every entry, [nb, k] int64."""
    ent = entries.view(-1, k)
    return (ent >> 16).to(torch.int64) + \
        torch.arange(ent.shape[0]).unsqueeze(1) * block


def hand_scatter(entries, k, block, P):
    """A row densified one entry at a time (the slow, obvious way)."""
    out = [0.0] * P
    for q, en in enumerate(entries.view(-1).tolist()):
        e = (q // k) * block + ((en >> 16) & 0xFFFF)
        if e < P:
            out[e] = struct.unpack(
                "<f", struct.pack("<I", (en & 0xFFFF) << 16))[0]
    return torch.tensor(out, dtype=torch.float32)
