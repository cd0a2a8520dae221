"""Shared cases of the robust-merge tests (test_robust_merge_cpu.py,
test_robust_merge_gpu.py): the (N, trim) lists, the special-value inputs and
a slow per-element reference of ops.trimmed_merge written in plain Python,
one element and one float at a time, with nothing in common with the torch
code of the CPU path but the definition.

Denormal INPUTS are left out of every set. The kernel orders and returns the
kept values by their bits and gfx950 code built by hipcc keeps fp32
denormals by default, as torch on the CPU does, but nothing in the build
pins either mode, so the bit-exact sets do not lean on it. Sums of the
normal inputs used here never land in the denormal range.
"""

import functools
import struct

import numpy as np
import torch

CANON_NAN = 0x7FC00000
KEY_NAN = 0xFFFFFFFF

N_CPU = (1, 2, 3, 4, 5, 8, 9, 32)
# each NP instantiation of the kernel full, and just past the previous one
N_GPU = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)


def trims(n):
    """Every legal trim among 0, 1 and the median's."""
    return sorted({t for t in (0, 1, (n - 1) // 2) if 2 * t < n})


def bits(t: torch.Tensor) -> torch.Tensor:
    """fp32 tensor -> its int32 bit patterns (what bit-exact compares)."""
    return t.detach().cpu().contiguous().view(torch.int32)


def special_deltas(n: int, P: int, seed: int = 0) -> torch.Tensor:
    """[n, P] fp32 with NaN, +-inf, +-0.0, exact ties across miners, an
    element where all miners agree, one that is all NaN, one that holds +inf
    and -inf, and (n >= 3) a whole-row outlier in the last row."""
    g = torch.Generator().manual_seed(1000 * n + P + seed)
    d = torch.randn(n, P, generator=g) * 0.02
    # scales spread over the columns, as parameter tensors differ
    d *= torch.logspace(-3, 3, P).roll(int(seed))
    col = torch.randperm(P, generator=g).tolist()

    def take(k):
        out = [col.pop() for _ in range(min(k, len(col)))]
        return out

    row = lambda: int(torch.randint(n, (1,), generator=g))   # noqa: E731
    for e in take(6):
        d[row(), e] = float("nan")
    for e in take(6):
        d[row(), e] = float("inf")
    for e in take(6):
        d[row(), e] = float("-inf")
    for e in take(6):
        d[row(), e] = 0.0
        d[row(), e] = -0.0
    for e in take(8):                     # ties: two or three miners agree
        v = d[row(), e].clone()
        d[row(), e] = v
        d[row(), e] = v
    for e in take(2):                     # everyone agrees
        d[:, e] = d[0, e].clone()
    for e in take(1):
        d[:, e] = float("nan")
    for e in take(2):                     # signed zeros only
        d[:, e] = 0.0
        d[::2, e] = -0.0
    for e in take(1):
        d[:, e] = -0.0
    if n >= 2:
        for e in take(2):
            d[0, e] = float("inf")
            d[n - 1, e] = float("-inf")
    if n >= 3:
        keep = d[n - 1].clone()
        d[n - 1] = 1e30
        # leave its NaN / inf in place
        bad = ~torch.isfinite(keep)
        d[n - 1][bad] = keep[bad]
    return d.contiguous()


def special_base(P: int, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(77 + P + seed)
    b = torch.randn(P, generator=g)
    if P > 4:
        b[1] = 0.0
        b[2] = -0.0
    return b


def _key(u: int) -> int:
    if (u & 0x7FFFFFFF) > 0x7F800000:
        return KEY_NAN
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u ^ 0x80000000)


def _unkey(k: int) -> int:
    if k == KEY_NAN:
        return CANON_NAN
    return (k ^ 0x80000000) if k & 0x80000000 else (~k & 0xFFFFFFFF)


def _f32(u: int) -> np.float32:
    return np.frombuffer(struct.pack("<I", u), dtype=np.float32)[0]


def reference(base: torch.Tensor, deltas: torch.Tensor, trim: int):
    """(out bits int32 [P], outside int64 [N]) of the definition, element by
    element in Python ints and numpy float32 scalars."""
    n, P = deltas.shape
    db = deltas.contiguous().view(torch.int32).numpy().astype(np.int64) \
        & 0xFFFFFFFF
    bb = base.contiguous().numpy()
    m = np.float32(n - 2 * trim)
    out = np.zeros(P, dtype=np.uint32)
    outside = [0] * n
    with np.errstate(all="ignore"):
        for e in range(P):
            keys = [_key(int(db[i, e])) for i in range(n)]
            srt = sorted(keys)
            kept = srt[trim:n - trim]
            s = _f32(_unkey(kept[0]))
            for k in kept[1:]:
                s = np.float32(s + _f32(_unkey(k)))
            o = np.float32(bb[e] + np.float32(s / m))
            out[e] = CANON_NAN if np.isnan(o) else \
                struct.unpack("<I", struct.pack("<f", o))[0]
            for i in range(n):
                if keys[i] < kept[0] or keys[i] > kept[-1]:
                    outside[i] += 1
    return (torch.from_numpy(out.view(np.int32).copy()),
            torch.tensor(outside, dtype=torch.int64))


@functools.lru_cache(maxsize=None)
def cpu_inputs(n: int, P: int):
    """(base, deltas) of the special-value set, made once per shape."""
    return special_base(P), special_deltas(n, P)
