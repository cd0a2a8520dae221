"""Token sampling: the definition (CPU, fp64) and the dispatch to the fused
gfx950 kernel (hip/sample.hip).

One row of logits gives one token:

* NaN counts as -inf. ``temperature <= 0``, or a row maximum that is not
  finite, takes the greedy rule: the lowest index of the maximum (an all -inf
  row gives 0).
* ``0 < top_k < V`` keeps the logits ``>=`` the k-th largest value, ties at
  that value included (as ``generate._sample``).
* weights ``w = exp2((l - max) * log2e / temperature)`` over what top-k kept.
* ``0 < top_p < 1`` keeps a value ``v`` iff the mass strictly above it,
  ``above(v)``, is ``<= top_p * W``: the smallest set of top values whose
  mass exceeds ``top_p``. Equal logits are kept or dropped together;
  ``_sample`` cuts inside a run of equal logits by sort position.
* the draw is ``u = h / 2^64``, ``h = droprng.sample_hash(counter, row)``,
  from the counter chain rather than a ``torch.Generator``; the token is the
  lowest index whose inclusive prefix sum of kept weights, in index order,
  exceeds ``u * W'``.

The kernel computes the same thing on 16-bit keys and 2^-40 fixed-point
weights; where ``u`` falls within ~2e-5 of a boundary of the CDF the two may
pick neighbouring tokens (tests/test_sample_gpu.py).
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import droprng
from .backend import require_ext, use_hip

LOG2E = 1.4426950408889634


def sample_cdf(row, temperature: float, top_k: int = 0,
               top_p: float = 0.0) -> Tuple[np.ndarray, float]:
    """-> (cdf, gap). ``cdf`` fp64 [V]: the normalised inclusive prefix sums,
    in index order, of the kept weights of one row of logits (a step at the
    greedy token where the greedy rule applies); the token of a draw ``u`` is
    ``searchsorted(cdf, u, "right")``. ``gap``: how far ``top_p`` lies from
    ``above(v) / W`` of the two values around the nucleus boundary (inf
    without top-p)."""
    x = np.asarray(torch.as_tensor(row).detach().to(torch.float64).cpu()
                   .numpy(), dtype=np.float64).copy()
    x[np.isnan(x)] = -np.inf
    V = x.shape[0]
    m = x.max()
    if temperature <= 0 or not np.isfinite(m):
        cdf = np.zeros(V)
        cdf[int(np.argmax(x)):] = 1.0
        return cdf, math.inf
    keep = np.ones(V, dtype=bool)
    if 0 < top_k < V:
        keep = x >= np.partition(x, V - top_k)[V - top_k]
    w = np.where(keep, np.exp2((x - m) * (LOG2E / temperature)), 0.0)
    gap = math.inf
    if 0.0 < top_p < 1.0:
        order = np.argsort(-x, kind="stable")
        xs, ws = x[order], w[order]
        excl = np.cumsum(ws) - ws
        above = excl[np.searchsorted(-xs, -xs, side="left")] / ws.sum()
        cut = above > top_p
        w[order[cut]] = 0.0
        gap = float(np.abs(above[ws > 0] - top_p).min())
    cdf = np.cumsum(w)
    return cdf / cdf[-1], gap


def _sample_cpu(logits, temperature, top_k, top_p, ctr: int) -> torch.Tensor:
    u = droprng.sample_uniform(ctr, logits.shape[0])
    out = [int(np.searchsorted(
        sample_cdf(logits[b], temperature, top_k, top_p)[0], u[b], "right"))
        for b in range(logits.shape[0])]
    return torch.tensor(out, dtype=torch.long, device=logits.device)


def sample_tokens(logits: torch.Tensor, temperature: float, top_k: int,
                  top_p: float, counter, *,
                  done: Optional[torch.Tensor] = None,
                  eos: Optional[int] = None,
                  tok: Optional[torch.Tensor] = None,
                  ids: Optional[torch.Tensor] = None,
                  pos=None) -> torch.Tensor:
    """One token per row of ``logits`` [B, V] -> int64 [B] (``tok`` itself,
    [B] or [B, 1], when given). ``counter``: the int64 [1] counter of the
    draw (an int on the CPU also works); it is read, not advanced.

    Bookkeeping of a generation loop, all optional: ``done`` (bool [B]) with
    ``eos``: a done row emits ``eos`` and ``done |= token == eos``; ``ids``
    (int64 [B, total]) with ``pos`` (int, or the int32 [1] device position of
    a graphable KV cache): the token is stored in column
    ``min(pos, total - 1)``.

    GPU: one launch of hip/sample.hip, bf16 logits only (the decode heads'
    dtype), no host sync, capturable when ``pos`` is a tensor. CPU: the fp64
    definition of this module."""
    if (done is None) != (eos is None):
        raise ValueError("done and eos go together")
    if (ids is None) != (pos is None):
        raise ValueError("ids and pos go together")
    if use_hip(logits):
        if logits.dtype != torch.bfloat16:
            raise TypeError("sample_tokens on the GPU takes bf16 logits")
        if ids is not None and not torch.is_tensor(pos):
            pos = torch.full((1,), int(pos), dtype=torch.int32,
                             device=logits.device)
        return require_ext().sample_tokens(
            logits, float(temperature), int(top_k), float(top_p), counter,
            done, -1 if eos is None else int(eos), tok, ids, pos)
    t = _sample_cpu(logits, temperature, top_k, top_p, int(counter))
    if done is not None:
        t = torch.where(done, torch.full_like(t, eos), t)
        done |= t == eos
    if ids is not None:
        ids[:, max(0, min(int(pos), ids.shape[1] - 1))] = t
    if tok is not None:
        tok.copy_(t.view_as(tok))
        return tok
    return t
