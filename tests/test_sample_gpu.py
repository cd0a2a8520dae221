"""Fused token sampler (hip/sample.hip) on the GPU against its fp64
definition (ops/sampling.py), its conventions, and seeded generation through
the decode graph."""

import functools
import math

import numpy as np
import pytest
import torch

from distributedtraining_amd import ops
from distributedtraining_amd.models import build_model, generate
from distributedtraining_amd.ops import droprng
from test_w8_gemv_gpu import TINY

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS, CTRS, MARGIN = 256, (3, 4), 1e-4
SETTINGS = [(1.0, 0, 0.0), (0.7, 8, 0.0), (0.8, 0, 0.9), (1.3, 50, 0.75),
            (1.0, 1, 0.0)]


@functools.lru_cache(maxsize=None)
def _row(V, regime):
    """3 * randn in bf16 (ties at 50k); "special" adds a -inf block, a NaN
    and a plateau of up to 64 equal maxima on odd indices (lowest: 1)."""
    g = torch.Generator().manual_seed(V)
    row = (3 * torch.randn(V, generator=g)).bfloat16()
    if regime == "special":
        row[V // 4:V // 2] = float("-inf")
        row[4] = float("nan")
        row[1:2 * min(64, V // 2):2] = 16.0
    return row


def _ctr(c):
    return torch.full((1,), c, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("regime", ["randn", "special"])
@pytest.mark.parametrize("setting", SETTINGS, ids=str)
@pytest.mark.parametrize("V", [37, 1000, 50257, 151936])
def test_tokens_match_definition(V, setting, regime):
    """256 rows of one logits row are 256 draws; two counters give 512. A
    draw u is ambiguous, and only then left out, if it lies within 1e-4 of
    the reference CDF boundary on either side of it: the kernel's fp32
    exponent argument is good to ~1e-5 for kept weights (exponents in
    [-40, 0]), so w to ~7e-6 relative, v_exp_f32 adds ~1 ulp, the 2^-40
    fixed point at most V * 2^-41: below 2e-5 in all, the margin is 5 x that.
    Every other draw matches exactly, an ambiguous one still lands on a kept
    token, and a second launch repeats the first bit for bit.

    Left-out draws: 2 of 512 are allowed where every kept token is wider than
    the margin (expectation 512 * 2e-4 = 0.1, so 2 is that + 6 sigma). With
    narrower tokens no choice of data meets 2: the reference alone leaves out
    162 of 512 at V = 50257 and 247 at V = 151936 without a filter (3 * randn
    puts a third of the mass on tokens below 2e-4). There the same rule is
    applied to the reference's own expectation, E = 512 * sum_i min(p_i,
    2e-4): at most max(2, floor(E + 6 sqrt(E)))."""
    T, k, p = setting
    row = _row(V, regime)
    cdf, gap = ops.sample_cdf(row, T, k, p)
    assert gap > MARGIN          # the nucleus itself is not in doubt
    pr = np.diff(cdf, prepend=0.0)
    logits = row.to(DEV).repeat(ROWS, 1)
    left = 0
    for c in CTRS:
        got = ops.sample_tokens(logits, T, k, p, _ctr(c))
        assert torch.equal(got, ops.sample_tokens(logits, T, k, p, _ctr(c)))
        got = got.cpu().numpy()
        u = droprng.sample_uniform(c, ROWS)
        want = np.searchsorted(cdf, u, "right")
        lo = np.where(want > 0, cdf[np.maximum(want - 1, 0)], 0.0)
        amb = (u - lo < MARGIN) | (cdf[want] - u < MARGIN)
        left += int(amb.sum())
        assert (got[~amb] == want[~amb]).all(), (got[~amb] != want[~amb]).sum()
        assert (pr[got] > 0).all()
    cpu = ops.sample_tokens(row[None].expand(2, V), T, k, p, CTRS[-1])
    assert cpu.tolist() == want[:2].tolist()
    E = 512 * float(np.minimum(pr[pr > 0], 2 * MARGIN).sum())
    print(f"V={V} {setting} {regime}: left out {left}, E={E:.2f}, gap={gap:.2e}")
    assert left <= max(2, math.floor(E + 6 * math.sqrt(E)))


def test_conventions():
    row = _row(1000, "special")
    logits = torch.stack([row, torch.full_like(row, float("-inf")),
                          _row(1000, "randn")]).to(DEV)
    greedy = ops.sample_tokens(logits, 0.0, 0, 0.0, _ctr(0))
    assert greedy.tolist() == [1, 0, int(_row(1000, "randn").float().argmax())]
    for T in (0.5, 2.0):         # top_k = 1 on a row with a single maximum
        assert ops.sample_tokens(logits[2:], T, 1, 0.0, _ctr(1)).tolist() \
            == greedy[2:].tolist()
    # done / eos: row 0 is done already, row 1 can only draw eos (7)
    sure = torch.full((3, 40), -30.0, dtype=torch.bfloat16, device=DEV)
    sure[:, 7] = 30.0
    sure[2, 7], sure[2, 9] = -30.0, 30.0
    done = torch.tensor([True, False, False], device=DEV)
    tok = torch.zeros(3, 1, dtype=torch.long, device=DEV)
    ids = torch.zeros(3, 5, dtype=torch.long, device=DEV)
    pos = torch.tensor([2], dtype=torch.int32, device=DEV)
    out = ops.sample_tokens(sure, 1.0, 0, 0.0, _ctr(2), done=done, eos=7,
                            tok=tok, ids=ids, pos=pos)
    assert out is tok and tok.view(-1).tolist() == [7, 7, 9]
    assert done.tolist() == [True, True, False]
    assert ids[:, 2].tolist() == [7, 7, 9] and int(ids.sum()) == 23
    ops.sample_tokens(sure, 1.0, 0, 0.0, _ctr(2), ids=ids, pos=pos + 7)
    assert ids[:, 4].tolist() == [7, 7, 9] and int(ids.sum()) == 46


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_seeded_generation_replays_from_a_graph(family):
    torch.manual_seed(4)
    model = build_model(TINY[family]).to(DEV, torch.bfloat16).eval()
    ids = torch.randint(0, 512, (3, 10), device=DEV)
    kw = dict(max_new_tokens=24, use_cache=True)
    skw = dict(temperature=0.8, top_k=20, top_p=0.9, **kw)
    graphed = generate(model, ids, seed=3, **skw)
    assert graphed.shape == (3, 34)
    assert torch.equal(graphed, generate(model, ids, seed=3, **skw))
    assert not torch.equal(graphed, generate(model, ids, seed=5, **skw))
    for rows in (ids, ids[:1]):  # one row: stops mid-way, the poll and trim
        eos = int(generate(model, rows, **kw)[0, 20])
        want = generate(model, rows, eos_token_id=eos, **kw)
        assert torch.equal(
            generate(model, rows, eos_token_id=eos, seed=0, **kw), want)
    assert want.shape[1] <= 21
    orig = model.new_cache
    model.new_cache = lambda *a, **k: orig(*a, **{**k, "graphable": False})
    eager = generate(model, ids, seed=3, **skw)
    model.new_cache = orig
    assert torch.equal(graphed, eager)
