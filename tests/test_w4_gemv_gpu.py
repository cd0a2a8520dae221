"""Int4 weight-only serving GEMM (hip/w4_gemv.hip) on the GPU: the kernel
against fp64 at the bounds the bf16 gemv is held to, the routes of ops.linear,
and graph-replayed decode on int4 models."""

import functools

import pytest
import torch

import _numerics as N
from distributedtraining_amd import ops
from distributedtraining_amd.config import ModelConfig
from distributedtraining_amd.models import (build_model, generate,
                                            quantize_for_serving)
from distributedtraining_amd.ops.backend import require_ext

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (M, N, K, nsplit). K: one group / a ragged turn of the 8-group register
# ring / 17 groups = three LDS stages with a ragged last one. N: 16 = one
# tile, 40 = padded tile in a partly empty block, 272 = several blocks and a
# ragged last one. nsplit 0 is the automatic split (K = 2176 gives two uneven
# slices of 9 and 8 groups). Then the paths it does not reach at these sizes:
# nsplit 1 = three stages in one block, nsplit 3 = slices of 6, 6 and 5
# groups, N 37 = the scalar stores of N % 4 != 0.
SHAPES = [(M, Nn, K, 0) for M in (1, 3, 16) for Nn in (16, 40, 272)
          for K in (128, 384, 2176)] + [
    (16, 40, 2176, 1), (3, 272, 2176, 3), (1, 37, 384, 0), (16, 37, 2176, 1)]
CASES = [(*s, b, r) for s in SHAPES for b in ("none", "bf16")
         for r in ("randn", "cancel")]


@functools.lru_cache(maxsize=None)
def _case(M, Nn, K, bias, regime):
    x, w, b = N.gemv_inputs(M, Nn, K, bias, regime)
    qw = ops.quantize_weight_int4(w)
    wq = N.d(ops.dequantize_weight(qw, torch.float32))   # float(q) * scale
    exact = N.d(x) @ wq.t()
    if b is not None:
        exact = exact + N.d(b)
    return x, b, qw, exact, N.bf16(exact)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_w4_gemv_accuracy(case):
    M, Nn, K, ns, bias, regime = case
    m = require_ext()
    x, b, qw, exact, rounded = _case(M, Nn, K, bias, regime)
    qd = qw.to(DEV)
    args = (x.to(DEV), qd.codes, qd.scales, None if b is None else b.to(DEV),
            Nn, ns)
    y = m.w4_gemv(*args)
    assert y.shape == (M, Nn) and y.dtype == torch.bfloat16
    N.check("w4_gemv", str(case), "y", y, exact, rounded)
    assert torch.equal(y, m.w4_gemv(*args))       # bit-repeatable


def test_linear_routes():
    m = require_ext()
    x, b, qw, _, _ = _case(16, 272, 2176, "bf16", "randn")
    qd, bd = qw.to(DEV), b.to(DEV)
    x16 = x.to(DEV)
    with torch.no_grad():
        y = ops.linear(x16.view(2, 8, -1), qd, bd)
        assert torch.equal(y.view(16, -1),
                           m.w4_gemv(x16, qd.codes, qd.scales, bd, 272))
        wd = m.w4_dequant(qd.codes, qd.scales, 272)
        assert torch.equal(wd.cpu(),
                           ops.dequantize_weight(qw, torch.bfloat16))
        x17 = torch.cat([x16, x16[:1]])
        assert torch.equal(ops.linear(x17, qd, bd), ops.linear(x17, wd, bd))
        assert torch.equal(ops.linear(x17, qd), ops.linear(x17, wd))


TINY = {
    "gpt2": ModelConfig(family="gpt2", vocab_size=512, n_layer=2, n_head=2,
                        n_embd=128, n_positions=64),
    "llama": ModelConfig(family="llama", vocab_size=512, n_layer=2, n_head=2,
                         n_kv_head=1, n_embd=128, n_positions=64,
                         intermediate_size=256, rope_theta=10000.0,
                         tie_word_embeddings=False),
}


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_int4_decode_replays_from_a_graph(family):
    """Greedy cached generation on an int4 model: the graph-replayed decode
    step (w4_gemv and its workspace captured) gives the tokens of the eager
    decode step."""
    torch.manual_seed(4)
    model = build_model(TINY[family]).to(DEV, torch.bfloat16).eval()
    st = quantize_for_serving(model, weights="int4")
    assert st["converted"] == (9 if family == "gpt2" else 15)
    ids = torch.randint(0, 512, (3, 10), device=DEV)
    graphed = generate(model, ids, max_new_tokens=24, use_cache=True)
    orig = model.new_cache
    model.new_cache = lambda *a, **kw: orig(*a, **{**kw, "graphable": False})
    eager = generate(model, ids, max_new_tokens=24, use_cache=True)
    model.new_cache = orig
    assert graphed.shape == (3, 34)
    assert torch.equal(graphed, eager)
