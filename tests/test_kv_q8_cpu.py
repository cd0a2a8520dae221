"""Int8 KV cache on the CPU: the format (ops.kv_quantize / kv_dequantize), the
CPU decode path on codes + scales, and the option through generate."""

import pytest
import torch

from distributedtraining_amd import ops
from distributedtraining_amd.config import ModelConfig
from distributedtraining_amd.models import build_model, generate
from distributedtraining_amd.models.gpt2 import KVCache


def test_kv_quantize_format():
    torch.manual_seed(0)
    x = torch.randn(3, 5, 64).to(torch.bfloat16)
    x[1, 2] = 0
    codes, scale = ops.kv_quantize(x)
    assert codes.dtype == torch.int8 and scale.dtype == torch.float32
    assert codes.shape == x.shape and scale.shape == x.shape[:-1]
    assert scale[1, 2] == 1.0 and not codes[1, 2].any()
    assert int(codes.abs().max()) <= 127
    assert torch.equal(scale[0], x[0].float().abs().amax(-1) / 127.0)
    deq = ops.kv_dequantize(codes, scale, torch.float32)
    bound = scale[..., None] / 2 * (1 + 2.0 ** -23)
    assert bool(((x.float() - deq).abs() <= bound).all())
    # a representable row (integer codes times a power-of-two scale with the
    # amax at 127) goes through exactly
    q = torch.randint(-127, 128, (4, 64))
    q[:, 0] = 127
    rep = (q.float() * 0.25).to(torch.bfloat16)
    c2, s2 = ops.kv_quantize(rep)
    assert torch.equal(c2, q.to(torch.int8)) and bool((s2 == 0.25).all())
    assert torch.equal(ops.kv_dequantize(c2, s2), rep)


def test_cpu_decode_on_codes_matches_dequantised_caches():
    torch.manual_seed(1)
    B, H, Hk, L, D = 2, 8, 2, 37, 64
    q = torch.randn(B, H, D)
    kc, ks = ops.kv_quantize(torch.randn(B, Hk, L + 3, D))
    vc, vs = ops.kv_quantize(torch.randn(B, Hk, L + 3, D))
    o = ops.decode_attention(q, kc, vc, L, k_scale=ks, v_scale=vs)
    ref = ops.decode_attention(q, kc.float() * ks[..., None],
                               vc.float() * vs[..., None], L)
    torch.testing.assert_close(o, ref, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        ops.decode_attention(q, kc.float(), vc.float(), L, k_scale=ks,
                             v_scale=vs)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_generate_with_int8_cache(family):
    kw = (dict(n_kv_head=2, intermediate_size=64, rope_theta=10000.0,
               tie_word_embeddings=False) if family == "llama" else {})
    cfg = ModelConfig(family=family, vocab_size=97, n_layer=2, n_head=4,
                      n_embd=32, n_positions=32, **kw)
    torch.manual_seed(2)
    model = build_model(cfg).eval()
    ids = torch.randint(0, 97, (2, 6))
    ref = generate(model, ids, 5, use_cache=True)
    for seed in (None, 3):
        a = generate(model, ids, 5, use_cache=True, kv_cache="int8", seed=seed,
                     temperature=0.0)
        assert a.shape == ref.shape
        assert torch.equal(a[:, :7], ref[:, :7])   # prefill logits: unchanged
    cache = model.new_cache(2, 16, "cpu", kv_dtype="int8")
    model.prefill(ids, cache)
    assert cache.k[0].dtype == torch.int8 and cache.v[1].dtype == torch.int8
    assert cache.k_scale[0].shape[-1] == ops.kv_scale_len(16)
    k0, s0 = cache.k[0][:, :, :6], cache.k_scale[0][:, :, :6]
    assert bool(k0.any()) and bool((s0 != 1).any())
    with pytest.raises(ValueError):
        generate(model, ids, 2, use_cache=True, kv_cache="fp8")


def test_kvcache_rejects_other_formats():
    with pytest.raises(ValueError):
        KVCache(1, 1, 1, 8, 64, "cpu", kv_dtype="fp8")


def test_int8_split_rule():
    """clamp(ceil(2 CUs / (B Hk)), 1, Lmax / 512); never 0; contract errors."""
    plan = ops.decode_split_plan_q8
    assert [plan(B, 32, 8, 8192, 128) for B in (1, 16, 64)] == [16, 4, 1]
    assert plan(16, 28, 4, 8192, 128) == 8 and plan(1, 12, 12, 100, 64) == 1
    for bad in ((1, 32, 1, 512, 64), (1, 8, 8, 512, 32)):
        with pytest.raises(ValueError):
            plan(*bad)
