"""ops.extend_attention's CPU composition (the definition of the op) and
chunked prefill through ``generate`` on fp32 CPU models."""

import math

import pytest
import torch

from distributedtraining_amd import ops
from distributedtraining_amd.config import ModelConfig
from distributedtraining_amd.models import build_model, generate


def test_extend_attention_cpu_matches_sdpa():
    B, H, Hk, P, Sq, D = 2, 4, 2, 5, 3, 16
    torch.manual_seed(1)
    q = torch.randn(B, H, Sq, D)
    k = torch.randn(B, Hk, P + Sq + 2, D)      # 2 rows past the valid range
    v = torch.randn(B, Hk, P + Sq + 2, D)
    mask = torch.arange(P + Sq)[None, :] <= P + torch.arange(Sq)[:, None]

    def sdpa(kk, vv):
        return torch.nn.functional.scaled_dot_product_attention(
            q, kk[:, :, :P + Sq], vv[:, :, :P + Sq], attn_mask=mask,
            scale=1.0 / math.sqrt(D), enable_gqa=True).transpose(1, 2)
    out = ops.extend_attention(q, k, v, P)
    assert out.shape == (B, Sq, H, D)
    torch.testing.assert_close(out, sdpa(k, v), rtol=1e-5, atol=1e-5)
    # int8 caches: the same call on the dequantised caches
    (kq, ks), (vq, vs) = ops.kv_quantize(k), ops.kv_quantize(v)
    out8 = ops.extend_attention(q, kq, vq, P, k_scale=ks, v_scale=vs)
    torch.testing.assert_close(
        out8, sdpa(kq.float() * ks[..., None], vq.float() * vs[..., None]),
        rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        ops.extend_attention(q, k, v, P + 3)     # past the cache capacity


CFGS = {
    "gpt2": ModelConfig.gpt2_tiny(),
    "llama": ModelConfig(family="llama", vocab_size=256, n_layer=2, n_head=4,
                         n_kv_head=2, n_embd=64, n_positions=64,
                         intermediate_size=128, rope_theta=10000.0,
                         tie_word_embeddings=False),
}


@pytest.mark.parametrize("seed", [None, 3])
@pytest.mark.parametrize("family", sorted(CFGS))
def test_chunked_prefill_generates_the_same_tokens(family, seed):
    cfg = CFGS[family]
    torch.manual_seed(2)
    model = build_model(cfg)
    ids = torch.randint(0, cfg.vocab_size, (2, 7))
    kw = dict(max_new_tokens=6, use_cache=True, seed=seed,
              temperature=0.0 if seed is None else 0.8)
    ref = generate(model, ids, prefill_chunk=0, **kw)
    assert torch.equal(generate(model, ids, prefill_chunk=3, **kw), ref)
    with pytest.raises(ValueError):
        generate(model, ids, prefill_chunk=-1, **kw)
