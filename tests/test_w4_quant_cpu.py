"""Int4 weight-only serving format on the CPU: the quantiser against its
definition, the packing against its inverse, and the model wiring."""

import pytest
import torch
import torch.nn.functional as F

from distributedtraining_amd import ops
from distributedtraining_amd.config import ModelConfig
from distributedtraining_amd.models import (build_model, generate,
                                            quantize_for_serving)
from distributedtraining_amd.ops.w8 import unpack_weight

G = 128


def _weight(N, K, dtype):
    g = torch.Generator().manual_seed(N * 7 + K)
    w = (torch.randn(N, K, generator=g) * 0.05).to(dtype)
    w[N // 2, K - G:] = 0          # one all-zero group
    return w


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("N,K", [(16, 128), (40, 384), (272, 1024)])
def test_quantiser_matches_its_definition(N, K, dtype):
    w = _weight(N, K, dtype)
    qw = ops.quantize_weight_int4(w)
    tiles = (N + 15) // 16
    assert qw.bits == 4 and qw.shape == (N, K)
    assert qw.codes.dtype == torch.uint8
    assert qw.codes.shape == (tiles, K // G, 64, 16)
    assert qw.scales.shape == (tiles, K // G, 16)
    assert qw.nbytes() == tiles * 16 * K // 2 + tiles * 16 * (K // G) * 4
    assert qw.to("cpu").bits == 4
    q, s = unpack_weight(qw)
    # the definition, computed directly
    wg = w.float().view(N, K // G, G)
    scale = wg.abs().amax(-1) / 7
    scale[scale == 0] = 1.0
    codes = torch.clamp(torch.round(wg / scale[..., None]), -7, 7)
    assert torch.equal(s, scale) and s[N // 2, -1] == 1.0
    assert torch.equal(q, codes.to(torch.int8).view(N, K))
    assert int(q.abs().max()) <= 7
    # the stored nibbles: column 8 d + e of lane (row 0, quarter 0) of tile 0,
    # group 0 sits in dword d at nibble e / 2 + 4 (e % 2); none is 0
    dw = qw.codes[0, 0, 0].view(4, 4).to(torch.int64)
    dw = dw[:, 0] | dw[:, 1] << 8 | dw[:, 2] << 16 | dw[:, 3] << 24
    for col in range(32):
        d, e = divmod(col, 8)
        assert int(dw[d] >> 4 * (e // 2 + 4 * (e % 2)) & 15) == q[0, col] + 8
    assert int((qw.codes & 15).min()) >= 1 and int((qw.codes >> 4).min()) >= 1
    # padded rows hold the zero code
    pad = qw.codes.view(tiles, K // G, 4, 16, 16)[-1, :, :, N % 16 or 16:]
    assert bool((pad == 0x88).all())
    rep = q.double().view(N, K // G, G) * s.double()[..., None]
    # half a step, plus the two fp32 roundings the definition contains (the
    # scale and the quotient, 2^-24 |w| each): an exact tie of w / scale can
    # fall either way
    slack = wg.double().abs() * 2.0 ** -23
    assert bool(((wg.double() - rep).abs()
                 <= s.double()[..., None] / 2 + slack).all())
    for dt in (torch.bfloat16, torch.float32):
        deq = ops.dequantize_weight(qw, dt)
        assert deq.shape == (N, K) and deq.dtype == dt
        want = (q.float().view(N, K // G, G) * s[..., None]).view(N, K).to(dt)
        assert torch.equal(deq, want)
    # bf16: the same bound plus the rounding of the represented weight, half
    # an ulp of 8 significand bits: at most 2^-8 |rep|
    deq = ops.dequantize_weight(qw, torch.bfloat16).double().view(N, K // G, G)
    assert bool(((wg.double() - deq).abs()
                 <= s.double()[..., None] / 2 + slack
                 + rep.abs() * 2.0 ** -8).all())


def test_linear_on_cpu_is_linear_on_the_dequantised_weight():
    w = _weight(40, 384, torch.float32)
    qw = ops.quantize_weight_int4(w)
    x = torch.randn(3, 5, 384)
    b = torch.randn(40)
    want = F.linear(x, ops.dequantize_weight(qw, torch.float32), b)
    assert torch.equal(ops.linear(x, qw, b), want)
    assert torch.equal(ops.linear(x, qw),
                       F.linear(x, ops.dequantize_weight(qw, torch.float32)))
    with pytest.raises(RuntimeError):        # inference only
        ops.linear(x.requires_grad_(), qw, b)


def test_rejects_bad_weights():
    with pytest.raises(ValueError):
        ops.quantize_weight_int4(torch.randn(16, 192))
    w = torch.randn(16, 128)
    w[3, 5] = float("inf")
    with pytest.raises(ValueError):
        ops.quantize_weight_int4(w)
    w[3, 5] = float("nan")
    with pytest.raises(ValueError):
        ops.quantize_weight_int4(w)


# the two tiny configs of tests/test_w8_gemv_gpu.py
TINY = {
    "gpt2": ModelConfig(family="gpt2", vocab_size=512, n_layer=2, n_head=2,
                        n_embd=128, n_positions=64),
    "llama": ModelConfig(family="llama", vocab_size=512, n_layer=2, n_head=2,
                         n_kv_head=1, n_embd=128, n_positions=64,
                         intermediate_size=256, rope_theta=10000.0,
                         tie_word_embeddings=False),
}


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_quantise_for_serving_int4(family):
    torch.manual_seed(0)
    model = build_model(TINY[family]).eval()
    torch.manual_seed(0)
    model8 = build_model(TINY[family]).eval()
    st = quantize_for_serving(model, weights="int4")
    st8 = quantize_for_serving(model8, weights="int8")
    assert st["converted"] == st8["converted"] == \
        (9 if family == "gpt2" else 15)
    assert st["kept"] == 0 and st["bytes_before"] == st8["bytes_before"]
    assert st["bytes_after"] < st8["bytes_after"] < st["bytes_before"]
    blk = model.blocks[0]
    w0 = blk.attn_qkv_w if family == "gpt2" else blk.down_w
    assert isinstance(w0, ops.QuantWeight) and w0.bits == 4
    assert model.head_q.bits == 4
    with pytest.raises(ValueError):
        quantize_for_serving(model8, weights="int2")
    ids = torch.randint(0, 512, (2, 9))
    out = generate(model, ids, max_new_tokens=4, use_cache=True)
    assert out.shape == (2, 13) and torch.equal(out[:, :9], ids)
