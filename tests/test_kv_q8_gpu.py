"""Int8 KV cache on the GPU: the quantising append (kv_append_q8_k) against
ops.kv_quantize bit for bit, the int8 split-KV decode kernel
(attn_decode_split_q8_k) against fp64, and graph-replayed decode.

Rounding points modelled in ``_rounded``: the walk of
test_decode_split_gpu.py (wave w of split s takes tiles w, w + 4, ... of its
chunk, m_run after the current 32-key tile) with bf16(p * v_scale[key]) in
place of bf16(p) and the integer codes in place of V. The K scale, l (the
unrounded, unscaled p), all partials and 1/l are fp32 in the kernel and exact
here; o is rounded once.
"""

import math

import pytest
import torch

import _numerics as N
from distributedtraining_amd import ops
from distributedtraining_amd.config import ModelConfig
from distributedtraining_amd.models import build_model
from distributedtraining_amd.models.generate import GraphedDecoder

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOG2E = 1.4426950408889634


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("B,Hk", [(2, 1), (3, 4)])
@pytest.mark.parametrize("D", [64, 128])
def test_append_equals_kv_quantize(D, B, Hk, S):
    Lmax, pos, F = 50, 37, Hk * D
    g = torch.Generator().manual_seed(D + B + S)
    qkv = torch.randn(B, S, 3 * F, generator=g).to(torch.bfloat16)
    kn = qkv[..., F:2 * F].view(B, S, Hk, D)
    vn = qkv[..., 2 * F:].view(B, S, Hk, D)
    kn[0, 0, 0] = 0                    # a zero row
    vn[-1, -1, -1] = 0                 # a row whose amax is its only element
    vn[-1, -1, -1, 3] = -1.5
    qkv = qkv.to(DEV)
    kn = qkv[..., F:2 * F].view(B, S, Hk, D)     # strided slices, in place
    vn = qkv[..., 2 * F:].view(B, S, Hk, D)
    Lp = ops.kv_scale_len(Lmax)
    kc = torch.full((B, Hk, Lmax, D), 77, dtype=torch.int8, device=DEV)
    vc = torch.full_like(kc, -77)
    ks = torch.full((B, Hk, Lp), 5.0, device=DEV)
    vs = torch.full_like(ks, 6.0)
    before = [t.clone() for t in (kc, ks, vc, vs)]
    p = (torch.tensor([pos], dtype=torch.int32, device=DEV) if S == 1 else pos)
    ops.kv_append_q8(kn, vn, kc, ks, vc, vs, p)
    for new, codes, scale, c0, s0 in ((kn, kc, ks, before[0], before[1]),
                                      (vn, vc, vs, before[2], before[3])):
        q, s = ops.kv_quantize(new.cpu().transpose(1, 2))
        assert torch.equal(codes[:, :, pos:pos + S].cpu(), q)
        assert torch.equal(scale[:, :, pos:pos + S].cpu(), s)
        c0[:, :, pos:pos + S] = codes[:, :, pos:pos + S]
        s0[:, :, pos:pos + S] = scale[:, :, pos:pos + S]
        assert torch.equal(codes, c0) and torch.equal(scale, s0)


# (L, split_kv, H, Hk, D), B = 2, cache capacity L + 7
CASES = [(1, 1, 4, 4, 64), (31, 3, 16, 1, 64), (32, 1, 8, 2, 128),
         (33, 3, 8, 2, 64), (33, 1, 7, 1, 128), (257, 1, 16, 1, 64),
         (257, 3, 8, 2, 128), (257, 3, 4, 4, 64)]


def _case(L, H, Hk, D):
    """bf16 randn rows with per-row power-of-two factors of periods 5 (K) and
    7 (V): the scales differ from key to key and between K and V."""
    Lmax = L + 7
    j = torch.arange(Lmax)
    q = N.randn_bf16(2, H, D, seed=700)
    k = N.randn_bf16(2, Hk, Lmax, D, seed=701).float()
    v = N.randn_bf16(2, Hk, Lmax, D, seed=702).float()
    k = (k * (2.0 ** ((3 * j) % 5 - 2))[:, None]).to(torch.bfloat16)
    v = (v * (2.0 ** ((5 * j) % 7 - 3))[:, None]).to(torch.bfloat16)
    kc, ks = ops.kv_quantize(k)
    vc, vs = ops.kv_quantize(v)
    pad = ops.kv_scale_len(Lmax) - Lmax
    ks, vs = (torch.nn.functional.pad(t, (0, pad), value=float("nan"))
              for t in (ks, vs))
    return q, kc, ks, vc, vs


def _rounded(q, kc, ks, vc, vs, L, scale, nsplit):
    B, H, D = q.shape
    Hk, Lmax = kc.shape[1], kc.shape[2]
    head = torch.arange(H) // (H // Hk)
    s = torch.einsum("bhd,bhkd->bhk", q, kc[:, head, :L]) \
        * ks[:, head, :L] * scale * LOG2E
    v, vsc = vc[:, head, :L], vs[:, head, :L]
    chunk = 32 * -(-Lmax // (32 * nsplit))
    M = s.amax(-1, keepdim=True)
    num = torch.zeros(B, H, D, dtype=N.F64)
    den = torch.zeros(B, H, 1, dtype=N.F64)
    for s0 in range(0, L, chunk):
        for w in range(4):
            m_run = torch.full((B, H, 1), -float("inf"), dtype=N.F64)
            for k0 in range(s0 + 32 * w, min(L, s0 + chunk), 128):
                k1 = min(L, k0 + 32)
                st = s[..., k0:k1]
                m_run = torch.maximum(m_run, st.amax(-1, keepdim=True))
                p = torch.exp2(st - m_run)
                r = torch.exp2(m_run - M)
                num += r * torch.einsum("bhk,bhkd->bhd",
                                        N.bf16(p * vsc[..., k0:k1]),
                                        v[:, :, k0:k1])
                den += r * p.sum(-1, keepdim=True)
    return N.bf16(num / den)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_decode_q8_accuracy(case):
    L, nsplit, H, Hk, D = case
    q, kc, ks, vc, vs = _case(L, H, Hk, D)
    scale = 1.0 / math.sqrt(D)
    dk = N.d(kc) * N.d(ks)[..., :kc.shape[2], None]     # codes * scale, fp64
    dv = N.d(vc) * N.d(vs)[..., :kc.shape[2], None]
    exact = N.decode_attention(N.d(q), dk, dv, L, scale)
    rounded = _rounded(N.d(q), N.d(kc), N.d(ks), N.d(vc), N.d(vs), L, scale,
                       nsplit)
    g = [t.to(DEV) for t in (q, kc, vc)]
    kw = dict(k_scale=ks.to(DEV), v_scale=vs.to(DEV), split_kv=nsplit)
    o = ops.decode_attention(*g, L, scale, **kw)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    N.check("attn_decode_split_q8", str(case), "o", o, exact, rounded)
    # bit-repeatable, and the device-length path is the same computation
    assert torch.equal(o, ops.decode_attention(*g, L, scale, **kw))
    pos = torch.tensor([L - 1], dtype=torch.int32, device=DEV)
    assert torch.equal(o, ops.decode_attention(*g, 0, scale, kv_len_dev=pos,
                                               **kw))


def test_int8_cache_replays_from_a_graph():
    """8 greedy tokens through GraphedDecoder on an int8, split_kv=2 cache
    equal the eager decode_step loop on a second such cache."""
    cfg = ModelConfig(family="llama", vocab_size=512, n_layer=2, n_head=4,
                      n_kv_head=2, n_embd=256, n_positions=64,
                      intermediate_size=512, rope_theta=10000.0,
                      tie_word_embeddings=False)
    torch.manual_seed(6)
    model = build_model(cfg).to(DEV, torch.bfloat16).eval()
    ids = torch.randint(0, 512, (2, 40), device=DEV)
    toks = {}
    with torch.no_grad():
        for graphed in (True, False):
            cache = model.new_cache(2, 64, DEV, graphable=graphed, split_kv=2,
                                    kv_dtype="int8")
            assert cache.k[0].dtype == torch.int8
            tok = model.prefill(ids, cache).argmax(-1, keepdim=True)
            step = (GraphedDecoder(model, cache, 2, DEV).step if graphed
                    else lambda t: model.decode_step(t, cache))
            out = [tok]
            for _ in range(8):
                out.append(step(out[-1]).argmax(-1, keepdim=True))
            toks[graphed] = torch.cat(out, 1)
    assert torch.equal(toks[True], toks[False])


def test_int8_route_errors():
    q = torch.zeros(1, 32, 64, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(1, 1, 32, 64, dtype=torch.int8, device=DEV)
    sc = torch.ones(1, 1, 32, device=DEV)
    with pytest.raises(ValueError):        # grp = 32
        ops.decode_attention(q, kc, kc, 8, k_scale=sc, v_scale=sc, split_kv=1)
    with pytest.raises(ValueError):        # no one-block-per-head route
        ops.decode_attention(q[:, :4], kc, kc, 8, k_scale=sc, v_scale=sc,
                             split_kv=0)
