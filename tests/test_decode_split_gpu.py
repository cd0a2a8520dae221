"""Split-KV decode attention (attn_decode_split_k + attn_decode_combine_k in
hip/attention.hip) on the GPU: the kernel against fp64, and graph-replayed
decode through a cache that selects the route.

Rounding points modelled in ``_rounded`` (the new kernel's, not
attn_decode_k's):
  * P before P.V: exp2(s - m_run) is packed to bf16, with m_run the running
    max of the wave's tile sequence after the CURRENT 32-key tile. Wave w of
    split s walks tiles w, w + 4, ... of the keys [s * chunk, (s + 1) * chunk),
    chunk = 32 * ceil(Lmax / (32 * nsplit)).
  * l sums the UNROUNDED fp32 p.
  * the accumulator rescales, the wave and split partials (m, l, acc) and
    1/l stay fp32: exact in the fp64 model.
  * o: rounded to bf16 once, after the last merge.
"""

import pytest
import torch

import _numerics as N
from distributedtraining_amd import ops
from distributedtraining_amd.config import ModelConfig
from distributedtraining_amd.models import build_model
from distributedtraining_amd.models.generate import GraphedDecoder

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOG2E = 1.4426950408889634     # the kernel works in exp2 units

# (L, split_kv, H, Hk, D, regime), B = 2, cache capacity L + 7.
# L = 33 x 3 splits: a full tile, a one-key tile and an empty split. L = 257:
# 1 split gives wave 0 three tiles (the look-ahead loads), 3 splits leave
# wave 3 idle; rising moves the max into the last split. grp 1, 4, 7, 16.
CASES = [
    (1, 1, 4, 4, 64, "diffuse"), (1, 3, 8, 2, 128, "diffuse"),
    (31, 1, 7, 1, 64, "diffuse"), (31, 3, 16, 1, 64, "rising"),
    (32, 3, 4, 4, 128, "diffuse"), (32, 1, 8, 2, 64, "diffuse"),
    (33, 3, 8, 2, 64, "diffuse"), (33, 3, 16, 1, 128, "rising"),
    (33, 1, 7, 1, 128, "rising"), (257, 3, 4, 4, 64, "rising"),
    (257, 3, 8, 2, 128, "rising"), (257, 1, 16, 1, 64, "diffuse"),
    (257, 3, 7, 1, 128, "diffuse"), (257, 1, 8, 2, 128, "rising"),
]


def _rounded(q, kc, vc, L, scale, nsplit):
    B, H, D = q.shape
    Hk, Lmax = kc.shape[1], kc.shape[2]
    head = torch.arange(H) // (H // Hk)
    s = torch.einsum("bhd,bhkd->bhk", q, kc[:, head, :L]) * scale * LOG2E
    v = vc[:, head, :L]
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
                num += r * torch.einsum("bhk,bhkd->bhd", N.bf16(p),
                                        v[:, :, k0:k1])
                den += r * p.sum(-1, keepdim=True)
    return N.bf16(num / den)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_decode_split_accuracy(case):
    L, nsplit, H, Hk, D, regime = case
    c = N.decode_case((2, H, Hk, L, D, regime))
    q, kc, vc = (c[k].to(DEV) for k in ("q", "kc", "vc"))
    o = ops.decode_attention(q, kc, vc, L, c["scale"], split_kv=nsplit)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    rounded = _rounded(N.d(c["q"]), N.d(c["kc"]), N.d(c["vc"]), L, c["scale"],
                       nsplit)
    N.check("attn_decode_split", str(case), "o", o, c["exact"], rounded)
    # bit-repeatable, and the device-length path is the same computation
    assert torch.equal(o, ops.decode_attention(q, kc, vc, L, c["scale"],
                                               split_kv=nsplit))
    pos = torch.tensor([L - 1], dtype=torch.int32, device=DEV)
    assert torch.equal(o, ops.decode_attention(q, kc, vc, 0, c["scale"],
                                               kv_len_dev=pos,
                                               split_kv=nsplit))


def test_split_decode_replays_from_a_graph():
    """8 greedy tokens through GraphedDecoder on a split_kv=2 cache equal the
    eager decode_step loop on a second split_kv=2 cache: the same kernels on
    both sides (workspace captured), so equal and not merely close."""
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
            cache = model.new_cache(2, 64, DEV, graphable=graphed, split_kv=2)
            assert cache.split_kv == 2
            tok = model.prefill(ids, cache).argmax(-1, keepdim=True)
            step = (GraphedDecoder(model, cache, 2, DEV).step if graphed
                    else lambda t: model.decode_step(t, cache))
            out = [tok]
            for _ in range(8):
                out.append(step(out[-1]).argmax(-1, keepdim=True))
            toks[graphed] = torch.cat(out, 1)
    assert torch.equal(toks[True], toks[False])
