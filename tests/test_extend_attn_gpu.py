"""Extend attention (attn_extend_k [+ attn_decode_combine_k] in
hip/attention.hip) on the GPU: Sq new queries on a filled KV cache against
fp64, and chunked prefill through both model families.

Rounding points modelled in ``_rounded`` (the kernel's):
  * P before P.V: exp2(s - m_run) is packed to bf16, with m_run the row's
    running max after the CURRENT 32-key tile of its walk. The walk of a row
    in split s starts at key s * chunk, chunk = 32 * ceil((P + Sq) / (32 *
    nsplit)), and a tile past the row's last visible key changes nothing.
  * l sums the UNROUNDED fp32 p.
  * the accumulator rescales, the split partials (m, l, acc) and 1/l stay
    fp32: exact in the fp64 model.
  * o: rounded to bf16 once, after the last merge.
"""

import copy

import pytest
import torch

import _numerics as N
from distributedtraining_amd import ops
from distributedtraining_amd.config import ModelConfig
from distributedtraining_amd.models import build_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOG2E = 1.4426950408889634     # the kernel works in exp2 units

# (P, Sq, nsplit, H, Hk, D, regime), B = 2, cache capacity P + Sq + 7.
CASES = [
    (40, 1, 1, 4, 4, 64, "diffuse"),      # Sq = 1: decode
    (0, 1, 2, 2, 2, 128, "diffuse"),      # one key, split 1 empty
    (0, 33, 1, 4, 2, 128, "diffuse"),     # P = 0: causal attention
    (1, 2, 1, 4, 4, 64, "diffuse"),       # band against the 32-key tile edges,
    (31, 5, 1, 8, 2, 128, "rising"),      # Sq * grp off the 16-row wave tile
    (32, 17, 1, 4, 4, 64, "diffuse"),
    (33, 5, 1, 6, 2, 128, "rising"),
    (31, 17, 2, 8, 2, 64, "diffuse"),
    (5, 19, 1, 7, 1, 64, "diffuse"),      # grp 7: 133 rows = 3 blocks, a block
    (5, 19, 2, 7, 1, 128, "rising"),      # boundary inside a head group
    (10, 5, 1, 16, 1, 128, "diffuse"),    # grp 16: two blocks
    (3, 70, 1, 2, 2, 64, "rising"),       # grp 1: two blocks, two walk lengths
    (257, 5, 1, 8, 2, 128, "rising"),     # several tiles, look-ahead
    (257, 5, 3, 8, 2, 64, "diffuse"),
    (20, 30, 2, 4, 2, 128, "diffuse"),    # early rows see nothing of split 1
    (28, 5, 3, 4, 4, 64, "diffuse"),      # full, one-key and empty split
]


def _inputs(case):
    """q of all P + Sq positions (the op gets the strided view of the last
    Sq), caches with 7 rows of 3e4 past the valid range: a key read from
    there is a gross error."""
    P, Sq, _, H, Hk, D, regime = case
    q, k, v, _ = N.attn_inputs(2, H, Hk, P + Sq, D, regime)
    fill = torch.full((2, Hk, 7, D), 3e4, dtype=torch.bfloat16)
    return q, torch.cat([k, fill], 2), torch.cat([v, fill], 2)


def _reference(q, kc, vc, P, scale, nsplit):
    """(exact, rounded) [B,Sq,H,D] in fp64."""
    B, H, Sq, D = q.shape
    L = P + Sq
    head = torch.arange(H) // (H // kc.shape[1])
    k, v = kc[:, head, :L], vc[:, head, :L]
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale * LOG2E
    vis = torch.arange(L)[None, :] <= P + torch.arange(Sq)[:, None]
    s = s.masked_fill(~vis, -float("inf"))
    exact = torch.einsum("bhqk,bhkd->bhqd", torch.softmax(s / LOG2E, -1), v)
    M = s.amax(-1, keepdim=True)
    chunk = 32 * -(-L // (32 * nsplit))
    num = torch.zeros(B, H, Sq, D, dtype=N.F64)
    den = torch.zeros(B, H, Sq, 1, dtype=N.F64)
    for s0 in range(0, L, chunk):
        m_run = torch.full((B, H, Sq, 1), -float("inf"), dtype=N.F64)
        for k0 in range(s0, min(L, s0 + chunk), 32):
            st = s[..., k0:k0 + 32]
            m_run = torch.maximum(m_run, st.amax(-1, keepdim=True))
            seen = m_run > -float("inf")
            p = torch.where(seen, torch.exp2(st - m_run), 0.0)
            r = torch.where(seen, torch.exp2(m_run - M), 0.0)
            num += r * torch.einsum("bhqk,bhkd->bhqd", N.bf16(p),
                                    v[:, :, k0:k0 + 32])
            den += r * p.sum(-1, keepdim=True)
    return exact.transpose(1, 2), N.bf16(num / den).transpose(1, 2)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_extend_accuracy(case):
    P, Sq, nsplit, H, Hk, D, _ = case
    q, kc, vc = _inputs(case)
    scale = D ** -0.5
    exact, rounded = _reference(N.d(q[:, :, P:]), N.d(kc), N.d(vc), P, scale,
                                nsplit)
    args = (q.to(DEV)[:, :, P:], kc.to(DEV), vc.to(DEV), P, scale)
    o = ops.extend_attention(*args, split_kv=nsplit)
    assert o.shape == (2, Sq, H, D) and o.dtype == torch.bfloat16
    assert o.is_contiguous()
    N.check("attn_extend", str(case), "o", o, exact, rounded)
    assert torch.equal(o, ops.extend_attention(*args, split_kv=nsplit))


def test_extend_contract_errors():
    def call(H, Hk, D, **kw):
        q = torch.zeros(1, H, 2, D, device=DEV, dtype=torch.bfloat16)
        c = torch.zeros(1, Hk, 8, D, device=DEV, dtype=kw.pop("cdtype", q.dtype))
        return ops.extend_attention(q, c, c, 3, **kw)
    assert call(4, 2, 64).shape == (1, 2, 4, 64)
    with pytest.raises(ValueError):
        call(4, 2, 32)
    with pytest.raises(ValueError):
        call(32, 1, 64)
    sc = torch.ones(1, 2, 32, device=DEV)
    with pytest.raises(ValueError):
        call(4, 2, 64, cdtype=torch.int8, k_scale=sc, v_scale=sc)


CFGS = {
    "gpt2": dict(family="gpt2", n_head=4, resid_pdrop=0.0, embd_pdrop=0.0,
                 attn_pdrop=0.0),
    "llama": dict(family="llama", n_head=4, n_kv_head=2, intermediate_size=512,
                  rope_theta=10000.0, tie_word_embeddings=False),
}


@pytest.mark.parametrize("family", sorted(CFGS))
def test_chunked_prefill_on_device(family):
    """A 40-token prompt prefilled as 16 + 16 + 8 against one pass (the code
    as it was): the last-position logits of both against an fp32 CPU forward
    of the same bf16-valued weights. The chunked error may be at most
    BF16_FACTOR x the one-pass error. Then 4 decode steps on that cache."""
    cfg = ModelConfig(vocab_size=512, n_layer=2, n_embd=256, n_positions=64,
                      **CFGS[family])
    torch.manual_seed(6)
    model = build_model(cfg).to(DEV, torch.bfloat16).eval()
    ids = torch.randint(0, 512, (2, 40), device=DEV)
    with torch.no_grad():
        ref = copy.deepcopy(model).to("cpu").float()(
            input_ids=ids.cpu()).logits[:, -1]
        one = model.prefill(ids, model.new_cache(2, 64, DEV))
        cache = model.new_cache(2, 64, DEV)
        for s0, s1 in ((0, 16), (16, 32), (32, 40)):
            got = model.prefill(ids[:, s0:s1], cache)
        e_one, e_got = N.errors(one, ref), N.errors(got, ref)
        print(f"[acc] chunked prefill {family}: one pass {e_one}, "
              f"chunked {e_got}")
        assert e_got[0] <= N.BF16_FACTOR * e_one[0]
        assert e_got[1] <= N.BF16_FACTOR * e_one[1]
        tok = got.argmax(-1, keepdim=True)
        for _ in range(4):
            tok = model.decode_step(tok, cache).argmax(-1, keepdim=True)
    assert cache.len == 44
