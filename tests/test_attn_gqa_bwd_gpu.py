"""GQA attention backward on the MI355X: the one-pass dK/dV kernel
(attn_bwd_dkv_gqa_k) that walks a KV head's query-head group in one block.

Every test forces the route with attn_gqa.bwd_enable(True) and asserts from
attn_gqa.bwd_calls() that each backward took it. References and bounds are
those of tests/_numerics.py and tests/_packed_seq.py (fp64 exact and
bf16-rounded attention, N.check's measured bf16-floor bounds); nothing here
sets a tolerance. The bit tests assert equality.

Run on the MI355X box: python -m pytest tests/test_attn_gqa_bwd_gpu.py -m gpu
"""

import pytest
import torch

import _numerics as N
import _packed_seq as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (B, H, Hk, S, D), kvlen, p: group sizes 2, 4, 3, 7; head dims 64, 128, 32;
# ragged key blocks (96, 130, 70), an odd tile count, the batch stride, the
# per-head dropout seed with a fully padded key block, one row
CASES = [((1, 4, 2, 96, 64), None, 0.0),
         ((1, 8, 2, 130, 128), None, 0.0),
         ((2, 6, 2, 64, 32), None, 0.0),
         ((1, 7, 1, 70, 64), None, 0.0),
         ((2, 4, 2, 96, 64), (96, 64), 0.25),
         ((1, 4, 2, 1, 64), None, 0.0)]
DOC_CASE = ((1, 4, 2, 96, 64), ((0, 40, 64),), None, 0.0)
assert DOC_CASE in P.ATTN_DOC_CASES
REGIMES = ("diffuse", "rising")


def _run(c, shape, entry, kvlen=None, p=0.0, q_lo=None):
    """o, dq, dk, dv ([B,heads,S,D]) of one forward + backward through the
    public ops with the one-pass route forced, and its launch count."""
    from distributedtraining_amd import ops
    from distributedtraining_amd.ops import droprng
    from distributedtraining_amd.ops.backend import require_ext
    B, H, Hk, S, D = shape
    m = require_ext()
    droprng.counter(DEV).fill_(N.DROP_CTR)
    was = m.attn_gqa.bwd_enable(True)
    try:
        n0 = m.attn_gqa.bwd_calls()
        if entry == "packed":
            qkv = torch.cat([c[n].permute(0, 2, 1, 3).reshape(B, S, -1)
                             for n in "qkv"], dim=-1).contiguous().to(DEV)
            qkv.requires_grad_(True)
            o = ops.qkv_attention(qkv, H, Hk, scale=c["scale"], kvlen=kvlen,
                                  p_drop=p, site=N.DROP_SITE, q_lo=q_lo)
            o.backward(c["do"].permute(0, 2, 1, 3).reshape(B, S, H * D)
                       .contiguous().to(DEV))
            o = o.view(B, S, H, D).transpose(1, 2)
            E, kvd = H * D, Hk * D
            g = qkv.grad
            dq = g[..., :E].view(B, S, H, D).transpose(1, 2)
            dk = g[..., E:E + kvd].view(B, S, Hk, D).transpose(1, 2)
            dv = g[..., E + kvd:].view(B, S, Hk, D).transpose(1, 2)
        else:
            q, k, v = (c[n].to(DEV).requires_grad_(True) for n in "qkv")
            o = ops.causal_attention(q, k, v, c["scale"], kvlen=kvlen,
                                     p_drop=p, site=N.DROP_SITE, q_lo=q_lo)
            o.backward(c["do"].to(DEV))
            dq, dk, dv = q.grad, k.grad, v.grad
        torch.cuda.synchronize()
        n_gqa = m.attn_gqa.bwd_calls() - n0
    finally:
        m.attn_gqa.bwd_enable(was)
    return dict(o=o.detach(), dq=dq, dk=dk, dv=dv), n_gqa


def _check(op, case_id, got, c, kv, shape):
    failures = []
    for name in N.ATTN_TENSORS:
        assert bool(torch.isfinite(got[name].float()).all()), name
        try:
            N.check(op, case_id, name, got[name], c["exact"][name],
                    c["rounded"][name],
                    live=c["live"] if name in ("o", "dq") else None)
        except AssertionError as e:      # report every tensor, then fail
            failures.append(str(e))
    assert not failures, "\n".join(failures)
    if kv is not None:                   # padded keys: exactly zero gradient
        for b in range(shape[0]):
            L = min(kv[b], shape[3])
            assert torch.all(got["dk"][b, :, L:] == 0)
            assert torch.all(got["dv"][b, :, L:] == 0)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_gqa_backward_accuracy(case, regime):
    shape, kv, p = case
    c = N.attn_case((shape, regime, kv, p))
    kvlen = None if kv is None else c["kvlen"].to(DEV)
    got, n_gqa = _run(c, shape, "views", kvlen, p)
    assert n_gqa == 1
    _check("attention_gqa", N.case_id((shape, regime, kv, p)), got, c, kv,
           shape)


@pytest.mark.parametrize("regime", REGIMES)
def test_gqa_backward_document_mask(regime):
    shape = DOC_CASE[0]
    c = P.attn_doc_case(DOC_CASE, regime)
    got, n_gqa = _run(c, shape, "views", q_lo=c["q_lo"].to(DEV))
    assert n_gqa == 1
    _check("attention_gqa_doc", f"{P.doc_case_id(DOC_CASE)}-{regime}", got,
           c, None, shape)


@pytest.mark.parametrize("shape", [(2, 8, 2, 96, 64), (1, 8, 2, 130, 128)],
                         ids=str)
def test_gqa_backward_packed(shape):
    case = (shape, "diffuse", None, 0.0)
    c = N.attn_case(case)
    got, n_gqa = _run(c, shape, "packed")
    assert n_gqa == 1
    _check("attention_gqa", N.case_id(case) + "/packed", got, c, None, shape)


def test_gqa_backward_bits():
    """Fixed summation order: two runs agree bit for bit, and so do separate
    dk/dv tensors and strided views of one dqkv buffer."""
    shape, p = (2, 8, 2, 130, 128), 0.1
    q, k, v, do = N.attn_inputs(*shape, "diffuse")
    c = dict(q=q, k=k, v=v, do=do, scale=shape[4] ** -0.5)
    a, n1 = _run(c, shape, "views", p=p)
    b, n2 = _run(c, shape, "views", p=p)
    pk, n3 = _run(c, shape, "packed", p=p)
    assert (n1, n2, n3) == (1, 1, 1)
    for name in ("dk", "dv"):
        assert torch.equal(a[name], b[name]), name
        assert torch.equal(a[name], pk[name]), name
