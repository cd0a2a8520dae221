"""Packed sequences on the MI355X: the document mask in the attention
kernels, position restart in the embedding kernels, and a whole captured
miner step on a packed batch.

The attention references are composed per document from tests/_numerics.py
(tests/_packed_seq.py) and asserted with N.check, i.e. at the project's
measured bf16-floor bounds; the bit-exactness tests assert equality.

Run on the MI355X box: python -m pytest tests/test_packed_seq_gpu.py -m gpu
"""

import pytest
import torch

import _numerics as N
import _packed_seq as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from distributedtraining_amd.ops.backend import require_ext
    return require_ext()


def _empty(dtype):
    return torch.empty(0, dtype=dtype, device=DEV)


def _pack(c, B, H, Hk, S, D):
    parts = [c[n].permute(0, 2, 1, 3).reshape(B, S, -1) for n in "qkv"]
    return torch.cat(parts, dim=-1).contiguous().to(DEV)


def _unpack(t, H, Hk, D):
    B, S, _ = t.shape
    E, kvd = H * D, Hk * D
    return (t[..., :E].view(B, S, H, D).transpose(1, 2),
            t[..., E:E + kvd].view(B, S, Hk, D).transpose(1, 2),
            t[..., E + kvd:].view(B, S, Hk, D).transpose(1, 2))


def _run(c, shape, entry, q_lo, kvlen=None, p=0.0, fused=True):
    """o, dq, dk, dv ([B,heads,S,D]) of one forward + backward through the
    public ops, and the number of fused-backward launches it made."""
    from distributedtraining_amd import ops
    from distributedtraining_amd.ops import droprng
    B, H, Hk, S, D = shape
    m = _ext()
    qkv = _pack(c, B, H, Hk, S, D)
    droprng.counter(DEV).fill_(N.DROP_CTR)
    was = m.attn_bwd_fused_enable(fused)
    try:
        n0 = m.attn_bwd_fused_calls()
        if entry == "packed":
            qkv.requires_grad_(True)
            o = ops.qkv_attention(qkv, H, Hk, scale=c["scale"], kvlen=kvlen,
                                  p_drop=p, site=N.DROP_SITE, q_lo=q_lo)
            o.backward(c["do"].permute(0, 2, 1, 3).reshape(B, S, H * D)
                       .contiguous().to(DEV))
            o = o.view(B, S, H, D).transpose(1, 2)
            dq, dk, dv = _unpack(qkv.grad, H, Hk, D)
        else:
            q, k, v = (t.detach().requires_grad_(True)
                       for t in _unpack(qkv, H, Hk, D))
            o = ops.causal_attention(q, k, v, c["scale"], kvlen=kvlen,
                                     p_drop=p, site=N.DROP_SITE, q_lo=q_lo)
            o.backward(c["do"].to(DEV))
            dq, dk, dv = q.grad, k.grad, v.grad
        torch.cuda.synchronize()
        n_fused = m.attn_bwd_fused_calls() - n0
    finally:
        m.attn_bwd_fused_enable(was)
    return dict(o=o.detach(), dq=dq, dk=dk, dv=dv), n_fused


# ---------------------------------------------------------------------------
# Accuracy against the composed fp64 references
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["views", "packed"])
@pytest.mark.parametrize("regime", P.ATTN_DOC_REGIMES)
@pytest.mark.parametrize("case", P.ATTN_DOC_CASES, ids=P.doc_case_id)
def test_document_mask_accuracy(case, regime, entry):
    shape, starts, kv, p = case
    B, H, Hk, S, D = shape
    c = P.attn_doc_case(case, regime)
    q_lo = c["q_lo"].to(DEV)
    kvlen = None if kv is None else c["kvlen"].to(DEV)
    got, n_fused = _run(c, shape, entry, q_lo, kvlen, p)
    assert n_fused == (1 if N.attn_fused_expected(shape) else 0)
    if S <= 64:
        assert n_fused == 1      # cases 1 and 2 are the fused kernel's
    for name in N.ATTN_TENSORS:
        assert bool(torch.isfinite(got[name].float()).all()), name
    failures = []
    for name in N.ATTN_TENSORS:
        try:
            N.check("attention_doc",
                    f"{P.doc_case_id(case)}-{regime}/{entry}", name,
                    got[name], c["exact"][name], c["rounded"][name],
                    live=c["live"] if name in ("o", "dq") else None)
        except AssertionError as e:      # report every tensor, then fail
            failures.append(str(e))
    assert not failures, "\n".join(failures)
    if kv is not None:
        for b in range(B):              # padded keys: exactly zero gradient
            L = min(kv[b], S)
            assert torch.all(got["dk"][b, :, L:] == 0)
            assert torch.all(got["dv"][b, :, L:] == 0)
    # a row that is one document equals the call without q_lo, bit for bit
    whole = [b for b in range(B) if starts[b] == (0,)]
    if whole:
        plain, _ = _run(c, shape, entry, None, kvlen, p)
        for b in whole:
            for name in N.ATTN_TENSORS:
                assert torch.equal(got[name][b], plain[name][b]), (name, b)


def test_one_token_document_has_zero_dq_dk():
    """Case 2, starts [0, 1, 33]: the document [0, 1) is one token. Its only
    probability is 1, so dS = dp - delta = 0 and dq, dk are exactly zero."""
    case = P.ATTN_DOC_CASES[1]
    shape = case[0]
    c = P.attn_doc_case(case, "diffuse")
    for entry in ("views", "packed"):
        got, _ = _run(c, shape, entry, c["q_lo"].to(DEV))
        print(f"[packed] one-token document/{entry}: max |dq| "
              f"{float(got['dq'][:, :, 0].float().abs().max()):.3e}, "
              f"max |dk| {float(got['dk'][:, :, 0].float().abs().max()):.3e}")
        assert torch.all(got["dq"][:, :, 0] == 0)
        assert torch.all(got["dk"][:, :, 0] == 0)
        assert bool((got["dv"][:, :, 0] != 0).any())   # dv = dO there


# ---------------------------------------------------------------------------
# Bit-exactness
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["views", "packed"])
@pytest.mark.parametrize("case", P.ATTN_DOC_CASES[:2], ids=P.doc_case_id)
def test_fused_backward_equals_pair_under_q_lo(case, entry):
    shape = case[0]
    c = P.attn_doc_case(case, "diffuse")
    q_lo = c["q_lo"].to(DEV)
    fused, n1 = _run(c, shape, entry, q_lo, fused=True)
    pair, n0 = _run(c, shape, entry, q_lo, fused=False)
    assert (n1, n0) == (1, 0)
    for name in ("o", "dq", "dk", "dv"):
        assert torch.equal(fused[name], pair[name]), name


def test_tile_skipping_changes_no_bit():
    """Three 64-token documents in one row of 192 against the same three as
    the rows of a B = 3, S = 64 call without q_lo (two-kernel backward): a
    masked probability is exactly 0 and a fully masked leading tile leaves
    (m, l, acc) at (-inf, 0, 0), so the packed walk does the standalone
    walk's arithmetic on the same tiles in the same order."""
    from distributedtraining_amd import ops
    m = _ext()
    H, S, D, n = 2, 64, 64, 3
    q, k, v, do = (t.to(DEV) for t in N.attn_inputs(1, H, H, n * S, D,
                                                    "diffuse"))
    scale = D ** -0.5
    q_lo = P.q_lo_of(((0, 64, 128),), n * S).to(DEV)

    def split(t):       # [1,H,3S,D] -> [3,H,S,D]
        return t.reshape(H, n, S, D).transpose(0, 1).contiguous()

    def run(q, k, v, do, q_lo):
        q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
        o = ops.causal_attention(q, k, v, scale, q_lo=q_lo)
        o.backward(do)
        return o.detach(), q.grad, k.grad, v.grad

    was = m.attn_bwd_fused_enable(False)
    try:
        packed = run(q, k, v, do, q_lo)
        alone = run(split(q), split(k), split(v), split(do), None)
        torch.cuda.synchronize()
    finally:
        m.attn_bwd_fused_enable(was)
    for name, a, b in zip(("o", "dq", "dk", "dv"), packed, alone):
        assert torch.equal(split(a), b), name


def test_out_of_contract_q_lo_is_clamped():
    """q_lo above q, below 0 and decreasing, with a k_hi to match: wrong
    numbers are allowed, an error or a non-finite output is not. The kernels
    clamp every value they read to [0, q] / [0, seq]."""
    m = _ext()
    B, H, S, D = 1, 1, 70, 32
    q, k, v, do = (t.to(DEV) for t in N.attn_inputs(B, H, H, S, D, "diffuse"))
    g = torch.Generator().manual_seed(5)
    q_lo = torch.randint(-9, 2 * S, (B, S), generator=g, dtype=torch.int32)
    q_lo[0, :4] = torch.tensor([-1, 5, -(2 ** 31), 2 ** 31 - 1])
    k_hi = torch.randint(-9, 2 * S, (B, S), generator=g, dtype=torch.int32)
    k_hi[0, -2:] = torch.tensor([-(2 ** 31), 2 ** 31 - 1])
    q_lo, k_hi = q_lo.to(DEV), k_hi.to(DEV)
    kv, rng = _empty(torch.int32), torch.zeros(1, dtype=torch.int64,
                                               device=DEV)
    for fused in (True, False):      # S = 70: both take the two-kernel path
        was = m.attn_bwd_fused_enable(fused)
        try:
            o, lse = m.attn_fwd(q, k, v, D ** -0.5, kv, rng, 0, 0.0, q_lo)
            dq, dk, dv = m.attn_bwd(do, q, k, v, o, lse, D ** -0.5, kv, rng,
                                    0, 0.0, q_lo, k_hi)
            torch.cuda.synchronize()
        finally:
            m.attn_bwd_fused_enable(was)
        for name, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
            assert bool(torch.isfinite(t.float()).all()), name


def test_bindings_check_q_lo():
    m = _ext()
    B, H, S, D = 1, 1, 16, 32
    q, k, v, do = (t.to(DEV) for t in N.attn_inputs(B, H, H, S, D, "diffuse"))
    kv, rng = _empty(torch.int32), torch.zeros(1, dtype=torch.int64,
                                               device=DEV)
    good = torch.zeros(B, S, dtype=torch.int32, device=DEV)
    for bad in (good.long(), good.cpu(), good[:, :8],
                torch.zeros(B, 2 * S, dtype=torch.int32,
                            device=DEV)[:, ::2]):
        with pytest.raises(RuntimeError):
            m.attn_fwd(q, k, v, 1.0, kv, rng, 0, 0.0, bad)
    o, lse = m.attn_fwd(q, k, v, 1.0, kv, rng, 0, 0.0, good)
    with pytest.raises(RuntimeError):     # the backward needs k_hi
        m.attn_bwd(do, q, k, v, o, lse, 1.0, kv, rng, 0, 0.0, good)


# ---------------------------------------------------------------------------
# Embedding
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.EMB_DOC_CASES, ids=str)
def test_embedding_position_restart(case):
    m = _ext()
    (B, S, E, V, Pn), _st = case
    c = P.emb_doc_case(case)
    ids, ds = c["ids"].to(DEV), c["doc_start"].to(DEV)
    wte, wpe, dy = (c[n].to(DEV) for n in ("wte", "wpe", "dy"))
    y = m.embedding_fwd(ids, wte, wpe, _empty(torch.int32), ds)
    assert torch.equal(N.d(y), c["y"])       # fp32 sum, rounded once
    dwte, dwpe = m.embedding_bwd(dy, ids, V, Pn, ds)
    N.check("embedding_doc", str(case), "dwpe", dwpe, c["dwpe_exact"],
            c["dwpe_f32"], fp32_out=True)
    assert torch.all(dwpe[~c["used"].to(DEV)] == 0)   # positions no token has
    assert bool(c["used"].any()) and not bool(c["used"].all())
    _, again = m.embedding_bwd(dy, ids, V, Pn, ds)
    assert torch.equal(dwpe, again)                   # repeats bit for bit
    # dwte does not depend on the layout. It is an fp32 atomic scatter whose
    # add order varies from launch to launch, so it does not repeat bit for
    # bit even between two unpacked calls: "unchanged" is asserted as both
    # calls meeting the same N.check bound against the same references
    ref = {mode: N.embedding(c["ids"], N.d(c["wte"]), N.d(c["wpe"]),
                             N.d(c["dy"]), mode=mode)["dwte"]
           for mode in ("exact", "rounded")}
    plain, _ = m.embedding_bwd(dy, ids, V, Pn)
    for tag, got in (("dwte", dwte), ("dwte_unpacked", plain)):
        N.check("embedding_doc", str(case), tag, got, ref["exact"],
                ref["rounded"], fp32_out=True)


def test_embedding_through_autograd_and_bad_doc_start():
    from distributedtraining_amd import ops
    case = P.EMB_DOC_CASES[0]
    (B, S, E, V, Pn), _st = case
    c = P.emb_doc_case(case)
    wte = c["wte"].to(DEV).requires_grad_(True)
    wpe = c["wpe"].to(DEV).requires_grad_(True)
    y = ops.embedding_fwd(c["ids"].to(DEV), wte, wpe,
                          doc_start=c["doc_start"].to(DEV))
    y.backward(c["dy"].to(DEV))
    # the fp32 sums cast to the parameter's bf16
    N.check("embedding_doc", str(case), "dwpe_autograd", wpe.grad,
            c["dwpe_exact"], N.bf16(c["dwpe_exact"]))
    # out of contract: clamped, finite, no error
    m = _ext()
    bad = torch.randint(-5, 3 * S, (B, S), dtype=torch.int32,
                        generator=torch.Generator().manual_seed(1)).to(DEV)
    y = m.embedding_fwd(c["ids"].to(DEV), c["wte"].to(DEV), c["wpe"].to(DEV),
                        _empty(torch.int32), bad)
    _, dwpe = m.embedding_bwd(c["dy"].to(DEV), c["ids"].to(DEV), V, Pn, bad)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y.float()).all())
    assert bool(torch.isfinite(dwpe).all())


# ---------------------------------------------------------------------------
# Whole step: captured graph on packed batches
# ---------------------------------------------------------------------------
def test_graphed_step_matches_eager_on_packed_batches():
    """GPT-2 tiny, seq 64 (the fused backward), dropout on. Two replays with
    different batches AND different document layouts against the same two
    steps run eagerly from the same state: doc_start is a static buffer the
    replay re-reads."""
    from distributedtraining_amd.config import Config, ModelConfig
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.ops import droprng
    from distributedtraining_amd.parallel.flat import FlatParams
    from distributedtraining_amd.parallel.graphstep import GraphedMinerStep
    from distributedtraining_amd.roles.miner import DeltaLoop
    from distributedtraining_amd.utils.data import synthetic_batches

    cfg = Config()
    cfg.model = ModelConfig.gpt2_tiny()
    cfg.model.resid_pdrop = cfg.model.embd_pdrop = cfg.model.attn_pdrop = 0.1
    B, S = 4, 64

    def mk():
        torch.manual_seed(0)
        model = build_model(cfg.model).to(DEV)
        fp = FlatParams(model)
        data = synthetic_batches(cfg.model.vocab_size, B, S, seed=1)
        return DeltaLoop(model, fp, data, cfg.train)

    g = torch.Generator().manual_seed(7)
    layouts = [((0, 17, 48), (0,), (0, 1, 33), (0, 63)),
               ((0,), (0, 32), (0, 5, 6, 40), (0, 20, 41))]
    batches = []
    for st in layouts:
        ids = torch.randint(0, cfg.model.vocab_size, (B, S), generator=g)
        batches.append({"input_ids": ids.to(DEV), "labels": ids.to(DEV),
                        "doc_start": P.q_lo_of(st, S).to(DEV)})

    ctr0 = 1234
    droprng.counter(DEV).fill_(ctr0)
    graphed = mk()
    gs = GraphedMinerStep(graphed, batches, warmup=3)
    assert gs.doc_start is not None        # the layout IS staged
    g_losses = []
    for b in batches:
        gs.step(b)
        g_losses.append(gs.loss.detach().float().clone())
    torch.cuda.synchronize()

    droprng.counter(DEV).fill_(ctr0)
    eager = mk()
    for _ in range(3):                      # match GraphedMinerStep warmup
        eager.train_step(batches[0])
    e_losses = [eager.train_step(b).detach().float().clone() for b in batches]
    torch.cuda.synchronize()
    for gl, el in zip(g_losses, e_losses):
        torch.testing.assert_close(gl, el, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(graphed.fp.master, eager.fp.master,
                               rtol=1e-4, atol=1e-4)
    # the second layout matters: the same steps with the second batch under
    # the FIRST layout end elsewhere by the very comparison passed above, so
    # a replay that kept the captured layout would have shown
    droprng.counter(DEV).fill_(ctr0)
    stale = mk()
    for _ in range(3):
        stale.train_step(batches[0])
    stale.train_step(batches[0])
    stale.train_step(dict(batches[1], doc_start=batches[0]["doc_start"]))
    torch.cuda.synchronize()
    assert not torch.allclose(graphed.fp.master, stale.fp.master, rtol=1e-4,
                              atol=1e-4)
    # a packed batch cannot be fed to a graph captured without a layout
    plain = mk()
    gp = GraphedMinerStep(plain, [{k: v for k, v in batches[0].items()
                                   if k != "doc_start"}], warmup=1)
    with pytest.raises(ValueError):
        gp.step(batches[0])
