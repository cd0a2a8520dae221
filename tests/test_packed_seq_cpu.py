"""Packed sequences on the CPU path: the q_lo contract check, the packer,
the CPU gold of the document mask, and the claim the feature rests on — one
packed row computes what its documents compute one per call (logits, loss,
gradients), for learned positions (GPT-2) and rotary ones (Llama)."""

import pytest
import torch

import _packed_seq as P
from distributedtraining_amd import ops
from distributedtraining_amd.config import ModelConfig
from distributedtraining_amd.models import build_model
from distributedtraining_amd.utils.textdata import (ByteTokenizer,
                                                    PackedTextDataset,
                                                    packed_text_batches)


# ---- check_q_lo -------------------------------------------------------------
def test_check_q_lo_accepts_valid_layouts():
    ops.check_q_lo(P.q_lo_of(((0, 17, 48), (0,)), 64))
    ops.check_q_lo(torch.zeros(3, 1, dtype=torch.int32))
    ops.check_q_lo(torch.arange(8, dtype=torch.int32)[None])   # 8 documents
    # not a document layout, still inside the contract (a sliding window)
    ops.check_q_lo(torch.tensor([[0, 0, 1, 2, 3]], dtype=torch.int32))


@pytest.mark.parametrize("bad", [
    torch.tensor([[0, 2, 2]], dtype=torch.int32),        # lo > q
    torch.tensor([[0, -1, 0]], dtype=torch.int32),       # negative
    torch.tensor([[0, 1, 0]], dtype=torch.int32),        # decreasing
    torch.tensor([[0, 0, 0]], dtype=torch.int64),        # dtype
    torch.tensor([0, 0, 0], dtype=torch.int32),          # shape
    torch.zeros(1, 2, 3, dtype=torch.int32),             # shape
], ids=["above_q", "negative", "decreasing", "int64", "1d", "3d"])
def test_check_q_lo_rejects(bad):
    with pytest.raises(ValueError):
        ops.check_q_lo(bad)


def test_q_lo_inverse_counts_queries():
    q_lo = P.q_lo_of(((0, 1, 5), (0,)), 9)
    k_hi = ops.q_lo_inverse(q_lo)
    assert k_hi.dtype == torch.int32
    for b in range(2):
        for k in range(9):
            assert int(k_hi[b, k]) == int((q_lo[b] <= k).sum())
    # documents: one past the last token of the document that holds k
    assert k_hi[0].tolist() == [1, 5, 5, 5, 5, 9, 9, 9, 9]


# ---- packer -----------------------------------------------------------------
TEXTS = ["the first record", "second, a little longer than the first one",
         "third one", "number four is here too", "and a fifth to end with"]
SEQ = 16


def _epoch_rows(it, n_rows, bs):
    out = {"input_ids": [], "doc_start": [], "labels": []}
    for _ in range(n_rows // bs):
        b = next(it)
        for k in out:
            out[k].append(b[k])
    return {k: torch.cat(v) for k, v in out.items()}


@pytest.mark.parametrize("bs", [1, 2, 3, 4, 5])
def test_packer_keeps_every_token_in_order(bs):
    """Across three epochs (two epoch boundaries) and batch sizes that do
    not divide the 7 rows of an epoch, the emitted ids are the EOS-joined
    stream, epoch after epoch, with nothing lost, repeated or reordered."""
    tok = ByteTokenizer()
    ds = PackedTextDataset(TEXTS, tok, seq_len=SEQ)
    stream = []
    for t in TEXTS:
        stream += tok.encode(t) + [tok.eos_token_id]
    assert len(stream) // SEQ == 7 and len(stream) % SEQ != 0
    it = packed_text_batches(ds, bs, shuffle=False)
    n_batches = 3 * len(stream) // (bs * SEQ)
    got = []
    for _ in range(n_batches):
        b = next(it)
        assert b["input_ids"].shape == (bs, SEQ)      # every batch is full
        assert torch.equal(b["labels"], b["input_ids"])
        assert tok.pad_token_id not in b["input_ids"]
        ops.check_q_lo(b["doc_start"])
        got += b["input_ids"].reshape(-1).tolist()
    assert len(got) > 2 * len(stream)                 # two epoch boundaries
    assert got == (stream * 4)[:len(got)]


def test_packer_doc_start_restarts_after_each_eos():
    tok = ByteTokenizer()
    ds = PackedTextDataset(TEXTS, tok, seq_len=SEQ)
    R = sum(len(d) for d in ds.docs) // SEQ
    rows = _epoch_rows(packed_text_batches(ds, 1, seed=3), R, 1)
    ids, st = rows["input_ids"], rows["doc_start"]
    assert st.dtype == torch.int32
    ops.check_q_lo(st)
    n_eos = 0
    for r in range(R):
        want = 0
        for s in range(SEQ):
            if s > 0 and int(ids[r, s - 1]) == tok.eos_token_id:
                want = s
                n_eos += 1
            assert int(st[r, s]) == want, (r, s)
    assert n_eos >= 2   # the layout is not trivially all zero


def test_packer_seeds():
    ds = PackedTextDataset(TEXTS, seq_len=SEQ)
    a = packed_text_batches(ds, 2, seed=5)
    b = packed_text_batches(ds, 2, seed=5)
    c = packed_text_batches(ds, 2, seed=6)
    same, differs = True, False
    for _ in range(3):
        x, y, z = next(a), next(b), next(c)
        same &= all(torch.equal(x[k], y[k]) for k in x)
        differs |= not torch.equal(x["input_ids"], z["input_ids"])
    assert same and differs


# ---- CPU gold ---------------------------------------------------------------
@pytest.mark.parametrize("kv", [None, (13, 4)])
def test_attn_ref_q_lo_is_dense_masked_softmax(kv):
    B, H, Hk, S, D = 2, 4, 2, 13, 8
    g = torch.Generator().manual_seed(0)
    q = torch.randn(B, H, S, D, generator=g)
    k = torch.randn(B, Hk, S, D, generator=g)
    v = torch.randn(B, Hk, S, D, generator=g)
    q_lo = P.q_lo_of(((0, 1, 6), (0, 12)), S)
    kvlen = None if kv is None else torch.tensor(kv, dtype=torch.int32)
    scale = 0.3
    got = ops.causal_attention(q, k, v, scale, kvlen=kvlen, q_lo=q_lo)
    # dense boolean mask, written out
    mask = torch.zeros(B, S, S, dtype=torch.bool)
    for b in range(B):
        for i in range(S):
            for j in range(S):
                mask[b, i, j] = (int(q_lo[b, i]) <= j <= i
                                 and (kv is None or j < kv[b]))
    ke = k.repeat_interleave(H // Hk, dim=1)
    ve = v.repeat_interleave(H // Hk, dim=1)
    s = torch.einsum("bhqd,bhkd->bhqk", q, ke) * scale
    s = s.masked_fill(~mask[:, None], float("-inf"))
    live = mask.any(-1)                                 # rows with a key
    want = torch.einsum("bhqk,bhkd->bhqd",
                        torch.softmax(s, -1).nan_to_num(0.0), ve)
    lv = live[:, None, :, None].expand_as(want)
    torch.testing.assert_close(got[lv], want[lv], rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        ops.causal_attention(q, k, v, scale, q_lo=q_lo + 1)


def test_embedding_cpu_restarts_positions():
    ids = torch.tensor([[3, 4, 5, 6, 7]])
    wte = torch.randn(10, 4)
    wpe = torch.randn(8, 4)
    st = torch.tensor([[0, 0, 2, 2, 4]], dtype=torch.int32)
    got = ops.embedding_fwd(ids, wte, wpe, doc_start=st)
    want = wte[ids] + wpe[torch.tensor([[0, 1, 0, 1, 0]])]
    torch.testing.assert_close(got, want, rtol=0, atol=0)


# ---- model equivalence ------------------------------------------------------
def _model(cfg, seed=0):
    torch.manual_seed(seed)
    m = build_model(cfg).float()
    m.eval()     # dropout is 0 in the tiny configs; eval returns logits
    return m


def _valid_targets(ids, doc_start=None):
    S = ids.shape[1]
    n = ids.shape[0] * (S - 1)
    if doc_start is not None:
        nxt = torch.arange(1, S, dtype=torch.int32)
        n -= int((doc_start[:, 1:] == nxt).sum())
    return n


def test_gpt2_packed_row_equals_separate_documents():
    cfg = ModelConfig.gpt2_tiny()
    m = _model(cfg)
    ids, doc_start, docs = P.equiv_batch(cfg.vocab_size)
    names = ["wte", "wpe", "blocks.0.attn_qkv_w"]
    params = dict(m.named_parameters())

    m.zero_grad()
    out = m(input_ids=ids, labels=ids, doc_start=doc_start)
    n_packed = _valid_targets(ids, doc_start)
    (out.loss * n_packed).backward()     # the loss is a mean: sum it back
    packed_loss = float(out.loss.detach()) * n_packed
    packed_grads = {n: params[n].grad.clone() for n in names}
    packed_logits = m(input_ids=ids, doc_start=doc_start).logits.detach()

    m.zero_grad()
    sep_loss, n_sep = 0.0, 0
    for s0, s1 in docs:
        d = ids[:, s0:s1]
        lg = m(input_ids=d).logits.detach()
        torch.testing.assert_close(packed_logits[:, s0:s1], lg, rtol=1e-4,
                                   atol=1e-4)
        if s1 - s0 < 2:
            continue         # a one-token document has no target
        o = m(input_ids=d, labels=d)
        n = _valid_targets(d)
        (o.loss * n).backward()
        sep_loss += float(o.loss.detach()) * n
        n_sep += n
    assert n_sep == n_packed == sum(n - 1 for n in P.EQUIV_LENS)
    torch.testing.assert_close(torch.tensor(packed_loss),
                               torch.tensor(sep_loss), rtol=1e-4, atol=1e-4)
    for n in names:
        torch.testing.assert_close(packed_grads[n], params[n].grad,
                                   rtol=1e-3, atol=1e-5)


def test_llama_packed_row_equals_separate_documents():
    """Rotary positions are not restarted: scores depend on position
    differences only, so the logits still agree."""
    cfg = ModelConfig.llama_tiny()
    m = _model(cfg, seed=1)
    ids, doc_start, docs = P.equiv_batch(cfg.vocab_size, seed=1)
    with torch.no_grad():
        packed = m(input_ids=ids, doc_start=doc_start).logits
        plain = m(input_ids=ids).logits
        for s0, s1 in docs:
            torch.testing.assert_close(packed[:, s0:s1],
                                       m(input_ids=ids[:, s0:s1]).logits,
                                       rtol=2e-4, atol=2e-4)
    # the mask is what makes them agree: without it the later documents differ
    assert not torch.allclose(packed[:, 6:], plain[:, 6:], rtol=2e-4,
                              atol=2e-4)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_label_rule_first_token_of_a_document_is_no_target(family):
    cfg = (ModelConfig.gpt2_tiny() if family == "gpt2"
           else ModelConfig.llama_tiny())
    m = _model(cfg, seed=2)
    S, starts = 16, (0, 5, 11)
    ids = torch.randint(0, cfg.vocab_size, (2, S),
                        generator=torch.Generator().manual_seed(2))
    doc_start = P.q_lo_of((starts, starts), S)
    s0 = starts[1]           # first token of the second document

    def loss(labels):
        with torch.no_grad():
            return float(m(input_ids=ids, labels=labels,
                           doc_start=doc_start).loss)

    base = loss(ids)
    first = ids.clone()
    first[:, s0] = (first[:, s0] + 1) % cfg.vocab_size
    assert loss(first) == base
    later = ids.clone()
    later[:, s0 + 1] = (later[:, s0 + 1] + 1) % cfg.vocab_size
    assert loss(later) != base
    # the last token of the first document (its separator) is still a target
    end = ids.clone()
    end[:, s0 - 1] = (end[:, s0 - 1] + 1) % cfg.vocab_size
    assert loss(end) != base


def test_check_doc_start_wants_a_document_layout():
    ops.check_doc_start(P.q_lo_of(((0, 17, 48), (0,)), 64))
    with pytest.raises(ValueError):     # inside the q_lo contract, no layout
        ops.check_doc_start(torch.tensor([[0, 0, 1, 2, 3]],
                                         dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.embedding_fwd(torch.zeros(1, 5, dtype=torch.long),
                          torch.randn(4, 4), torch.randn(8, 4),
                          doc_start=torch.tensor([[0, 0, 1, 2, 3]],
                                                 dtype=torch.int32))
