"""The two fused backward kernels against the kernel pairs they replace,
in one build: attn_bwd_fused_k vs attn_bwd_dq_k + attn_bwd_dkv_k, and
ce_fwd_bwd_k vs ce_fwd_k + ce_bwd_k.

Both fused kernels run the arithmetic of the pair in the same order, so
everything a single block computes is compared bit for bit. The one value
that is not is CE's loss_sum: it is an fp32 atomicAdd over the rows in
whatever order the blocks finish, which differs between two runs of ce_fwd
alone. It is checked against the bound of a reordered fp32 sum instead.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from distributedtraining_amd.ops.backend import require_ext
    return require_ext()


def _rand_bf16(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV, torch.bfloat16)


# ---------------------------------------------------------------------------
# Attention
# ---------------------------------------------------------------------------
# head dim 128 is not instantiated for the fused kernel (its panels need
# 90 KB of LDS): it is a fallback shape below, not an equality case.
ATTN_SHAPES = [(2, 3, 3, 64, 64), (1, 1, 1, 48, 32), (2, 2, 2, 17, 64),
               (1, 2, 2, 1, 64)]


def _kvlen_sets(B, S):
    """Batches of kvlen rows that between them hold a full row, a short one
    and a single key."""
    lens = [S, min(5, S), 1]
    sets = []
    for i in range(0, len(lens), B):
        row = lens[i:i + B]
        row += [S] * (B - len(row))
        sets.append(torch.tensor(row, dtype=torch.int32, device=DEV))
    return sets


def _attn_grads(entry, shape, kvlen, p, fused):
    """(grads, number of fused launches) of one forward + backward."""
    from distributedtraining_amd import ops
    from distributedtraining_amd.ops import droprng
    B, H, Hkv, S, D = shape
    m = _ext()
    was = m.attn_bwd_fused_enable(fused)
    try:
        n0 = m.attn_bwd_fused_calls()
        droprng.counter(DEV).fill_(42)
        if entry == "packed":
            qkv = _rand_bf16(B, S, (H + 2 * Hkv) * D,
                             seed=41).requires_grad_(True)
            o = ops.qkv_attention(qkv, H, Hkv, kvlen=kvlen, p_drop=p, site=7)
            o.backward(_rand_bf16(B, S, H * D, seed=44))
            grads = (qkv.grad,)
        else:
            q = _rand_bf16(B, S, H * D, seed=31).view(B, S, H, D) \
                .transpose(1, 2).requires_grad_(True)
            k = _rand_bf16(B, S, Hkv * D, seed=32).view(B, S, Hkv, D) \
                .transpose(1, 2).requires_grad_(True)
            v = _rand_bf16(B, S, Hkv * D, seed=33).view(B, S, Hkv, D) \
                .transpose(1, 2).requires_grad_(True)
            o = ops.causal_attention(q, k, v, 1.0 / math.sqrt(D),
                                     kvlen=kvlen, p_drop=p, site=7)
            o.backward(_rand_bf16(B, H, S, D, seed=34))
            grads = (q.grad, k.grad, v.grad)
        torch.cuda.synchronize()
        return grads, m.attn_bwd_fused_calls() - n0
    finally:
        m.attn_bwd_fused_enable(was)


@pytest.mark.parametrize("entry", ["packed", "views"])
@pytest.mark.parametrize("variant", ["plain", "kvlen", "drop0.1", "drop0.25"])
@pytest.mark.parametrize("shape", ATTN_SHAPES)
def test_attention_fused_equals_two_kernels(shape, variant, entry):
    B, _H, _Hkv, S, _D = shape
    p = float(variant[4:]) if variant.startswith("drop") else 0.0
    masks = _kvlen_sets(B, S) if variant == "kvlen" else [None]
    for kvlen in masks:
        got, n_fused = _attn_grads(entry, shape, kvlen, p, True)
        ref, n_ref = _attn_grads(entry, shape, kvlen, p, False)
        assert n_fused == 1 and n_ref == 0
        for name, a, b in zip("qkv", got, ref):
            assert not torch.isnan(b.float()).any()
            assert torch.equal(a, b), (
                f"d{name} differs, kvlen={kvlen}: max abs "
                f"{(a.float() - b.float()).abs().max().item()}")


@pytest.mark.parametrize("shape,fused", [
    ((2, 8, 2, 64, 128), 0),    # GQA
    ((2, 3, 3, 70, 64), 0),     # two tiles
    ((2, 2, 2, 64, 128), 0),    # head dim 128: not instantiated
    ((2, 3, 3, 64, 64), 1),
])
def test_attention_fused_fallback_rule(shape, fused):
    for entry in ("packed", "views"):
        _, n = _attn_grads(entry, shape, None, 0.0, True)
        assert n == fused


# ---------------------------------------------------------------------------
# Cross entropy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows,vocab,all_ignored", [
    (64, 50257, False), (32, 1000, False), (128, 512, False), (3, 7, False),
    (5, 50257, True)])
def test_ce_fwd_bwd_equals_two_kernels(rows, vocab, all_ignored):
    m = _ext()
    logits = _rand_bf16(rows, vocab, seed=14, scale=3.0)
    g = torch.Generator().manual_seed(15)
    targets = torch.randint(0, vocab, (rows,), generator=g).to(DEV)
    targets[::7] = -100  # ignore_index stripes
    if all_ignored:
        targets[:] = -100
    loss_sum, lse, count = m.ce_fwd(logits, targets, -100)
    cf = count.clamp(min=1).to(torch.float32)
    inv = (torch.ones_like(cf) / cf).reshape(1)
    dl = m.ce_bwd(logits, targets, lse, inv, 0.0, -100, 0, True)

    buf = logits.clone()
    loss_sum2, lse2, count2 = m.ce_fwd_bwd(buf, targets, -100, inv)
    assert int(count2) == int(count) == int((targets != -100).sum())
    assert torch.equal(lse2, lse)
    assert torch.equal(buf, dl)
    if all_ignored:
        assert not buf.float().any() and float(loss_sum2) == 0.0
    # loss_sum: the same n fp32 terms, atomically added in block-finish
    # order. With unit roundoff u = 2^-24 an fp32 sum in any order is within
    # (n - 1) u sum|t| of the exact sum of its terms, and each term
    # lse - logit carries one more rounding: n u sum|t| from the fp64 sum,
    # twice that between two orders.
    valid = targets != -100
    terms = (lse.double() - logits[torch.arange(rows, device=DEV),
                                   targets.clamp(min=0)].double())[valid]
    bound = 2 * int(valid.sum()) * 2.0 ** -24 * float(terms.abs().sum())
    print(f"loss_sum fused {float(loss_sum2)!r} two-kernel "
          f"{float(loss_sum)!r} fp64 {float(terms.sum())!r} bound {bound!r}")
    assert abs(float(loss_sum2) - float(loss_sum)) <= bound
    assert abs(float(loss_sum2) - float(terms.sum())) <= bound


@pytest.mark.parametrize("rows,vocab,all_ignored", [
    (64, 50257, False), (32, 1000, False), (128, 512, False), (3, 7, False),
    (5, 50257, True), (300, 50257, False)])
def test_ce_fwd_bwd_lds_row(rows, vocab, all_ignored):
    """The variant that holds the row in LDS: 1024 threads cut a row into
    other per-thread (m, s) streams than ce_fwd's 256, so lse and with it
    dlogits agree to rounding, not bit for bit. Hence the tolerances of
    test_ops_gpu.py::test_cross_entropy against F.cross_entropy. Odd vocab
    puts every row on another 16 B phase (head/tail peel); 300 rows is more
    than one row per block."""
    m = _ext()
    logits = _rand_bf16(rows, vocab, seed=14, scale=3.0)
    g = torch.Generator().manual_seed(15)
    targets = torch.randint(0, vocab, (rows,), generator=g).to(DEV)
    targets[::7] = -100
    if all_ignored:
        targets[:] = -100
    n_valid = int((targets != -100).sum())
    inv = torch.tensor([1.0 / max(n_valid, 1)], device=DEV)
    buf = logits.clone()
    loss_sum, lse, count = m.ce_fwd_bwd(buf, targets, -100, inv, 0, True)
    assert int(count) == n_valid
    torch.testing.assert_close(
        lse, torch.logsumexp(logits.float(), dim=1), rtol=1e-5, atol=1e-5)
    if all_ignored:
        assert not buf.float().any() and float(loss_sum) == 0.0
        return
    ref = torch.nn.functional.cross_entropy(logits.float(), targets,
                                            ignore_index=-100,
                                            reduction="sum")
    torch.testing.assert_close(loss_sum.float().cpu(), ref.cpu(),
                               rtol=1e-2, atol=1e-2 * rows)
    lr = logits.float().detach().requires_grad_(True)
    torch.nn.functional.cross_entropy(lr, targets,
                                      ignore_index=-100).backward()
    torch.testing.assert_close(buf.float(), lr.grad, rtol=5e-2, atol=1e-4)


def _head_grads(ops, fused, mult, main_grad, tgt, T, K, V):
    """(loss, x.grad, w grad) of (mult * lm_head_ce).backward()."""
    keep = ops._CE_FUSED
    try:
        ops._CE_FUSED = fused
        x = _rand_bf16(T, K, seed=70, scale=0.5).requires_grad_(True)
        w = _rand_bf16(V, K, seed=71, scale=0.2).requires_grad_(True)
        if main_grad:
            w.main_grad = torch.zeros_like(w)
        loss, logits = ops.lm_head_ce(x, w, tgt, need_logits=False,
                                      overwrite_logits=True)
        assert (logits is None) == fused
        (mult * loss).backward()
        return (loss.detach(), x.grad.float(),
                (w.main_grad if main_grad else w.grad).float())
    finally:
        ops._CE_FUSED = keep


def _close_at_scale(got, ref, what):
    """The linear-backward tolerances of test_ops_gpu.py (rtol 5e-2, atol
    5e-2), with the atol brought down to the gradient's own magnitude
    where that is below 1: these gradients are about 1e-2 at dloss == 1,
    and an atol above them would accept any value, zero included."""
    peak = float(ref.abs().max())
    assert peak > 0, what
    print(f"{what}: max|ref| {peak:.4g} max|diff| "
          f"{float((got - ref).abs().max()):.4g}")
    torch.testing.assert_close(got, ref, rtol=5e-2,
                               atol=5e-2 * min(1.0, peak), msg=lambda m: (
                                   f"{what}: {m}"))


@pytest.mark.parametrize("main_grad", [False, True])
def test_lm_head_ce_fused_dloss(main_grad):
    """The kernel bakes dloss == 1 into the stored gradient; backward puts
    the real dloss on the [T, K] side of both head GEMMs. Against the
    unfused path, at dloss 1, 3 and 64 (64 lifts the gradients to O(1)),
    and the fused gradients must scale with dloss."""
    from distributedtraining_amd import ops
    T, K, V = 96, 64, 1000
    tgt = torch.randint(0, V, (T,),
                        generator=torch.Generator().manual_seed(3)).to(DEV)
    tgt[::5] = -100
    fused = {}
    for mult in (1.0, 3.0, 64.0):
        got = _head_grads(ops, True, mult, main_grad, tgt, T, K, V)
        ref = _head_grads(ops, False, mult, main_grad, tgt, T, K, V)
        # the loss is an atomically ordered fp32 sum of T positive terms
        torch.testing.assert_close(got[0], ref[0],
                                   rtol=2 * (T + 2) * 2.0 ** -24, atol=0)
        _close_at_scale(got[1], ref[1], f"x.grad, dloss {mult}")
        _close_at_scale(got[2], ref[2], f"w grad, dloss {mult}")
        fused[mult] = got
    for mult in (3.0, 64.0):
        _close_at_scale(fused[mult][1], mult * fused[1.0][1],
                        f"x.grad, dloss {mult} against {mult} x dloss 1")
        _close_at_scale(fused[mult][2], mult * fused[1.0][2],
                        f"w grad, dloss {mult} against {mult} x dloss 1")


def test_lm_head_ce_fused_lds_row_variant():
    """DTA_CE_FUSED=lds through ops.lm_head_ce, against the unfused path."""
    from distributedtraining_amd import ops
    T, K, V = 96, 64, 1000
    tgt = torch.randint(0, V, (T,),
                        generator=torch.Generator().manual_seed(3)).to(DEV)
    tgt[::5] = -100
    keep = ops._CE_FUSED_LDS
    try:
        ops._CE_FUSED_LDS = True
        got = _head_grads(ops, True, 64.0, True, tgt, T, K, V)
    finally:
        ops._CE_FUSED_LDS = keep
    ref = _head_grads(ops, False, 64.0, True, tgt, T, K, V)
    # atomic order of T terms (1.2e-5) plus the last bit of each lse
    torch.testing.assert_close(got[0], ref[0], rtol=2e-5, atol=0)
    _close_at_scale(got[1], ref[1], "x.grad, LDS row")
    _close_at_scale(got[2], ref[2], "w grad, LDS row")


def test_lm_head_ce_keeps_logits_unless_given_up():
    """need_logits=False alone still returns the one-shot logits; only
    overwrite_logits hands the buffer to the fused kernel."""
    from distributedtraining_amd import ops
    x = _rand_bf16(32, 64, seed=72, scale=0.5).requires_grad_(True)
    w = _rand_bf16(300, 64, seed=73, scale=0.2).requires_grad_(True)
    tgt = torch.randint(0, 300, (32,), device=DEV)
    loss, logits = ops.lm_head_ce(x, w, tgt, need_logits=False)
    if not ops._CE_PIPE:
        torch.testing.assert_close(logits.float(),
                                   x.detach().float() @ w.detach().float().T,
                                   rtol=2e-2, atol=2e-2)
    with torch.no_grad():
        _, logits = ops.lm_head_ce(x, w, tgt, need_logits=False,
                                   overwrite_logits=True)
    assert logits is not None   # no grad wanted: nothing to overwrite with
