"""Fused LM-head loss kernel (hip/head_loss.hip) on the GPU.

Reference: always fp64 on the CPU from the same bf16 inputs upcast to fp64.

Tolerance: atol = 2e-4, rtol = 0 on per-row lse and target logit. The MFMA
error model gives 1.5e-7 * sum|a*b| <~ 3e-5 for these inputs (sum|a*b| <=
~150), the exp2/log2 path adds ~1e-5; 2e-4 leaves room for summation order
and is still 250x below the 0.05-0.09 error of logits rounded to bf16, so
passing also proves the accumulators are never rounded.

Inputs: N(0,1) operands at K = 64, 0.5*N(0,1) at K = 768 and 0.84*N(0,1) at
K = 128 (same logit std of ~7-8 in each case): max |logit| is ~33-36, so the
online rescale is exercised.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 2e-4
II = -100


def _ext():
    from distributedtraining_amd.ops.backend import require_ext
    return require_ext()


def _scale(K):
    return {64: 1.0, 128: 0.84, 768: 0.5}.get(K, 1.0)


def _make(T, K, V, seed=0, all_ignored=False, neg=False):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(T, K, generator=g) * _scale(K)).to(torch.bfloat16)
    w = (torch.randn(V, K, generator=g) * _scale(K)).to(torch.bfloat16)
    if neg:      # every logit negative, row max well below 0
        x, w = x.abs(), -w.abs()
    t = torch.randint(0, V, (T,), generator=g)
    t[0] = 0
    if T > 1:
        t[1] = V - 1
    # rows 2..5: targets inside the last vocab tile / last split
    for i, c in enumerate((V - 2, V - 60, V - 100, (V - 1) // 128 * 128)):
        if T > 2 + i:
            t[2 + i] = c
    t[6::7] = II   # every 7th ignored (rows 0..5 keep their forced targets)
    if all_ignored:
        t[:] = II
    return x, w, t


@functools.lru_cache(maxsize=None)
def _case(T, K, V, neg=False):
    """(x, w, t on CPU, fp64 lse, fp64 target logit) — computed once and
    shared; tests must not modify it."""
    x, w, t = _make(T, K, V, neg=neg)
    logits = x.double() @ w.double().t()
    lse = torch.logsumexp(logits, dim=-1)
    tl = logits.gather(1, t.clamp(min=0).unsqueeze(1)).squeeze(1)
    return x, w, t, lse, tl


def _check(T, K, V, nsplit, neg=False):
    x, w, t, lse_ref, tl_ref = _case(T, K, V, neg)
    loss_sum, lse, count, tl = _ext().head_loss_fwd(
        x.to(DEV), w.to(DEV), t.to(DEV), II, nsplit)
    lse, tl = lse.cpu().double(), tl.cpu().double()
    valid = t != II
    n_valid = int(valid.sum())
    e_lse = float((lse - lse_ref).abs().max())
    e_tl = float((tl - tl_ref)[valid].abs().max()) if n_valid else 0.0
    ref_sum = float((lse_ref - tl_ref)[valid].sum())
    e_sum = abs(float(loss_sum) - ref_sum)
    print(f"T={T} K={K} V={V} nsplit={nsplit} neg={neg}: max|dlse|={e_lse:.3e}"
          f" max|dtlogit|={e_tl:.3e} |dloss_sum|={e_sum:.3e} n={n_valid}")
    assert torch.isfinite(lse).all()
    assert e_lse <= ATOL
    assert e_tl <= ATOL
    assert not tl[~valid].any()      # ignored rows keep the zero init
    assert int(count) == n_valid
    assert e_sum <= ATOL * max(n_valid, 1)
    return lse, tl


# row tails below / just above one tile, vocab smaller than a few tiles,
# ragged odd vocab tails, the real GPT-2 vocab
@pytest.mark.parametrize("T,K,V", [(1, 64, 517), (17, 64, 517),
                                   (130, 128, 1000), (257, 768, 5003),
                                   (512, 64, 50257)])
def test_shape_sweep(T, K, V):
    _check(T, K, V, 0)


def test_tail_masking():
    # all logits negative: a tail column left at 0 instead of -inf would
    # shift lse by several units
    x, w, t, lse_ref, _ = _case(64, 64, 517, True)
    assert float(lse_ref.max()) < -1.0
    _check(64, 64, 517, 0, neg=True)


@pytest.mark.parametrize("nsplit", [1, 2, 3, 1000])
def test_split_invariance(nsplit):
    T, K, V = 130, 128, 1000       # 8 vocab tiles
    _, _, t, _, _ = _case(T, K, V)
    assert int(((t >= 896) & (t != II)).sum()) >= 4   # last tile / split
    _check(T, K, V, nsplit)


def test_deterministic():
    x, w, t, _, _ = _case(257, 768, 5003)
    xd, wd, td = x.to(DEV), w.to(DEV), t.to(DEV)
    _, lse1, _, tl1 = _ext().head_loss_fwd(xd, wd, td, II, 0)
    _, lse2, _, tl2 = _ext().head_loss_fwd(xd, wd, td, II, 0)
    assert torch.equal(lse1, lse2)
    assert torch.equal(tl1, tl2)


def test_all_ignored():
    from distributedtraining_amd import ops
    x, w, t = _make(130, 128, 1000, all_ignored=True)
    xd, wd, td = x.to(DEV), w.to(DEV), t.to(DEV)
    loss_sum, lse, count, tl = _ext().head_loss_fwd(xd, wd, td, II, 0)
    assert int(count) == 0
    assert float(loss_sum) == 0.0
    assert torch.isfinite(lse).all()
    assert float(ops.lm_head_loss(xd, wd, td)) == 0.0


def test_no_logits_in_memory():
    from distributedtraining_amd import ops
    T, K, V = 4096, 64, 8192
    x, w, t = _make(T, K, V)
    xd, wd, td = x.to(DEV), w.to(DEV), t.to(DEV)
    torch.cuda.synchronize()

    def rise(fn):
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        r = torch.cuda.max_memory_allocated() - base
        del out
        return r

    fused = rise(lambda: ops.lm_head_loss(xd, wd, td))
    with torch.no_grad():
        lib = rise(lambda: ops.lm_head_ce(xd, wd, td)[0])
    print(f"peak rise: fused {fused} B, lm_head_ce {lib} B, "
          f"logits {T * V * 2} B")
    # workspace: 8 B per (split, row) + 12 B per row, <= 64 vocab tiles
    assert fused < T * V * 2 // 8
    assert lib >= T * V * 2     # sanity check of the method


def test_graph_capture():
    from distributedtraining_amd import ops
    T, K, V = 130, 128, 1000
    x, w, t, _, _ = _case(T, K, V)
    x2 = _make(T, K, V, seed=7)[0]
    xs, wd, td = x.to(DEV), w.to(DEV), t.to(DEV)   # xs: static graph input
    x2d = x2.to(DEV)
    e1 = ops.lm_head_loss(xs, wd, td, return_lse=True)
    e2 = ops.lm_head_loss(x2d, wd, td, return_lse=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.lm_head_loss(xs, wd, td, return_lse=True)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss, lse = ops.lm_head_loss(xs, wd, td, return_lse=True)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(lse, e1[1])
    # loss_sum is folded with float atomics in ce_finalize: order-dependent
    torch.testing.assert_close(loss, e1[0], rtol=1e-5, atol=1e-5)
    xs.copy_(x2d)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(lse, e2[1])
    torch.testing.assert_close(loss, e2[0], rtol=1e-5, atol=1e-5)
    assert not torch.equal(e1[1], e2[1])


def test_unsupported_k_routes_to_library_path():
    from distributedtraining_amd import ops
    T, K, V = 130, 40, 1000
    x, w, t = _make(T, K, V)
    logits = x.float() @ w.float().t()
    ref = torch.nn.functional.cross_entropy(logits, t, ignore_index=II)
    loss, lse = ops.lm_head_loss(x.to(DEV), w.to(DEV), t.to(DEV),
                                 return_lse=True)
    torch.testing.assert_close(loss.cpu(), ref, rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(lse.cpu(), torch.logsumexp(logits, -1),
                               rtol=1e-2, atol=1e-2)
    with pytest.raises(RuntimeError, match="K % 64"):
        _ext().head_loss_fwd(x.to(DEV), w.to(DEV), t.to(DEV), II, 0)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_models_loss_only(family):
    from distributedtraining_amd.config import ModelConfig
    from distributedtraining_amd.models import build_model
    import dataclasses
    # llama_tiny with 2 heads: head dim 32, the smallest the GPU attention
    # kernel takes
    cfg = (ModelConfig.gpt2_tiny() if family == "gpt2"
           else dataclasses.replace(ModelConfig.llama_tiny(), n_head=2,
                                    n_kv_head=1))
    torch.manual_seed(0)
    model = build_model(cfg).to(DEV, torch.bfloat16).eval()
    ids = torch.randint(0, cfg.vocab_size, (4, 32)).to(DEV)
    am = torch.ones(4, 32, dtype=torch.long)
    am[1, 20:] = 0
    am = am.to(DEV)
    with torch.no_grad():
        full = model(input_ids=ids, attention_mask=am, labels=ids)
        lo = model(input_ids=ids, attention_mask=am, labels=ids,
                   loss_only=True)
    assert full.logits is not None and lo.logits is None
    print(f"{family}: default {float(full.loss):.6f} "
          f"loss_only {float(lo.loss):.6f}")
    torch.testing.assert_close(lo.loss.float(), full.loss.float(),
                               rtol=1e-3, atol=1e-3)


def test_validator_flag():
    from distributedtraining_amd.config import (Config, ModelConfig,
                                                ValidateConfig)
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.parallel.flat import FlatParams
    from distributedtraining_amd.roles.validator import DeltaValidator
    from distributedtraining_amd.store import DeltaCheckpoint
    from distributedtraining_amd.utils.data import synthetic_eval_set

    cfg = Config()
    cfg.model = ModelConfig.gpt2_tiny()
    ev = synthetic_eval_set(cfg.model.vocab_size, 2, 4, 32)
    res = {}
    for flag in (False, True):
        torch.manual_seed(0)
        model = build_model(cfg.model).to(DEV)
        fp = FlatParams(model)
        v = DeltaValidator(model, fp, ev, ValidateConfig(fused_head_loss=flag))
        g = torch.Generator().manual_seed(3)
        noise = torch.randn(fp.numel, generator=g)
        small = DeltaCheckpoint(noise * 0.02, fp.spec, "")
        big = DeltaCheckpoint(noise * 0.3, fp.spec, "")
        res[flag] = (v.base_loss, v.score_delta(small)[0],
                     v.score_delta(big)[0])
    print(f"validator (base, small, big): off {res[False]} on {res[True]}")
    assert res[True][0] == pytest.approx(res[False][0], rel=1e-3, abs=1e-3)
    assert (res[True][1] < res[True][2]) == (res[False][1] < res[False][2])
    assert abs(res[False][1] - res[False][2]) > 1e-2   # ordering is not a tie
