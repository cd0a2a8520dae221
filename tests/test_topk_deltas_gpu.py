"""Top-k sparse deltas on the GPU (merge.hip): the compressor against the CPU
definition bit for bit, weighted_merge / grad_W / axpy on "topk" storage
against the fp32 kernels on the densified rows, and one node-level round.
No tolerance anywhere: every comparison is bit (or, for axpy, number)
equality."""

import functools

import pytest
import torch

import _topk_cases as tc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEGS = [1000, 37, 4096, 123]     # boundaries inside blocks and 16 B vectors
SEGS_TAIL = [1000, 37, 4096, 3]  # 16 elements in the last 1024-block: < k
SEGS_WIDE = SEGS + [12000]       # three 8192-blocks, each wider than a tile
GUARD = 64


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------
# Compressor
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(P, block, k, mode):
    """CPU definition for one mode: (w, base, residual, entries, res)."""
    from distributedtraining_amd.parallel import comm
    x, _ = tc.crafted(P, block, k)
    base = residual = None
    w = x
    if mode != "plain":
        base, r = tc.crafted_base_residual(P, block, k)
        w = base + x
        if mode != "base":
            residual = r
    ent, res = comm.topk_compress_blockwise(
        w if base is None else w - base, k, block, residual)
    return w, base, residual, ent, res


@pytest.mark.parametrize("P,block,k", tc.SHAPES)
def test_crafted_tie_group_straddles_the_cut(P, block, k):
    """What the crafted block 0 is for, under the CPU definition: in every
    mode some members of the tie group are kept and some are dropped, and
    the kept ones are the lowest indices."""
    _, info = tc.crafted(P, block, k)
    members, keep = info["members"], info["keep"]
    for mode in ("plain", "base", "both"):
        _, _, _, ent, _ = _reference(P, block, k, mode)
        kept = set(tc.entry_index(ent, k, block)[0].tolist())
        assert [m for m in members if m in kept] == members[:keep]
        assert 0 < keep < len(members)


@pytest.mark.parametrize("mode", ["plain", "base", "both", "frozen"])
@pytest.mark.parametrize("P,block,k", tc.SHAPES)
def test_compressor_equals_cpu_definition(P, block, k, mode):
    from distributedtraining_amd import ops
    frozen = mode == "frozen"       # update_residual=False
    w, base, residual, ent, res = _reference(
        P, block, k, "both" if frozen else mode)
    wd = w.to(DEV)
    bd = None if base is None else base.to(DEV)
    rd = None if residual is None else residual.to(DEV)
    got, out = ops.topk_compress_blockwise(
        wd, k, block, base=bd, residual=rd, update_residual=not frozen)
    assert got.dtype == torch.int32
    assert torch.equal(got.cpu(), ent)
    if frozen:
        assert out is rd
        assert torch.equal(_bits(rd.cpu()), _bits(residual))
    else:
        if rd is not None:
            assert out is rd          # rewritten in place
        assert torch.equal(_bits(out.cpu()), _bits(res))


def test_bindings_reject_bad_arguments():
    """The top-k form goes through the extension's packed entry points:
    quantize_int8 with topk_k > 0 makes the entries, and int32 data selects
    the sparse consumers."""
    from distributedtraining_amd.ops.backend import require_ext
    ext = require_ext()
    x = torch.zeros(5000, device=DEV)
    e = x.new_empty(0)
    s0 = torch.empty(0, device=DEV)
    for k, block in [(6, 4096), (-4, 4096), (1028, 4096), (128, 512),
                     (128, 3000), (128, 32768)]:
        with pytest.raises(RuntimeError):
            ext.quantize_int8(x, e, block, topk_k=k)
    with pytest.raises(RuntimeError):      # base of another length
        ext.quantize_int8(x, x[:-1], 4096, topk_k=128)
    with pytest.raises(RuntimeError):      # residual of another length
        ext.quantize_int8(x, e, 4096, topk_k=128, residual_in=x[:-4])
    with pytest.raises(RuntimeError):      # a residual without top-k
        ext.quantize_int8(x, e, 4096, residual_out=x.clone())
    ent, = ext.quantize_int8(x, e, 4096, topk_k=128)
    assert ent.dtype == torch.int32 and tuple(ent.shape) == (2 * 128,)
    w = torch.zeros(5000, device=DEV)
    good = ent.view(1, -1)
    ext.axpy_packed(w, good, s0, 4096, 0, 1.0)
    with pytest.raises(RuntimeError):      # k = 130 / 2 = 65: not % 4
        ext.axpy_packed(w, good[:, :130].contiguous(), s0, 4096, 0, 1.0)
    with pytest.raises(RuntimeError):      # 129 columns: no whole k
        ext.axpy_packed(w, good[:, :129].contiguous(), s0, 4096, 0, 1.0)
    with pytest.raises(RuntimeError):      # dtype
        ext.axpy_packed(w, good.to(torch.int64), s0, 4096, 0, 1.0)
    with pytest.raises(RuntimeError):      # row
        ext.axpy_packed(w, good, s0, 4096, 1, 1.0)
    with pytest.raises(RuntimeError):      # block
        ext.axpy_packed(w, good, s0, 512, 0, 1.0)


# ---------------------------------------------------------------------------
# Consumers
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plane(block, k, segs=tuple(SEGS)):
    """Three rows on the plane cut into ``segs``. Row 1 is the crafted input
    (ties; NaN and inf taken out). On SEGS_TAIL the last block has fewer
    than k in-range elements, so every row ends in entries that point past
    P; row 2's get non-zero value bits there, which a consumer without the
    bounds check would write into the guard region. Returns CPU tensors."""
    from distributedtraining_amd.parallel.comm import PackedDeltas
    P = sum(segs)
    g = torch.Generator().manual_seed(block + k)
    d = torch.randn(3, P, generator=g) * 1e-3
    x, _ = tc.crafted(P, block, k)
    d[1] = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    d[2, (P // block) * block:] = 0.0      # tail block: all ties at zero
    d[2, P - 1] = 3e-3
    pd = PackedDeltas.pack(d, "topk", block=block, k=k)
    past = tc.entry_index(pd.data[2], k, block).view(-1) >= P
    assert bool(past.any()) == (P % block < k)
    pd.data[2, past] |= 0x3F80            # 1.0 where nothing may be written
    offsets = torch.tensor([0] + torch.tensor(segs).cumsum(0).tolist())
    base = torch.randn(P, generator=g)
    W = torch.rand(3, len(segs), generator=g)
    grad = torch.randn(P, generator=g)
    return pd, offsets, base, W, grad


def _to_dev(pd):
    from distributedtraining_amd.parallel.comm import PackedDeltas
    return PackedDeltas("topk", pd.data.to(DEV), pd.numel, None, pd.block,
                        pd.k)


def _guarded(t):
    """A device copy of ``t`` followed by a guard region, as (view, whole)."""
    whole = torch.full((t.numel() + GUARD,), 777.0, device=DEV)
    whole[:t.numel()] = t.to(DEV)
    return whole[:t.numel()], whole


# the last one: a block of two 4096-element LDS tiles, the path of every
# block above 4096
CONSUMER_FORMATS = [(1024, 32, tuple(SEGS)), (4096, 128, tuple(SEGS)),
                    (1024, 32, tuple(SEGS_TAIL)),
                    (8192, 64, tuple(SEGS_WIDE))]


@pytest.mark.parametrize("block,k,segs", CONSUMER_FORMATS)
def test_row_and_dequantize_equal_cpu_scatter(block, k, segs):
    pd, *_ = _plane(block, k, segs)
    got = _to_dev(pd).dequantize().cpu()
    assert torch.equal(_bits(got), _bits(pd.dequantize()))
    for i in range(3):
        assert torch.equal(_bits(pd.row(i)), _bits(
            tc.hand_scatter(pd.data[i], k, block, pd.numel)))


@pytest.mark.parametrize("block,k,segs", CONSUMER_FORMATS)
def test_topk_merge_equals_fp32_kernel(block, k, segs):
    from distributedtraining_amd import ops
    pd, offsets, base, W, _ = _plane(block, k, segs)
    pdd = _to_dev(pd)
    dense = pdd.dequantize()
    bd, Wd = base.to(DEV), W.to(DEV)
    want = ops.weighted_merge(bd, dense, Wd, offsets)
    out, whole = _guarded(torch.zeros(pd.numel))
    ops.weighted_merge(bd, pdd, Wd, offsets, out=out)
    assert torch.equal(out, want)
    assert not torch.equal(out, bd)
    assert bool((whole[pd.numel:] == 777.0).all())


@pytest.mark.parametrize("g_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("block,k,segs", CONSUMER_FORMATS)
def test_topk_grad_w_equals_fp32_kernel(block, k, segs, g_dtype):
    from distributedtraining_amd import ops
    pd, offsets, base, W, grad = _plane(block, k, segs)
    pdd = _to_dev(pd)
    dense = pdd.dequantize()
    bd, gd = base.to(DEV), grad.to(DEV).to(g_dtype)
    merged = ops.weighted_merge(bd, dense, W.to(DEV), offsets)
    want = ops.grad_merge_weights(gd, bd, dense, merged, offsets)
    got = ops.grad_merge_weights(gd, bd, pdd, merged, offsets)
    assert torch.equal(got, want)
    assert bool((got != 0).all())


@pytest.mark.parametrize("alpha", [1.0, -0.5])
@pytest.mark.parametrize("block,k,segs", CONSUMER_FORMATS)
def test_topk_axpy_equals_fp32_kernel(block, k, segs, alpha):
    from distributedtraining_amd import ops
    pd, _, base, _, _ = _plane(block, k, segs)
    pdd = _to_dev(pd)
    dense = pdd.dequantize()
    assert not bool(((base == 0) & torch.signbit(base)).any())
    for row in range(3):
        w, whole = _guarded(base)
        ops.axpy_(w, (pdd, row), alpha)
        want = ops.axpy_(base.to(DEV), dense[row], alpha)
        assert torch.equal(w, want)
        assert bool((whole[pd.numel:] == 777.0).all())


def test_nan_entry_reaches_merged_and_w():
    from distributedtraining_amd import ops
    from distributedtraining_amd.parallel.comm import PackedDeltas
    block, k = 1024, 32
    pd, offsets, base, W, _ = _plane(block, k)
    d = pd.dequantize()
    poison = 1000 + 37 + 2000            # inside the 4096-long segment
    d[1, poison] = float("nan")
    pdd = _to_dev(PackedDeltas.pack(d, "topk", block=block, k=k))
    bd = base.to(DEV)
    merged = ops.weighted_merge(bd, pdd, W.to(DEV), offsets)
    bad = torch.isnan(merged).nonzero().view(-1).tolist()
    assert bad == [poison]
    dense_way = ops.weighted_merge(bd, pdd.dequantize(), W.to(DEV), offsets)
    assert torch.equal(torch.nan_to_num(merged, nan=7.0),
                       torch.nan_to_num(dense_way, nan=7.0))
    w = bd.clone()
    ops.axpy_(w, (pdd, 1), 1.0)
    assert torch.isnan(w).nonzero().view(-1).tolist() == [poison]


# ---------------------------------------------------------------------------
# Node level
# ---------------------------------------------------------------------------
def test_node_round_on_one_gpu():
    from distributedtraining_amd import ops
    from distributedtraining_amd.config import (Config, ModelConfig,
                                                TrainConfig)
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.parallel import comm as cm
    from distributedtraining_amd.parallel.flat import FlatParams
    from distributedtraining_amd.parallel.local_sgd import LocalSGDNode
    from distributedtraining_amd.utils.data import (synthetic_batches,
                                                    synthetic_eval_set)
    cfg = Config()
    cfg.model = ModelConfig.gpt2_tiny()
    cfg.train = TrainConfig(batch_size=2, seq_len=16,
                            send_interval_steps=10**9, pull_interval_steps=0)
    cfg.comm.exchange_dtype = "topk"
    cfg.comm.resident_dtype = "wire"
    k, block = cfg.comm.topk_k, cfg.comm.topk_block
    torch.manual_seed(100)
    model = build_model(cfg.model).to(DEV)
    fp = FlatParams(model)
    plane = cm.CommPlane(device=torch.device(DEV))
    data = synthetic_batches(cfg.model.vocab_size, 2, 16, seed=0)
    ev = synthetic_eval_set(cfg.model.vocab_size, 1, 2, 16)
    node = LocalSGDNode(model, fp, data, cfg, plane, val_batches=ev,
                        merge_strategy="score_weighted")
    node.sync_initial_base()
    node.train_steps(2)
    P = fp.master.numel()
    base = node.miner.base.clone()
    master = fp.master.clone()
    ent, res = cm.topk_compress_blockwise(
        ops.delta_sub(master, base).cpu(), k, block, torch.zeros(P))
    dense = cm.topk_densify(ent, k, P, block).view(1, P).to(DEV)
    W = torch.ones(1, len(fp.spec), device=DEV)
    want = ops.weighted_merge(base, dense, W, fp.offsets)

    node.merge_round(scores=[1.0])
    assert torch.equal(fp.master, want)
    assert bool(torch.isfinite(fp.master).all())
    assert not torch.equal(fp.master, base)
    assert torch.equal(_bits(node.residual.cpu()), _bits(res))
    node.train_steps(1)
    before = node.residual.clone()
    scores = node.validation_round()
    assert torch.equal(_bits(node.residual), _bits(before))
    assert list(scores) == ["rank0"]
    assert all(s == s and abs(s) != float("inf") for s in scores.values())
