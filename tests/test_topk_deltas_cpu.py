"""Top-k sparse delta exchange on the CPU: the definition
(comm.topk_compress_blockwise), the "topk" kind of PackedDeltas, the CPU ops
on it, the two-rank gloo merge / validation rounds and the config checks.
Every comparison is exact."""

import hashlib
import os

import pytest
import torch
import torch.multiprocessing as mp

import _topk_cases as tc
from distributedtraining_amd import ops
from distributedtraining_amd.parallel import comm
from distributedtraining_amd.parallel.comm import PackedDeltas

SEGS = [1000, 37, 4096, 123]


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------
# Definition
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("P,block,k", tc.SHAPES)
def test_definition_ties_order_and_identity(P, block, k):
    x, info = tc.crafted(P, block, k)
    ent, res = comm.topk_compress_blockwise(x, k, block)
    nb = (P + block - 1) // block
    assert ent.dtype == torch.int32 and ent.shape == (nb * k,)
    assert res.dtype == torch.float32 and res.shape == (P,)
    idx = tc.entry_index(ent, k, block)
    # entries ascend inside every block
    assert bool((idx[:, 1:] > idx[:, :-1]).all())
    # block 0: every larger value, then the tie group cut by index order
    members, keep = info["members"], info["keep"]
    assert 0 < keep < len(members)
    assert idx[0].tolist() == sorted(info["big"] + members[:keep])
    assert all(float(res[o]) == float(x[o]) for o in members[keep:])
    assert all(float(res[o]) == 0.0 for o in members[:keep])   # 5.0 is bf16
    # densify + residual == d wherever d is finite
    dense = comm.topk_densify(ent, k, P, block)
    fin = torch.isfinite(x)
    assert torch.equal((dense + res)[fin], x[fin])
    assert torch.equal(_bits(dense),
                       _bits(tc.hand_scatter(ent, k, block, P)))
    # out-of-range entries of a ragged tail carry zero value bits
    past = idx >= P
    assert bool(((ent.view(-1, k) & 0xFFFF)[past] == 0).all())
    if P % block and P % block < k:
        assert int(past.sum()) == k - P % block
    else:
        assert not bool(past.any())
    # a second round fed the residual alone keeps the identity
    ent2, res2 = comm.topk_compress_blockwise(
        torch.zeros(P), k, block, residual=res)
    dense2 = comm.topk_densify(ent2, k, P, block)
    assert torch.equal(dense2 + res2, res)
    assert bool(torch.isfinite(res).all())


def test_definition_near_equal_zero_sparse_and_poison():
    P, block, k = tc.SHAPES[0]
    x, info = tc.crafted(P, block, k)
    ent, res = comm.topk_compress_blockwise(x, k, block)
    idx = tc.entry_index(ent, k, block)
    # block 1: the k largest of the 1 + j 2^-23 values, lower index on ties
    near = info["near"]
    order = sorted(near, key=lambda o: (-abs(float(x[o])), o))
    assert idx[1].tolist() == sorted(order[:k])
    # block 2, all zeros: ties everywhere, the first k indices win
    assert idx[2].tolist() == list(range(2 * block, 2 * block + k))
    # block 3: fewer than k non-zeros, all kept; NaN and inf kept, residual 0
    sp = info["special"]
    kept = set(idx[3].tolist())
    assert set(sp["nonzero"]) <= kept
    v = (ent.view(-1, k)[3] & 0xFFFF).tolist()
    at = {e: b for e, b in zip(idx[3].tolist(), v)}
    assert at[sp["nan"]] == 0x7FC0 and at[sp["inf"]] == 0x7F80
    assert float(res[sp["nan"]]) == 0.0 and float(res[sp["inf"]]) == 0.0
    # the denormal is kept (it is among the few non-zeros); bf16 keeps the
    # top bits of its mantissa and the remainder stays behind, exactly
    d = float(x[sp["denormal"]])
    sent = float(comm.topk_densify(ent, k, P, block)[sp["denormal"]])
    assert sent + float(res[sp["denormal"]]) == d and sent != 0.0


def test_definition_rejects_bad_format():
    x = torch.zeros(5000)
    for k, block in [(6, 4096), (0, 4096), (1028, 4096), (128, 512),
                     (128, 3000), (128, 32768)]:
        with pytest.raises(ValueError):
            comm.topk_compress_blockwise(x, k, block)


# ---------------------------------------------------------------------------
# Container
# ---------------------------------------------------------------------------
def _stack(P, block, k, N=3):
    g = torch.Generator().manual_seed(P + block)
    d = torch.randn(N, P, generator=g) * 1e-3
    d[1, ::7] = 0.0
    return d


def test_container_checks_and_rows():
    P, block, k = 5 * 1024 + 1, 1024, 8
    d = _stack(P, block, k)
    pd = PackedDeltas.pack(d, "topk", block=block, k=k)
    nb = 6
    assert pd.kind == "topk" and pd.data.dtype == torch.int32
    assert tuple(pd.data.shape) == (3, nb * k) and pd.shape == (3, P)
    for i in range(3):
        ent, _ = comm.topk_compress_blockwise(d[i], k, block)
        assert torch.equal(pd.data[i], ent)
        assert torch.equal(_bits(pd.row(i)),
                           _bits(tc.hand_scatter(ent, k, block, P)))
    assert torch.equal(pd.dequantize(),
                       torch.stack([pd.row(i) for i in range(3)]))
    with pytest.raises(ValueError):      # wrong dtype
        PackedDeltas("topk", pd.data.to(torch.int64), P, None, block, k)
    with pytest.raises(ValueError):      # wrong shape
        PackedDeltas("topk", pd.data[:, :-k], P, None, block, k)
    with pytest.raises(ValueError):      # k % 4
        PackedDeltas("topk", torch.zeros(3, nb * 6, dtype=torch.int32), P,
                     None, block, 6)
    with pytest.raises(ValueError):      # k > block / 4
        PackedDeltas("topk", torch.zeros(3, nb * 260, dtype=torch.int32), P,
                     None, block, 260)


# ---------------------------------------------------------------------------
# CPU ops
# ---------------------------------------------------------------------------
def test_cpu_ops_equal_tensor_path():
    P, block, k = sum(SEGS), 1024, 32
    offsets = torch.tensor([0] + list(torch.tensor(SEGS).cumsum(0)))
    d = _stack(P, block, k)
    pd = PackedDeltas.pack(d, "topk", block=block, k=k)
    dense = pd.dequantize()
    g = torch.Generator().manual_seed(3)
    base = torch.randn(P, generator=g)
    W = torch.rand(3, len(SEGS), generator=g)
    grad = torch.randn(P, generator=g)
    merged = ops.weighted_merge(base, pd, W, offsets)
    assert torch.equal(merged, ops.weighted_merge(base, dense, W, offsets))
    assert not torch.equal(merged, base)
    assert torch.equal(
        ops.grad_merge_weights(grad, base, pd, merged, offsets),
        ops.grad_merge_weights(grad, base, dense, merged, offsets))
    for alpha in (1.0, -0.5):
        w1, w2 = base.clone(), base.clone()
        ops.axpy_(w1, (pd, 1), alpha)
        ops.axpy_(w2, dense[1], alpha)
        assert torch.equal(w1, w2)


def test_cpu_compress_modes():
    P, block, k = tc.SHAPES[2]
    x, _ = tc.crafted(P, block, k)
    base, residual = tc.crafted_base_residual(P, block, k)
    w = base + x
    ent0, res0 = comm.topk_compress_blockwise((w - base), k, block, residual)
    r = residual.clone()
    ent, out = ops.topk_compress_blockwise(w, k, block, base=base,
                                           residual=r)
    assert out is r and torch.equal(ent, ent0)
    assert torch.equal(_bits(r), _bits(res0))
    r = residual.clone()
    ent, out = ops.topk_compress_blockwise(w, k, block, base=base,
                                           residual=r, update_residual=False)
    assert torch.equal(ent, ent0) and torch.equal(_bits(r), _bits(residual))
    ent, out = ops.topk_compress_blockwise(x, k, block)
    e1, r1 = comm.topk_compress_blockwise(x, k, block)
    assert torch.equal(ent, e1) and torch.equal(_bits(out), _bits(r1))


# ---------------------------------------------------------------------------
# Config
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,block", [(6, 4096), (0, 4096), (2048, 4096),
                                     (128, 512), (128, 5000), (128, 32768)])
def test_config_rejects_bad_topk_values(k, block):
    from distributedtraining_amd.config import Config, ModelConfig
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.parallel.comm import CommPlane
    from distributedtraining_amd.parallel.flat import FlatParams
    from distributedtraining_amd.parallel.local_sgd import LocalSGDNode
    from distributedtraining_amd.utils.data import synthetic_batches
    cfg = Config()
    assert cfg.comm.topk_k == 128 and cfg.comm.topk_block == 4096
    assert cfg.comm.topk_error_feedback is True
    cfg.model = ModelConfig.gpt2_tiny()
    cfg.comm.exchange_dtype = "topk"
    cfg.comm.topk_k, cfg.comm.topk_block = k, block
    model = build_model(cfg.model)
    fp = FlatParams(model)
    plane = CommPlane(device=torch.device("cpu"))
    data = synthetic_batches(cfg.model.vocab_size, 2, 16)
    with pytest.raises(ValueError):
        LocalSGDNode(model, fp, data, cfg, plane)


# ---------------------------------------------------------------------------
# Two gloo ranks
# ---------------------------------------------------------------------------
def _node_worker(rank, world, port, resident, k, block, q):
    os.environ.update({
        "RANK": str(rank), "WORLD_SIZE": str(world),
        "LOCAL_RANK": str(rank), "MASTER_ADDR": "127.0.0.1",
        "MASTER_PORT": str(port),
    })
    import torch
    from distributedtraining_amd import ops
    from distributedtraining_amd.config import (Config, ModelConfig,
                                                TrainConfig)
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.parallel import comm as cm
    from distributedtraining_amd.parallel.flat import FlatParams
    from distributedtraining_amd.parallel.local_sgd import LocalSGDNode
    from distributedtraining_amd.utils.data import (synthetic_batches,
                                                    synthetic_eval_set)
    try:
        cfg = Config()
        cfg.model = ModelConfig.gpt2_tiny()
        cfg.train = TrainConfig(batch_size=2, seq_len=16,
                                send_interval_steps=10**9,
                                pull_interval_steps=0)
        cfg.comm.exchange_dtype = "topk"
        cfg.comm.resident_dtype = resident
        cfg.comm.topk_k, cfg.comm.topk_block = k, block
        torch.manual_seed(100 + rank)
        model = build_model(cfg.model)
        fp = FlatParams(model)
        plane = cm.CommPlane(backend="gloo", device=torch.device("cpu"))
        data = synthetic_batches(cfg.model.vocab_size, 2, 16, seed=rank)
        ev = synthetic_eval_set(cfg.model.vocab_size, 1, 2, 16)
        node = LocalSGDNode(model, fp, data, cfg, plane, val_batches=ev,
                            merge_strategy="score_weighted")
        node.sync_initial_base()
        P = fp.master.numel()
        checks = {}

        def expected_round(residual):
            base = node.miner.base
            ent, res = cm.topk_compress_blockwise(
                fp.master - base, k, block, residual)
            rows = plane.all_gather_flat(ent)
            dense = torch.stack([cm.topk_densify(rows[r], k, P, block)
                                 for r in range(world)])
            W = torch.full((world, len(fp.spec)), 1.0 / world)
            return ops.weighted_merge(base, dense, W, fp.offsets), res

        node.train_steps(2)
        base0 = node.miner.base.clone()
        merged, res = expected_round(torch.zeros(P))
        node.merge_round(scores=[1.0] * world)
        checks["merge1"] = torch.equal(fp.master, merged)
        checks["moved"] = not torch.equal(merged, base0)
        checks["residual1"] = torch.equal(
            node.residual.view(torch.int32), res.view(torch.int32))
        checks["residual_nonzero"] = bool(node.residual.abs().sum() > 0)

        node.train_steps(1)
        before = node.residual.clone()
        scores = node.validation_round()
        checks["validation_keeps_residual"] = torch.equal(
            node.residual.view(torch.int32), before.view(torch.int32))
        checks["scores"] = len(scores) == world

        merged, res = expected_round(before)
        node.merge_round(scores=[1.0] * world)
        checks["merge2"] = torch.equal(fp.master, merged)
        checks["residual2"] = torch.equal(
            node.residual.view(torch.int32), res.view(torch.int32))
        digest = hashlib.sha1(fp.master.numpy().tobytes()).hexdigest()
        q.put((rank, checks, digest))
        plane.close()
    except Exception as e:  # pragma: no cover
        q.put((rank, {"exception": False, "what": repr(e)}, ""))
        raise


@pytest.mark.timeout(300)
@pytest.mark.parametrize("resident,k,block,port", [
    ("wire", 128, 4096, 29911), ("fp32", 32, 1024, 29923)])
def test_gloo_merge_and_validation_rounds(resident, k, block, port):
    """score_weighted merge rounds with a validation round between them:
    the merged base is the one the definition gives from both ranks'
    deltas, identical on both ranks; the residual is the definition's, and
    a validation round leaves it bit-identical."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_node_worker,
                         args=(r, world, port, resident, k, block, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    for _, checks, _ in results:
        assert all(bool(v) for v in checks.values()), results
    assert results[0][2] == results[1][2], "ranks diverged after merge"
