"""Gathered deltas kept in wire form (parallel.comm.PackedDeltas), CPU side:
the container against the comm.py quantiser, the ops fallbacks against the
tensor path on the dequantised stack, and the LocalSGDNode wiring of
comm.resident_dtype = "wire" over gloo."""

import os

import pytest
import torch
import torch.multiprocessing as mp

SEGS = [1000, 37, 4096, 123]


def _inputs(seed=31, N=3):
    g = torch.Generator().manual_seed(seed)
    P = sum(SEGS)
    offsets = torch.tensor([0] + list(torch.tensor(SEGS).cumsum(0)))
    base = torch.randn(P, generator=g)
    deltas = torch.randn(N, P, generator=g) * 1e-3
    W = torch.rand(N, len(SEGS), generator=g)
    grad = torch.randn(P, generator=g)
    return P, offsets, base, deltas, W, grad


@pytest.mark.parametrize("block", [256, 4096])
def test_packed_int8_row_and_dequantize(block):
    from distributedtraining_amd.parallel.comm import (
        PackedDeltas, dequantize_blockwise_int8, quantize_blockwise_int8)
    P, _, _, deltas, _, _ = _inputs()
    pd = PackedDeltas.pack(deltas, "int8", block)
    nb = (P + block - 1) // block
    assert pd.shape == (3, P) and pd.kind == "int8"
    assert pd.data.dtype == torch.int8 and pd.data.shape == (3, nb * block)
    assert pd.scales.shape == (3, nb)
    for i in range(3):
        q, s = quantize_blockwise_int8(deltas[i], block)
        assert torch.equal(pd.data[i], q) and torch.equal(pd.scales[i], s)
        want = dequantize_blockwise_int8(q, s, P, block)
        row = pd.row(i)
        assert row.dtype == torch.float32 and row.shape == (P,)
        assert torch.equal(row, want)
        assert torch.equal(pd.dequantize()[i], want)


def test_packed_bf16_and_fp32_rows():
    from distributedtraining_amd.parallel.comm import PackedDeltas
    P, _, _, deltas, _, _ = _inputs()
    pb = PackedDeltas.pack(deltas, "bf16")
    assert pb.shape == (3, P) and pb.data.dtype == torch.bfloat16
    assert torch.equal(pb.dequantize(), deltas.to(torch.bfloat16).float())
    pf = PackedDeltas.pack(deltas, "fp32")
    assert torch.equal(pf.dequantize(), deltas)
    row = pf.row(1)
    row.zero_()                       # a fresh tensor, not a view
    assert torch.equal(pf.data[1], deltas[1])


def test_packed_rejects_bad_layout():
    from distributedtraining_amd.parallel.comm import PackedDeltas
    with pytest.raises(ValueError):
        PackedDeltas("int4", torch.zeros(1, 8), 8)
    with pytest.raises(ValueError):      # codes not nb*block wide
        PackedDeltas("int8", torch.zeros(2, 100, dtype=torch.int8), 100,
                     torch.ones(2, 1), 256)
    with pytest.raises(ValueError):      # wrong dtype for the kind
        PackedDeltas("bf16", torch.zeros(2, 8), 8)


def test_ops_quantize_cpu_is_the_comm_definition():
    from distributedtraining_amd import ops
    from distributedtraining_amd.parallel import comm
    g = torch.Generator().manual_seed(5)
    w = torch.randn(3 * 256 + 17, generator=g)
    base = torch.randn(3 * 256 + 17, generator=g)
    q, s = ops.quantize_blockwise_int8(w, 256)
    q0, s0 = comm.quantize_blockwise_int8(w, 256)
    assert torch.equal(q, q0) and torch.equal(s, s0)
    q, s = ops.quantize_blockwise_int8(w, 256, base=base)
    q0, s0 = comm.quantize_blockwise_int8(w - base, 256)
    assert torch.equal(q, q0) and torch.equal(s, s0)
    assert torch.equal(
        ops.dequantize_blockwise_int8(q, s, w.numel(), 256),
        comm.dequantize_blockwise_int8(q0, s0, w.numel(), 256))


@pytest.mark.parametrize("kind,block", [("int8", 256), ("int8", 4096),
                                        ("bf16", 4096), ("fp32", 4096)])
def test_ops_on_packed_equal_tensor_path(kind, block):
    from distributedtraining_amd import ops
    from distributedtraining_amd.parallel.comm import PackedDeltas
    P, offsets, base, deltas, W, grad = _inputs()
    pd = PackedDeltas.pack(deltas, kind, block)
    dense = pd.dequantize()
    if kind != "fp32":
        assert not torch.equal(dense, deltas)      # it did compress
    merged = ops.weighted_merge(base, dense, W, offsets)
    assert torch.equal(ops.weighted_merge(base, pd, W, offsets), merged)
    assert torch.equal(
        ops.grad_merge_weights(grad, base, pd, merged, offsets),
        ops.grad_merge_weights(grad, base, dense, merged, offsets))
    for alpha in (1.0, -0.37):
        w0 = base.clone()
        w1 = base.clone()
        ops.axpy_(w0, dense[2], alpha)
        assert ops.axpy_(w1, (pd, 2), alpha) is w1
        assert torch.equal(w1, w0)


def _node(rank, cfg, merge_strategy):
    import torch
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.parallel.comm import CommPlane
    from distributedtraining_amd.parallel.flat import FlatParams
    from distributedtraining_amd.parallel.local_sgd import LocalSGDNode
    from distributedtraining_amd.utils.data import (synthetic_batches,
                                                    synthetic_eval_set)
    torch.manual_seed(100 + rank)
    model = build_model(cfg.model)
    fp = FlatParams(model)
    comm = CommPlane(backend="gloo", device=torch.device("cpu"))
    data = synthetic_batches(cfg.model.vocab_size, 2, 16, seed=rank)
    ev = synthetic_eval_set(cfg.model.vocab_size, 2, 2, 16)
    node = LocalSGDNode(model, fp, data, cfg, comm, val_batches=ev,
                        merge_strategy=merge_strategy)
    return node, fp, comm


def _wire_worker(rank, world, port, q):
    os.environ.update({
        "RANK": str(rank), "WORLD_SIZE": str(world),
        "LOCAL_RANK": str(rank), "MASTER_ADDR": "127.0.0.1",
        "MASTER_PORT": str(port),
    })
    import torch
    from distributedtraining_amd.config import (Config, ModelConfig,
                                                TrainConfig)
    from distributedtraining_amd.parallel.comm import PackedDeltas
    try:
        cfg = Config()
        cfg.model = ModelConfig.gpt2_tiny()
        cfg.train = TrainConfig(batch_size=2, seq_len=16,
                                send_interval_steps=10**9,
                                pull_interval_steps=0)
        cfg.comm.exchange_dtype = "int8"
        assert cfg.comm.resident_dtype == "fp32"       # the default
        node, fp, comm = _node(rank, cfg, "score_weighted")
        node.sync_initial_base()
        node.train_steps(2)
        state = fp.master.clone()
        base = node.miner.base.clone()
        scores = [1.0, 3.0]

        def run(resident):
            """validation scores and the merged base, from the same state"""
            cfg.comm.resident_dtype = resident
            node.miner.install_base(base.clone())
            fp.load_flat_master(state)
            gathered = node._gather_deltas(
                node._local_delta(node.miner.base), node.miner.base)
            val = node.validation_round()
            kept = torch.equal(fp.master, state)
            node.merge_round(scores=scores)
            return gathered, val, fp.master.clone(), kept

        g32, val32, merged32, kept32 = run("fp32")
        gw, valw, mergedw, keptw = run("wire")
        ok_types = (isinstance(g32, torch.Tensor)
                    and g32.dtype == torch.float32
                    and g32.shape == (world, fp.numel)
                    and isinstance(gw, PackedDeltas) and gw.kind == "int8"
                    and gw.data.dtype == torch.int8
                    and gw.shape == (world, fp.numel))
        ok_rows = torch.equal(gw.dequantize(), g32)
        ok_merge = torch.equal(mergedw, merged32)
        moved = not torch.equal(merged32, state)
        q.put((rank, bool(ok_types and ok_rows and ok_merge and moved
                          and kept32 and keptw),
               tuple(sorted(val32.items())), tuple(sorted(valw.items())),
               float(mergedw.sum())))
        comm.close()
    except Exception as e:  # pragma: no cover
        q.put((rank, False, repr(e), None, None))
        raise


@pytest.mark.timeout(300)
def test_int8_wire_resident_merge_and_validation():
    """exchange int8 + resident "wire", world 2: the gather is a PackedDeltas
    whose rows are the fp32-resident gather's; merge_round(score_weighted)
    gives the bit-identical base; validation_round gives the same scores
    dict as resident "fp32" from the same state."""
    world = 2
    port = 29897
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_wire_worker, args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok, *_ in results), results
    for _, _, val32, valw, _ in results:
        print("validation fp32-resident:", val32)
        print("validation wire-resident:", valw)
        assert valw == val32
    assert results[0][2] == results[1][2], "ranks disagree on scores"
    assert results[0][4] == results[1][4], "ranks diverged after merge"


def test_default_gather_is_fp32_tensor():
    """resident_dtype defaults to "fp32": _gather_deltas returns the [world,
    P] fp32 tensor it always did, at every wire dtype."""
    from distributedtraining_amd.config import (Config, ModelConfig,
                                                TrainConfig)
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.parallel.comm import CommPlane, PackedDeltas
    from distributedtraining_amd.parallel.flat import FlatParams
    from distributedtraining_amd.parallel.local_sgd import LocalSGDNode
    from distributedtraining_amd.utils.data import synthetic_batches
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    cfg = Config()
    assert cfg.comm.resident_dtype == "fp32"
    cfg.model = ModelConfig.gpt2_tiny()
    cfg.train = TrainConfig(batch_size=2, seq_len=16,
                            send_interval_steps=10**9, pull_interval_steps=0)
    torch.manual_seed(0)
    model = build_model(cfg.model)
    fp = FlatParams(model)
    comm = CommPlane(device=torch.device("cpu"))
    node = LocalSGDNode(model, fp, synthetic_batches(cfg.model.vocab_size,
                                                     2, 16, seed=0),
                        cfg, comm, merge_strategy="score_weighted")
    flat = torch.randn(fp.numel) * 1e-3
    for wire in ("fp32", "bf16", "int8"):
        cfg.comm.exchange_dtype = wire
        got = node._gather_deltas(flat)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32
        assert got.shape == (1, fp.numel)
    cfg.comm.resident_dtype = "wire"
    for wire in ("fp32", "bf16", "int8"):
        cfg.comm.exchange_dtype = wire
        got = node._gather_deltas(flat)
        assert isinstance(got, PackedDeltas) and got.kind == wire
        assert got.shape == (1, fp.numel)
    cfg.comm.resident_dtype = "int8"
    with pytest.raises(ValueError):
        node._gather_deltas(flat)
