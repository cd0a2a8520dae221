"""ops.trimmed_merge on the CPU (the definition the kernel is held to) and the
layers above it: averager strategy, config flags, the gather path of local
SGD over gloo.

The fp64 bound, with u = 2^-24, m kept values v_j, mean = fl(fl(sum) / m):
the m - 1 adds each err by at most u |partial sum| <= u sum|v|, the division
by u |mean| and the final add by u |base + mean|, so
    |out - exact| <= u ((m - 1) sum|v| / m + |mean| + |base + mean|)
up to terms in u^2, which the 1e-3 relative slack covers.
"""

import os

import pytest
import torch
import torch.multiprocessing as mp

import _robust_cases as rc

from distributedtraining_amd import ops
from distributedtraining_amd.parallel.comm import PackedDeltas

P_CPU = 257


# ---------------------------------------------------------------------------
# The definition
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", rc.N_CPU)
def test_equals_python_reference(n):
    """out and outside bit for bit against the per-element Python reference,
    on NaN, +-inf, +-0.0, ties and a whole-row outlier."""
    base, d = rc.cpu_inputs(n, P_CPU)
    for t in rc.trims(n):
        want, want_out = rc.reference(base, d, t)
        got, outside = ops.trimmed_merge(base, d, t)
        assert got.dtype == torch.float32 and outside.dtype == torch.int64
        assert torch.equal(rc.bits(got), want), (n, t)
        assert torch.equal(outside, want_out), (n, t)


@pytest.mark.parametrize("n", (2, 5, 8, 32))
def test_row_permutation(n):
    base, d = rc.cpu_inputs(n, P_CPU)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
    for t in rc.trims(n):
        o0, c0 = ops.trimmed_merge(base, d, t)
        o1, c1 = ops.trimmed_merge(base, d[perm].contiguous(), t)
        assert torch.equal(rc.bits(o0), rc.bits(o1))
        assert torch.equal(c0[perm], c1)


@pytest.mark.parametrize("n", (1, 3, 5, 9))
def test_odd_median_is_torch_median(n):
    g = torch.Generator().manual_seed(n)
    d = torch.randn(n, 1000, generator=g)
    assert ops.median_trim(n) == (n - 1) // 2
    out, _ = ops.trimmed_merge(torch.zeros(1000), d, ops.median_trim(n))
    assert torch.equal(out, d.median(dim=0).values)


def test_even_median_is_mean_of_middle_two():
    d = torch.tensor([[4.0], [1.0], [2.0], [8.0]])
    out, outside = ops.trimmed_merge(torch.tensor([10.0]), d,
                                     ops.median_trim(4))
    assert out.item() == 13.0
    assert outside.tolist() == [0, 1, 0, 1]


def test_kept_negative_zero_stays_negative_zero():
    d = torch.tensor([[-0.0], [-1.0], [1.0]])
    out, _ = ops.trimmed_merge(torch.tensor([-0.0]), d, 1)
    assert rc.bits(out).item() == -2 ** 31     # 0x80000000


def test_hostile_rows():
    """One miner sends 1e30, one NaN: t = 2 of N = 8 trims both at every
    element, the plain mean does not survive either."""
    P = 4096
    g = torch.Generator().manual_seed(3)
    honest = torch.randn(6, P, generator=g) * 0.01
    base = torch.randn(P, generator=g)
    d = torch.cat([honest[:2], torch.full((1, P), 1e30), honest[2:4],
                   torch.full((1, P), float("nan")), honest[4:]])
    out, outside = ops.trimmed_merge(base, d, 2)
    assert bool(torch.isfinite(out).all())
    lo = base + honest.min(dim=0).values
    hi = base + honest.max(dim=0).values
    # fl(base + mean) against fl(base + min): both monotone roundings
    assert bool((out >= lo).all()) and bool((out <= hi).all())
    assert outside[2].item() == P and outside[5].item() == P
    W = torch.full((8, 1), 1.0 / 8)
    mean = ops.weighted_merge(base, d, W, torch.tensor([0, P]))
    assert not bool(torch.isfinite(mean).any())


def test_fp64_bound():
    n, P = 9, 20000
    g = torch.Generator().manual_seed(11)
    scale = torch.logspace(-3, 3, P)
    d = torch.randn(n, P, generator=g) * scale
    base = torch.randn(P, generator=g) * scale
    u = 2.0 ** -24
    worst = 0.0
    for t in rc.trims(n):
        out, _ = ops.trimmed_merge(base, d, t)
        kept = d.double().sort(dim=0).values[t:n - t]
        m = n - 2 * t
        mean = kept.sum(dim=0) / m
        exact = base.double() + mean
        bound = u * ((m - 1) * kept.abs().sum(dim=0) / m + mean.abs()
                     + exact.abs())
        err = (out.double() - exact).abs()
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound * (1 + 1e-3)).all()), (t, worst)
    print(f"worst |err| / bound = {worst:.3f}")


# ---------------------------------------------------------------------------
# Storages and argument errors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,block,P", [("fp32", 4096, 1027),
                                          ("bf16", 4096, 1027),
                                          ("int8", 16, 1027),
                                          ("int8", 4096, 4096 + 5)])
def test_packed_storage_equals_tensor_path(kind, block, P):
    n = 5
    _, d = rc.cpu_inputs(n, P)
    # int8 of a block with an inf is all NaN: keep that to two blocks
    d = torch.nan_to_num(d, nan=0.0, posinf=3.0, neginf=-3.0).clone()
    d[1, 7] = float("nan")
    d[2, P - 1] = float("inf")
    base = rc.special_base(P)
    pd = PackedDeltas.pack(d, kind, block)
    for t in rc.trims(n):
        o0, c0 = ops.trimmed_merge(base, pd.dequantize(), t)
        o1, c1 = ops.trimmed_merge(base, pd, t)
        assert torch.equal(rc.bits(o0), rc.bits(o1))
        assert torch.equal(c0, c1)


def test_topk_is_refused():
    d = torch.randn(4, 4096)
    pd = PackedDeltas.pack(d, "topk", 1024, 16)
    with pytest.raises(ValueError, match="top-k"):
        ops.trimmed_merge(torch.zeros(4096), pd, 1)


def test_argument_errors():
    base = torch.zeros(8)
    for n, t in [(4, 2), (5, 3), (1, 1), (3, -1)]:
        with pytest.raises(ValueError):
            ops.trimmed_merge(base, torch.zeros(n, 8), t)
    with pytest.raises(ValueError):
        ops.trimmed_merge(base, torch.zeros(0, 8), 0)
    with pytest.raises(ValueError):
        ops.trimmed_merge(base, torch.zeros(33, 8), 1)
    with pytest.raises(ValueError):
        ops.trimmed_merge(base, torch.zeros(4, 9), 1)
    with pytest.raises(ValueError):
        ops.trimmed_merge(base, torch.zeros(4, 8, dtype=torch.float64), 1)


def test_given_buffers_are_overwritten():
    base, d = rc.cpu_inputs(5, P_CPU)
    want, want_c = ops.trimmed_merge(base, d, 1)
    out = torch.full((P_CPU,), 7.0)
    outside = torch.full((5,), 99, dtype=torch.int64)
    o, c = ops.trimmed_merge(base, d, 1, out=out, outside=outside)
    assert o is out and c is outside
    assert torch.equal(rc.bits(out), rc.bits(want))
    assert torch.equal(outside, want_c)


# ---------------------------------------------------------------------------
# Averager and config
# ---------------------------------------------------------------------------
def test_config_flags_parse():
    from distributedtraining_amd.config import AverageConfig, from_args
    assert AverageConfig().trim_count == 1
    cfg = from_args(["--average.strategy", "trimmed_mean",
                     "--average.trim-count", "2"])
    assert cfg.average.strategy == "trimmed_mean"
    assert cfg.average.trim_count == 2


def test_trim_count_is_clamped():
    from distributedtraining_amd.config import AverageConfig
    from distributedtraining_amd.roles.averager import ParameterizedAverager
    av = ParameterizedAverager(None, None, AverageConfig(
        strategy="trimmed_mean", trim_count=3))
    assert [av.robust_trim(n) for n in (1, 2, 3, 6, 7, 8)] == \
        [0, 0, 1, 2, 3, 3]
    assert av.robust_trim(8, "median") == 3


def test_run_round_median_over_file_store(tmp_path):
    """Five tiny-GPT-2 miners, one of which publishes -20 x its delta."""
    from distributedtraining_amd.config import (AverageConfig, Config,
                                                ModelConfig, TrainConfig)
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.parallel.flat import FlatParams
    from distributedtraining_amd.registry import FileRegistry
    from distributedtraining_amd.roles.averager import ParameterizedAverager
    from distributedtraining_amd.roles.miner import DeltaLoop
    from distributedtraining_amd.store import DeltaCheckpoint, FileStore
    from distributedtraining_amd.utils.data import synthetic_batches

    torch.manual_seed(0)
    cfg = Config()
    cfg.model = ModelConfig.gpt2_tiny()
    cfg.train = TrainConfig(batch_size=2, seq_len=16,
                            send_interval_steps=10 ** 9,
                            pull_interval_steps=0)
    model = build_model(cfg.model)
    fp = FlatParams(model)
    base = fp.snapshot()
    registry = FileRegistry(str(tmp_path))
    hostile = "m3"
    for i in range(5):
        fp.load_flat_master(base)
        loop = DeltaLoop(model, fp, synthetic_batches(
            cfg.model.vocab_size, 2, 16, seed=10 + i), cfg.train)
        for _ in range(2):
            loop.train_step()
        flat = loop.make_delta().flat.clone()
        hk = f"m{i}"
        if hk == hostile:
            flat = -20.0 * flat
        st = FileStore(str(tmp_path), hotkey=hk)
        st.push_delta(DeltaCheckpoint(flat, fp.spec, ""))
        registry.store_address(hk, st.my_address())
    fp.load_flat_master(base)

    av = ParameterizedAverager(model, fp, AverageConfig(strategy="median"),
                               store=FileStore(str(tmp_path), hotkey="avg"),
                               registry=registry)
    stack, active = av.collect_deltas()
    assert stack.shape[0] == 5
    merged = av.run_round([])
    want, outside = ops.trimmed_merge(base, stack, ops.median_trim(5))
    assert torch.equal(rc.bits(merged), rc.bits(want))
    assert torch.equal(rc.bits(fp.master), rc.bits(want))
    share = av.last_outside_share
    assert set(share) == set(active)
    assert max(share, key=share.get) == hostile
    assert share[hostile] == outside[active.index(hostile)].item() / fp.numel


# ---------------------------------------------------------------------------
# Local SGD over gloo, world 4
# ---------------------------------------------------------------------------
def _gloo_worker(rank, world, port, exchange, q):
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
    from distributedtraining_amd.parallel.comm import CommPlane
    from distributedtraining_amd.parallel.flat import FlatParams
    from distributedtraining_amd.parallel.local_sgd import LocalSGDNode
    from distributedtraining_amd.utils.data import synthetic_batches
    try:
        cfg = Config()
        cfg.model = ModelConfig.gpt2_tiny()
        cfg.train = TrainConfig(batch_size=2, seq_len=16,
                                send_interval_steps=10 ** 9,
                                pull_interval_steps=0)
        cfg.comm.exchange_dtype = exchange
        cfg.comm.resident_dtype = "wire"
        cfg.average.trim_count = 1
        torch.manual_seed(100 + rank)
        model = build_model(cfg.model)
        fp = FlatParams(model)
        comm = CommPlane(backend="gloo", device=torch.device("cpu"))
        data = synthetic_batches(cfg.model.vocab_size, 2, 16, seed=rank)
        # the combination with top-k is refused before anything is exchanged
        cfg.comm.exchange_dtype = "topk"
        try:
            LocalSGDNode(model, fp, data, cfg, comm,
                         merge_strategy="trimmed_mean")
            refused = False
        except ValueError:
            refused = True
        cfg.comm.exchange_dtype = exchange
        node = LocalSGDNode(model, fp, data, cfg, comm,
                            merge_strategy="trimmed_mean")
        node.sync_initial_base()
        base0 = fp.master.clone()
        node.train_steps(2)
        gathered = node._gather_deltas(node._local_delta(base0), base0)
        want, _ = ops.trimmed_merge(base0, gathered, 1)
        node.merge_round()
        same = torch.equal(fp.master.view(torch.int32),
                           want.view(torch.int32))
        moved = not torch.equal(fp.master, base0)
        digest = fp.master.view(torch.int32).to(torch.int64).sum().item()
        q.put((rank, bool(refused and same and moved), digest,
               node.averager.last_outside_share))
        comm.close()
    except Exception as e:  # pragma: no cover
        q.put((rank, False, repr(e), None))
        raise


@pytest.mark.timeout(300)
@pytest.mark.parametrize("exchange,port", [("fp32", 29911), ("int8", 29913)])
def test_gloo_world4_trimmed_mean(exchange, port):
    """trimmed_mean through the gather path, deltas resident in wire form:
    every rank computes the merge itself and all hold the same bits, the
    bits of ops.trimmed_merge on the gathered deltas."""
    world = 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker,
                         args=(r, world, port, exchange, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok, _, _ in results), results
    assert len({d for _, _, d, _ in results}) == 1, results
    assert all(len(s) == world for _, _, _, s in results)
