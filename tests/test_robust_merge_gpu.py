"""trimmed_merge_k (hip/merge.hip) against the CPU definition of
ops.trimmed_merge on the same inputs, bit for bit, in out and in outside.

The inputs are the special-value sets of tests/_robust_cases.py: NaN, +-inf,
+-0.0, ties, a whole-row outlier. Denormal inputs are left out (see there:
nothing in the build pins the fp32 denormal mode of either side). Packed
storages are quantised once on the CPU and copied, so both sides read the
same codes and scales.
"""

import functools

import pytest
import torch

import _robust_cases as rc

from distributedtraining_amd import ops
from distributedtraining_amd.parallel.comm import PackedDeltas

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (storage, int8 block, P). 1 and 3: less than a vector; 1027: several
# blocks, ragged, rows of bf16 not 8 B aligned (one element per lane);
# 4096: the four-elements-per-lane path of fp32 and bf16, which needs
# P % 4 == 0; 4096 + 5: a ragged tail after full vectors. int8 rows are
# padded to whole blocks and always take four elements per lane.
STORAGE_SHAPES = (
    [(k, 0, P) for k in ("fp32", "bf16") for P in (1, 3, 1027, 4096,
                                                   4096 + 5)]
    + [("int8", 16, 1027), ("int8", 4096, 4096 + 5)])


def _to_dev(pd: PackedDeltas) -> PackedDeltas:
    return PackedDeltas(pd.kind, pd.data.to(DEV), pd.numel,
                        None if pd.scales is None else pd.scales.to(DEV),
                        pd.block, pd.k)


@functools.lru_cache(maxsize=None)
def _case(kind, block, P, n):
    """(base, deltas on the CPU, the same on the device)."""
    base, d = rc.cpu_inputs(n, P)
    if kind == "fp32":
        return base, d, d.to(DEV)
    if kind == "int8":
        # an inf or NaN makes its whole int8 block NaN: keep a few of them
        d = torch.nan_to_num(d, nan=0.0, posinf=3.0, neginf=-3.0).clone()
        d[0, 0] = float("nan")
        d[n - 1, P - 1] = float("inf")
    pd = PackedDeltas.pack(d, kind, block or 4096)
    return base, pd, _to_dev(pd)


def _same(got, want):
    (o, c), (o0, c0) = got, want
    assert o.device.type == "cuda" and c.device.type == "cuda"
    assert c.dtype == torch.int64
    assert torch.equal(rc.bits(o), rc.bits(o0))
    assert torch.equal(c.cpu(), c0)


@pytest.mark.parametrize("n", rc.N_GPU)
@pytest.mark.parametrize("kind,block,P", STORAGE_SHAPES)
def test_equals_cpu_definition(kind, block, P, n):
    base, d_cpu, d_dev = _case(kind, block, P, n)
    for t in rc.trims(n):
        _same(ops.trimmed_merge(base.to(DEV), d_dev, t),
              ops.trimmed_merge(base, d_cpu, t))


def test_second_trip_of_the_grid_stride_loop():
    """P just past what one sweep of the capped grid covers: some lanes take
    the loop a second time and carry their counters across."""
    from distributedtraining_amd.ops.backend import require_ext
    n = 4
    probe = torch.empty(n, 4, device=DEV)
    sweep = require_ext().robust.sweep(probe, 4)     # P % 4 == 0
    P = sweep + 4 * 300 + 4
    assert P % 4 == 0 and P > sweep
    assert require_ext().robust.sweep(torch.empty(n, 1, device=DEV), P) \
        == sweep
    g = torch.Generator().manual_seed(5)
    d = torch.randn(n, P, generator=g)
    d[1, sweep + 7] = float("nan")
    d[2, P - 1] = 1e30
    base = torch.randn(P, generator=g)
    _same(ops.trimmed_merge(base.to(DEV), d.to(DEV), 1),
          ops.trimmed_merge(base, d, 1))


@pytest.mark.parametrize("kind,block,P,n", [("fp32", 0, 4096 + 5, 9),
                                            ("bf16", 0, 4096, 17),
                                            ("int8", 16, 1027, 8)])
def test_repeats_and_ignores_row_order(kind, block, P, n):
    base, d_cpu, d_dev = _case(kind, block, P, n)
    b = base.to(DEV)
    t = rc.trims(n)[-1]
    o0, c0 = ops.trimmed_merge(b, d_dev, t)
    o1, c1 = ops.trimmed_merge(b, d_dev, t)
    assert torch.equal(rc.bits(o0), rc.bits(o1)) and torch.equal(c0, c1)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
    if kind == "fp32":
        dp = d_dev[perm.to(DEV)].contiguous()
    else:
        dp = PackedDeltas(
            d_dev.kind, d_dev.data[perm.to(DEV)].contiguous(), d_dev.numel,
            None if d_dev.scales is None
            else d_dev.scales[perm.to(DEV)].contiguous(), d_dev.block)
    o2, c2 = ops.trimmed_merge(b, dp, t)
    assert torch.equal(rc.bits(o0), rc.bits(o2))
    assert torch.equal(c0[perm.to(DEV)], c2)


@pytest.mark.parametrize("P", (1027, 4096))
def test_writes_only_its_sub_views(P):
    n = 5
    base, d_cpu, d_dev = _case("fp32", 0, P, n)
    big = torch.full((P + 64,), -7.0, device=DEV)
    cnt = torch.full((n + 8,), -7, dtype=torch.int64, device=DEV)
    out, outside = big[32:32 + P], cnt[4:4 + n]     # 16 B aligned views
    o, c = ops.trimmed_merge(base.to(DEV), d_dev, 1, out=out,
                             outside=outside)
    assert o.data_ptr() == out.data_ptr() and c.data_ptr() == outside.data_ptr()
    _same((out, outside), ops.trimmed_merge(base, d_cpu, 1))
    assert bool((big[:32] == -7.0).all()) and bool((big[32 + P:] == -7.0).all())
    assert bool((cnt[:4] == -7).all()) and bool((cnt[4 + n:] == -7).all())


def test_binding_refuses_bad_arguments():
    from distributedtraining_amd.ops.backend import require_ext
    rb = require_ext().robust
    base = torch.zeros(8, device=DEV)
    e = base.new_empty(0)
    out = torch.empty_like(base)

    def go(d, trim=0, out=out, outside=None, base=base):
        rb.trimmed_merge(base, d, e, 0, trim, out, outside)

    with pytest.raises(RuntimeError):
        go(torch.zeros(4, 8, device=DEV), trim=2)
    with pytest.raises(RuntimeError):
        go(torch.zeros(33, 8, device=DEV))
    with pytest.raises(RuntimeError):
        go(torch.zeros(4, 9, device=DEV))
    with pytest.raises(RuntimeError):
        go(torch.zeros(4, 8, device=DEV, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        go(torch.zeros(4, 8, device=DEV), out=torch.empty(7, device=DEV))
    with pytest.raises(RuntimeError):
        go(torch.zeros(4, 8, device=DEV),
           outside=torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):       # four per lane wants 16 B
        go(torch.zeros(4, 8, device=DEV),
           base=torch.zeros(9, device=DEV)[1:])
    with pytest.raises(RuntimeError):       # int8 block not a power of two
        rb.trimmed_merge(base, torch.zeros(4, 24, dtype=torch.int8,
                                           device=DEV),
                         torch.ones(4, 1, device=DEV), 24, 0, out, None)
    pd = PackedDeltas.pack(torch.randn(4, 4096), "topk", 1024, 16)
    with pytest.raises(ValueError, match="top-k"):
        ops.trimmed_merge(torch.zeros(4096, device=DEV), _to_dev(pd), 1)


def test_averager_robust_merge_on_device():
    """ParameterizedAverager.robust_merge on five real tiny-GPT-2 deltas."""
    from distributedtraining_amd.config import (AverageConfig, Config,
                                                ModelConfig, TrainConfig)
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.parallel.flat import FlatParams
    from distributedtraining_amd.roles.averager import ParameterizedAverager
    from distributedtraining_amd.roles.miner import DeltaLoop
    from distributedtraining_amd.utils.data import synthetic_batches

    torch.manual_seed(0)
    cfg = Config()
    cfg.model = ModelConfig.gpt2_tiny()
    cfg.train = TrainConfig(batch_size=2, seq_len=16,
                            send_interval_steps=10 ** 9,
                            pull_interval_steps=0)
    model = build_model(cfg.model).to(DEV)
    fp = FlatParams(model)
    base = fp.snapshot()
    deltas = []
    for i in range(5):
        fp.load_flat_master(base)
        loop = DeltaLoop(model, fp, synthetic_batches(
            cfg.model.vocab_size, 2, 16, seed=20 + i), cfg.train)
        loop.train_step()
        d = loop.make_delta().flat.clone()
        deltas.append(-20.0 * d if i == 3 else d)
    stack = torch.stack(deltas)
    av = ParameterizedAverager(model, fp,
                               AverageConfig(strategy="trimmed_mean"))
    merged = av.robust_merge(base, stack)
    want, outside = ops.trimmed_merge(base.cpu(), stack.cpu(), 1)
    assert merged.device.type == "cuda"
    assert torch.equal(rc.bits(merged), rc.bits(want))
    assert av.last_outside_share == [c / fp.numel for c in outside.tolist()]
    assert max(range(5), key=av.last_outside_share.__getitem__) == 3
