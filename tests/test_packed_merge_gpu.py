"""Packed deltas on the GPU (merge.hip): the int8 quantiser against the CPU
definition bit for bit, and weighted_merge / grad_W / axpy on bf16 and int8
storage against the fp32 kernels on the dequantised rows.

Measured on an MI355X: grad_W against the fp64 formula, rel_l2 / worst entry,
is 8.9e-08 to 2.0e-07 / 9.6e-08 to 3.1e-07 for the packed kernels, against
8.5e-08 to 2.5e-07 / 1.3e-07 to 4.1e-07 for the fp32 formula summed in the
kernel's order on the CPU (tests/_numerics.py, the baseline the check holds
them to); they sum in the fp32 kernel's order and give its bits.
"""

import functools

import pytest
import torch

import _numerics as nm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEGS = [1000, 37, 4096, 123]     # boundaries inside blocks and 16 B vectors


def _ext():
    from distributedtraining_amd.ops.backend import require_ext
    return require_ext()


# ---------------------------------------------------------------------------
# Quantiser
# ---------------------------------------------------------------------------
QUANT_SHAPES = [(3 * 4096 + 37, 4096), (1000, 4096), (5 * 256 + 1, 256)]


@functools.lru_cache(maxsize=None)
def _quant_input(P, block):
    """randn * 1e-3 with, block by block as far as there are blocks: exact
    .5 code ties (block 0: absmax 127 * 2^-10, so the scale is 2^-10, and
    values (j + .5) * 2^-10 of both signs, odd and even j), one 1e3 outlier
    (block 1), all zeros (block 2). The last block is the ragged one."""
    g = torch.Generator().manual_seed(P + block)
    x = torch.randn(P, generator=g) * 1e-3
    nb = (P + block - 1) // block
    s = 2.0 ** -10
    n0 = min(block, P)
    x[0] = 127 * s
    js = torch.tensor([0, 1, 2, 3, 10, 11, 125, 126], dtype=torch.float32)
    x[1:9] = (js + 0.5) * s
    x[9:17] = -(js + 0.5) * s
    assert n0 > 17
    if nb > 1:
        x[block + 5] = 1e3
    if nb > 2:
        x[2 * block:3 * block] = 0.0
    return x


@pytest.mark.parametrize("P,block", QUANT_SHAPES)
def test_quantizer_equals_cpu_definition(P, block):
    from distributedtraining_amd import ops
    from distributedtraining_amd.parallel import comm
    x = _quant_input(P, block)
    q0, s0 = comm.quantize_blockwise_int8(x, block)
    # the ties are there, and went to even
    assert s0[0].item() == 2.0 ** -10
    assert q0[1:9].tolist() == [0, 2, 2, 4, 10, 12, 126, 126]
    assert q0[9:17].tolist() == [0, -2, -2, -4, -10, -12, -126, -126]
    q, s = ops.quantize_blockwise_int8(x.to(DEV), block)
    assert q.dtype == torch.int8 and s.dtype == torch.float32
    assert torch.equal(q.cpu(), q0)
    assert torch.equal(s.cpu(), s0)

    # fused (w, base): one fp32 subtraction, then the same quantiser
    g = torch.Generator().manual_seed(7)
    base = torch.randn(P, generator=g)
    w = base + x
    if P > 2 * block:
        w[2 * block:3 * block] = base[2 * block:3 * block]
    q0, s0 = comm.quantize_blockwise_int8(w - base, block)
    q, s = ops.quantize_blockwise_int8(w.to(DEV), block, base=base.to(DEV))
    assert torch.equal(q.cpu(), q0)
    assert torch.equal(s.cpu(), s0)


def test_quantizer_propagates_nan():
    from distributedtraining_amd import ops
    from distributedtraining_amd.parallel import comm
    P, block = 5 * 256 + 1, 256
    x = _quant_input(P, block).clone()
    x[3 * block + 77] = float("nan")
    _, s0 = comm.quantize_blockwise_int8(x, block)
    _, s = ops.quantize_blockwise_int8(x.to(DEV), block)
    s = s.cpu()
    bad = torch.zeros(6, dtype=torch.bool)
    bad[3] = True
    assert torch.equal(torch.isnan(s), bad)
    assert torch.equal(torch.isnan(s0), bad)
    assert torch.equal(s[~bad], s0[~bad])
    assert bool(torch.isfinite(s[~bad]).all())


# ---------------------------------------------------------------------------
# Packed merge / grad_W / axpy
# ---------------------------------------------------------------------------
def _offsets(segs):
    return torch.tensor([0] + list(torch.tensor(segs).cumsum(0)))


@functools.lru_cache(maxsize=None)
def _merge_inputs(segs=tuple(SEGS), N=3, seed=23):
    g = torch.Generator().manual_seed(seed)
    P = sum(segs)
    return dict(P=P, offsets=_offsets(list(segs)),
                base=torch.randn(P, generator=g),
                deltas=torch.randn(N, P, generator=g) * 1e-3,
                W=torch.rand(N, len(segs), generator=g),
                grad=torch.randn(P, generator=g))


PACKED_KINDS = [("int8", 256), ("int8", 4096), ("bf16", 4096)]


@functools.lru_cache(maxsize=None)
def _packed(kind, block, segs=tuple(SEGS), N=3):
    """(PackedDeltas on the GPU, its rows dequantised on the GPU)."""
    from distributedtraining_amd.parallel.comm import PackedDeltas
    t = _merge_inputs(segs, N)
    pd = PackedDeltas.pack(t["deltas"].to(DEV), kind, block)
    return pd, pd.dequantize()


def _cpu_rows(pd):
    """The rows by the CPU definition, from the codes the GPU made."""
    from distributedtraining_amd.parallel import comm
    if pd.kind == "bf16":
        return pd.data.cpu().float()
    return torch.stack([
        comm.dequantize_blockwise_int8(pd.data[i].cpu(), pd.scales[i].cpu(),
                                       pd.numel, pd.block)
        for i in range(pd.shape[0])])


@pytest.mark.parametrize("kind,block", PACKED_KINDS)
def test_packed_merge_equals_fp32_kernel(kind, block):
    from distributedtraining_amd import ops
    m = _ext()
    t = _merge_inputs()
    pd, dense = _packed(kind, block)
    assert pd.shape == (3, t["P"]) and dense.dtype == torch.float32
    assert torch.equal(dense.cpu(), _cpu_rows(pd))
    base, W, offs = t["base"].to(DEV), t["W"].to(DEV), t["offsets"].to(DEV)
    want = torch.empty(t["P"], device=DEV)
    m.weighted_merge(base, dense, W, offs, want)
    got = ops.weighted_merge(base, pd, W, t["offsets"])
    assert torch.equal(got, want)


@pytest.mark.parametrize("kind,block", PACKED_KINDS)
def test_packed_grad_w(kind, block):
    from distributedtraining_amd import ops
    m = _ext()
    t = _merge_inputs()
    pd, dense = _packed(kind, block)
    base, offs = t["base"].to(DEV), t["offsets"].to(DEV)
    merged = torch.empty(t["P"], device=DEV)
    m.weighted_merge(base, dense, t["W"].to(DEV), offs, merged)
    # the formula in fp64, and in fp32 summed in the kernel's order, on
    # exactly the values the kernels read (tests/_numerics.py)
    for g in (t["grad"].to(DEV), t["grad"].to(DEV, torch.bfloat16)):
        a = (nm.d(g), nm.d(t["base"]), nm.d(dense), nm.d(merged),
             t["offsets"])
        ex = nm.grad_merge_weights(*a, mode="exact")
        rd = nm.grad_merge_weights(*a, mode="rounded")
        ref = m.grad_merge_weights(g, base, dense, merged, offs)
        got = ops.grad_merge_weights(g, base, pd, merged, t["offsets"])
        nm.check("grad_merge_weights_packed",
                 f"{kind} block {block} g {g.dtype}", "grad_W", got, ex, rd,
                 row_dim=None, fp32_out=True)
        # one chunk per segment and the fp32 kernel's summation order
        assert torch.equal(got, ref)


@pytest.mark.parametrize("kind,block", PACKED_KINDS)
def test_axpy_packed(kind, block):
    from distributedtraining_amd import ops
    m = _ext()
    t = _merge_inputs()
    pd, dense = _packed(kind, block)
    for alpha in (1.0, -0.37):
        want = t["base"].to(DEV)
        m.axpy(want, dense[1].contiguous(), alpha)
        got = t["base"].to(DEV)
        assert ops.axpy_(got, (pd, 1), alpha) is got
        assert torch.equal(got, want)


# P % 4 != 0 (cut last vector; bf16 rows no longer 8 B aligned: one element
# per lane), a plane the capped grid walks twice (2048 blocks x 256 lanes x 4
# elements), and segments of more than one 1M-element chunk.
ODD_SEGS = (1001, 2, 4098)
BIG_SEGS = (1_300_003, 37, 900_001)


@pytest.mark.parametrize("kind,block,segs,N", [
    ("int8", 256, ODD_SEGS, 3), ("bf16", 4096, ODD_SEGS, 3),
    ("bf16", 4096, ODD_SEGS, 2),      # odd rows, even buffer: shared words
    ("int8", 4096, BIG_SEGS, 2), ("bf16", 4096, BIG_SEGS + (3,), 2)])
def test_packed_odd_and_large_planes(kind, block, segs, N):
    from distributedtraining_amd import ops
    m = _ext()
    t = _merge_inputs(segs, N)
    pd, dense = _packed(kind, block, segs, N)
    assert torch.equal(dense.cpu(), _cpu_rows(pd))
    base, W, offs = t["base"].to(DEV), t["W"].to(DEV), t["offsets"].to(DEV)
    want = torch.empty(t["P"], device=DEV)
    m.weighted_merge(base, dense, W, offs, want)
    assert torch.equal(ops.weighted_merge(base, pd, W, t["offsets"]), want)
    g = t["grad"].to(DEV)
    # at most two chunks per segment: their two atomic adds commute
    assert torch.equal(
        ops.grad_merge_weights(g, base, pd, want, t["offsets"]),
        m.grad_merge_weights(g, base, dense, want, offs))
    a, b = base.clone(), base.clone()
    m.axpy(a, dense[N - 1].clone(), -0.37)     # a row of its own: aligned
    ops.axpy_(b, (pd, N - 1), -0.37)
    assert torch.equal(a, b)


def test_packed_bindings_reject_bad_arguments():
    m = _ext()
    P = 1024
    base = torch.zeros(P, device=DEV)
    codes = torch.zeros(2, 1024, dtype=torch.int8, device=DEV)
    scales = torch.ones(2, 4, device=DEV)
    W = torch.ones(2, 1, device=DEV)
    offs = torch.tensor([0, P], device=DEV)
    out = torch.empty(P, device=DEV)
    m.weighted_merge_packed(base, codes, scales, 256, W, offs, out)
    with pytest.raises(RuntimeError):       # scales not [N, nb]
        m.weighted_merge_packed(base, codes, scales[:, :3].contiguous(), 256,
                                W, offs, out)
    with pytest.raises(RuntimeError):       # codes not nb*block wide
        m.weighted_merge_packed(base, codes[:, :1000].contiguous(), scales,
                                256, W, offs, out)
    with pytest.raises(RuntimeError):       # block not a power of two
        m.weighted_merge_packed(base, codes, scales, 250, W, offs, out)
    with pytest.raises(RuntimeError):       # fp32 data is not a packed form
        m.weighted_merge_packed(base, codes.float(), scales, 256, W, offs,
                                out)
    with pytest.raises(RuntimeError):       # more models than MAX_MODELS
        m.weighted_merge_packed(
            base, torch.zeros(33, 1024, dtype=torch.int8, device=DEV),
            torch.ones(33, 4, device=DEV), 256, torch.ones(33, 1, device=DEV),
            offs, out)
    with pytest.raises(RuntimeError):       # W past the LDS budget
        S = 1024
        m.weighted_merge_packed(
            base, torch.zeros(32, 1024, dtype=torch.int8, device=DEV),
            torch.ones(32, 4, device=DEV), 256,
            torch.ones(32, S, device=DEV),
            torch.arange(S + 1, device=DEV), out)
    with pytest.raises(RuntimeError):       # row out of range
        m.axpy_packed(out, codes, scales, 256, 2, 1.0)
    with pytest.raises(RuntimeError):
        m.quantize_int8(base, torch.empty(0, device=DEV), 100)


# ---------------------------------------------------------------------------
# Footprint
# ---------------------------------------------------------------------------
def test_packed_footprint():
    """N = 8, P = 2^20, int8: merge + grad_W allocate the output plane and
    small tables (about P*4 bytes), never a dequantised stack (8*P*4)."""
    from distributedtraining_amd import ops
    from distributedtraining_amd.parallel.comm import PackedDeltas
    N, P = 8, 1 << 20
    g = torch.Generator().manual_seed(3)
    deltas = (torch.randn(N, P, generator=g) * 1e-3).to(DEV)
    pd = PackedDeltas.pack(deltas, "int8")
    del deltas
    base = torch.randn(P, generator=g).to(DEV)
    grad = torch.randn(P, generator=g).to(DEV, torch.bfloat16)
    offsets = torch.arange(0, P + 1, P // 16)
    W = torch.full((N, 16), 1.0 / N, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    merged = ops.weighted_merge(base, pd, W, offsets)
    gw = ops.grad_merge_weights(grad, base, pd, merged, offsets)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"[packed merge] footprint: peak rise {rise} B = "
          f"{rise / (P * 4):.3f} x P*4")
    assert rise < 2 * P * 4
    assert gw.shape == (N, 16) and bool(torch.isfinite(gw).all())
    assert bool(torch.isfinite(merged).all())


# ---------------------------------------------------------------------------
# End to end through the averager
# ---------------------------------------------------------------------------
def test_packed_averager_end_to_end():
    from distributedtraining_amd.config import Config, ModelConfig
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.parallel.comm import PackedDeltas
    from distributedtraining_amd.parallel.flat import FlatParams
    from distributedtraining_amd.roles.averager import ParameterizedAverager
    from distributedtraining_amd.utils.data import synthetic_eval_set

    cfg = Config()
    cfg.model = ModelConfig.gpt2_tiny()
    torch.manual_seed(0)
    model = build_model(cfg.model).to(DEV)
    fp = FlatParams(model)
    base = fp.master.clone()
    g = torch.Generator().manual_seed(11)
    deltas = (torch.randn(3, fp.numel, generator=g) * 1e-3).to(DEV)
    val = synthetic_eval_set(cfg.model.vocab_size, 1, 4, 32)
    for kind in ("int8", "bf16"):
        pd = PackedDeltas.pack(deltas, kind)
        dense = pd.dequantize()

        def both(d):
            av = ParameterizedAverager(model, fp, cfg.average)
            fp.load_flat_master(base)
            meta = av.meta_learning(base, d, val, meta_epochs=1).clone()
            sw = av.score_weighted_merge(base, d, [0.2, 0.5, 0.3])
            return meta, sw, av.weights.clone()

        meta_p, sw_p, w_p = both(pd)
        meta_d, sw_d, w_d = both(dense)
        assert torch.equal(sw_p, sw_d)
        assert not torch.equal(sw_p, base)
        assert torch.equal(w_p, w_d)
        assert torch.equal(meta_p, meta_d)
    fp.load_flat_master(base)
