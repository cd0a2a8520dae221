"""Bias and norm-parameter gradients: the GELU backward that also sums its
columns (gelu_bwd_colsum_k), the one kernel that finishes every column
reduction (colred_finish_k: fp32 store or accumulation into a bf16
destination, no atomics), and the one-node MLP built on them.

Bit-for-bit where the arithmetic is the same (dx of the fused GELU backward,
repeated calls of the finisher, the bf16 accumulation against its fp32
store mode, every GEMM of the MLP node). A column sum whose order changed
is held to the fp32 bound of tests/_numerics.py, or, after its rounding to
bf16, to the reordered-sum bound of `_reorder_tol`.
"""

import functools

import pytest
import torch

import _numerics as N

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from distributedtraining_amd.ops.backend import require_ext
    return require_ext()


def _bf16_accum(dst_before, s32):
    """bf16(float(dst) + sum): accum_f32_bf16_k's rounding."""
    return (dst_before.float() + s32).to(torch.bfloat16)


def _dst_views(cols, seed):
    """[(label, buffer, its copy, offset)]: a random bf16 buffer holding a
    16 B aligned view and one shifted by a single element."""
    out = []
    for label, off in (("aligned", 8), ("odd", 9)):
        buf = N.randn_bf16(cols + 24, seed=seed).to(DEV)
        assert (buf[off:].data_ptr() % 16 == 0) == (label == "aligned")
        out.append((label, buf, buf.clone(), off))
    return out


def _check_view(buf, before, off, cols, want):
    assert torch.equal(buf[off:off + cols], want)
    assert torch.equal(buf[:off], before[:off])
    assert torch.equal(buf[off + cols:], before[off + cols:])


# ---------------------------------------------------------------------------
# 1. fused GELU backward + column sum
# ---------------------------------------------------------------------------
GELU_SHAPES = [(1, 8), (33, 520), (70, 16), (333, 3072), (4099, 24)]
# cols % 8 != 0: the binding's gelu_bwd + colsum fallback
GELU_FALLBACK_SHAPES = [(33, 12), (70, 5)]


@functools.lru_cache(maxsize=None)
def _gelu_inputs(rows, cols, regime):
    x, _up, dy = N.ew_inputs(rows * cols, regime)
    return x.view(rows, cols), dy.view(rows, cols)


@pytest.mark.parametrize("regime", ["randn2", "tail"])
@pytest.mark.parametrize("rows,cols", GELU_SHAPES + GELU_FALLBACK_SHAPES)
def test_gelu_bwd_colsum(rows, cols, regime):
    m = _ext()
    x, dy = (t.to(DEV) for t in _gelu_inputs(rows, cols, regime))
    want_dx = m.gelu_bwd(dy, x)
    dx, db = m.gelu_bwd_colsum(dy, x)
    assert torch.equal(dx, want_dx)
    assert db.dtype == torch.float32 and db.shape == (cols,)
    # the sum is of the ROUNDED bf16 dx, as colsum(dx) is
    N.check("gelu_bwd_colsum", f"({rows}, {cols})/{regime}", "db", db,
            N.colsum(N.d(want_dx)), N.colsum(N.d(want_dx), "rounded"),
            row_dim=None, fp32_out=True)
    dx2, db2 = m.gelu_bwd_colsum(dy, x)
    assert torch.equal(dx2, dx) and torch.equal(db2, db)
    for label, buf, before, off in _dst_views(cols, seed=61):
        dx3, none = m.gelu_bwd_colsum(dy, x, buf[off:off + cols])
        assert none is None and torch.equal(dx3, dx), label
        _check_view(buf, before, off, cols,
                    _bf16_accum(before[off:off + cols], db))


# ---------------------------------------------------------------------------
# 2. / 3. the finisher through colsum: fp32 store, bf16 accumulation
# ---------------------------------------------------------------------------
COLSUM_SHAPES = [(65, 8), (333, 520), (4099, 24), (70000, 768)]


@functools.lru_cache(maxsize=None)
def _colsum_case(rows, cols):
    x = N.randn_bf16(rows, cols, seed=23)
    return x, N.colsum(N.d(x)), N.colsum(N.d(x), "rounded")


@pytest.mark.parametrize("rows,cols", COLSUM_SHAPES + [(33, 12), (7, 3)])
def test_colsum_fp32_store(rows, cols):
    m = _ext()
    x, exact, rounded = _colsum_case(rows, cols)
    xd = x.to(DEV)
    a = m.colsum(xd)
    N.check("colsum", f"({rows}, {cols})", "sum", a, exact, rounded,
            row_dim=None, fp32_out=True)
    # the output is torch.empty: a second call lands on other memory and
    # must still give the same bits
    keep = torch.full((cols,), float("nan"), device=DEV)
    b = m.colsum(xd)
    assert torch.equal(a, b)
    del keep


@pytest.mark.parametrize("rows,cols", COLSUM_SHAPES[:3] + [(33, 12)])
def test_colsum_bf16_accumulate(rows, cols):
    m = _ext()
    xd = _colsum_case(rows, cols)[0].to(DEV)
    s32 = m.colsum(xd)
    for label, buf, before, off in _dst_views(cols, seed=62):
        assert m.colsum(xd, buf[off:off + cols]) is None, label
        _check_view(buf, before, off, cols,
                    _bf16_accum(before[off:off + cols], s32))


def test_embedding_dwpe_tail_stays_zero():
    m = _ext()
    V, P, E, B, S = 64, 48, 64, 5, 32
    dy = N.randn_bf16(B, S, E, seed=702).to(DEV)
    ids = torch.randint(0, V, (B, S),
                        generator=torch.Generator().manual_seed(703)).to(DEV)
    _dwte, dwpe = m.embedding_bwd(dy, ids, V, P)
    assert dwpe.shape == (P, E)
    assert torch.all(dwpe[S:] == 0)
    assert torch.equal(dwpe[:S].reshape(-1), m.colsum(dy.view(B, S * E)))


# ---------------------------------------------------------------------------
# 4. norm backward with destinations
# ---------------------------------------------------------------------------
NORM_SHAPES = [(33, 8), (5, 768), (33, 4096), (2100, 520)]


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize("kind", ["layer", "rms"])
@pytest.mark.parametrize("rows,cols", NORM_SHAPES)
def test_norm_bwd_destinations(rows, cols, kind, drop):
    from distributedtraining_amd.ops import droprng
    m = _ext()
    t = {k: v.to(DEV) for k, v in N.norm_inputs(rows, cols, "randn").items()}
    p, site, ctr = N.NORM_DROP if drop else (0.0, 0, 0)
    rng = droprng.counter(DEV)
    rng.fill_(ctr)
    empty = t["x"].new_empty(0)
    res, ds = (t["res"], t["ds"]) if drop else (empty, empty)
    layer = kind == "layer"
    if layer:
        _y, mean, rstd, s = m.layernorm_fwd(t["x"], res, t["w"], t["b"],
                                            N.NORM_EPS, rng, site, p)
    else:
        _y, rstd, s = m.rmsnorm_fwd(t["x"], res, t["w"], N.NORM_EPS, rng,
                                    site, p)
    xin = s if drop else t["x"]

    def bwd(*dst):
        if layer:
            return m.layernorm_bwd(t["dy"], ds, xin, t["w"], mean, rstd, rng,
                                   site, p, *dst)
        dx, dw, dres = m.rmsnorm_bwd(t["dy"], ds, xin, t["w"], rstd, rng,
                                     site, p, *dst[:1])
        return dx, dw, None, dres

    dx, dw, db, dres = bwd()
    dx2, dw2, db2, dres2 = bwd()
    assert torch.equal(dw, dw2) and torch.equal(dx, dx2)
    assert (db is None) == (not layer)
    if layer:
        assert torch.equal(db, db2)
    for (label, wbuf, wbefore, off), (_l, bbuf, bbefore, _o) in zip(
            _dst_views(cols, seed=63), _dst_views(cols, seed=64)):
        dx3, dw3, db3, dres3 = bwd(wbuf[off:off + cols], bbuf[off:off + cols])
        assert dw3 is None and db3 is None, label
        assert torch.equal(dx3, dx) and torch.equal(dres3, dres), label
        _check_view(wbuf, wbefore, off, cols,
                    _bf16_accum(wbefore[off:off + cols], dw))
        if layer:
            _check_view(bbuf, bbefore, off, cols,
                        _bf16_accum(bbefore[off:off + cols], db))
        else:
            assert torch.equal(bbuf, bbefore)


# ---------------------------------------------------------------------------
# 5. the MLP node against linear -> gelu -> linear
# ---------------------------------------------------------------------------
E, HID = 16, 64
MLP_NAMES = ("w1", "b1", "w2", "b2")
MLP_SHAPES = dict(w1=(HID, E), b1=(HID,), w2=(E, HID), b2=(E,))


def _mlp_params(flat):
    """bf16 leaf parameters; flat: carve main_grad views out of one zeroed
    bf16 plane, unpadded as parallel.flat.FlatParams lays them out (b1's
    view starts at an odd element)."""
    ps = {n: N.randn_bf16(*MLP_SHAPES[n], seed=70 + i, scale=0.3).to(DEV)
          .requires_grad_(True) for i, n in enumerate(MLP_NAMES)}
    plane = None
    if flat:
        plane = torch.zeros(1 + sum(p.numel() for p in ps.values()),
                            dtype=torch.bfloat16, device=DEV)
        o = 1
        for n in MLP_NAMES:
            ps[n].main_grad = plane[o:o + ps[n].numel()].view(MLP_SHAPES[n])
            o += ps[n].numel()
    return ps, plane


def _mlp_run(rows, flat, node, passes=1):
    from distributedtraining_amd import ops
    ps, plane = _mlp_params(flat)
    x = N.randn_bf16(rows, E, seed=80).to(DEV).requires_grad_(True)
    dy = N.randn_bf16(rows, E, seed=81).to(DEV)
    was = ops.mlp_node_enable(node)
    try:
        for _ in range(passes):
            x.grad = None
            y = ops.mlp_gelu(x, *(ps[n] for n in MLP_NAMES))
            kinds = set()
            stack = [y.grad_fn]
            while stack:
                f = stack.pop()
                if f is not None:
                    kinds.add(type(f).__name__)
                    stack += [g for g, _ in f.next_functions]
            assert ("_MLPGeluFnBackward" in kinds) == node, kinds
            y.backward(dy)
    finally:
        ops.mlp_node_enable(was)
    grads = {n: (ps[n].main_grad if flat else ps[n].grad) for n in MLP_NAMES}
    if flat:
        assert all(ps[n].grad is None for n in MLP_NAMES)
    return y.detach(), x.grad, grads, ps


def _reorder_tol(n_terms, abs_sum, value, passes):
    """How far two bf16 results of the same column sum may lie apart when
    only the ORDER of the fp32 additions differs: either fp32 sum is within
    (n - 1) * 2^-24 * sum|x| of the exact one, so the two lie within twice
    that of each other, and rounding each to bf16 (8 significant bits) adds
    at most one bf16 ulp of the value where they straddle a rounding
    boundary. Each accumulating pass may add that again."""
    ulp = torch.exp2(torch.floor(torch.log2(
        value.abs().double().clamp(min=2.0 ** -126))) - 7)
    return passes * (ulp + 2 * (n_terms - 1) * 2.0 ** -24 * abs_sum.double())


# (flat, passes): two passes without zeroing only where the kernels do the
# accumulating themselves (main_grad)
@pytest.mark.parametrize("flat,passes", [(False, 1), (True, 1), (True, 2)],
                         ids=["autograd", "main_grad", "main_grad-2passes"])
@pytest.mark.parametrize("rows", [10, 130])
def test_mlp_node_matches_three_nodes(rows, flat, passes, monkeypatch):
    from distributedtraining_amd import ops
    m = _ext()
    # both settings on the composed path, whatever hipBLASLt offers here
    monkeypatch.setitem(ops._lt_fused_shape_ok, (rows, HID, E), False)
    y0, dx0, g0, ps = _mlp_run(rows, flat, node=False, passes=passes)
    y1, dx1, g1, _ = _mlp_run(rows, flat, node=True, passes=passes)
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
    for n in ("w1", "w2", "b2"):
        assert torch.equal(g1[n], g0[n]), n
    if flat and passes == 2:
        one = _mlp_run(rows, flat, node=True, passes=1)[2]
        assert not torch.equal(g1["w1"], one["w1"])   # it did accumulate
    # db1: the same bf16 dh_pre values summed in another order
    with torch.no_grad():
        x = N.randn_bf16(rows, E, seed=80).to(DEV)
        dy = N.randn_bf16(rows, E, seed=81).to(DEV)
        pre = torch.addmm(ps["b1"], x, ps["w1"].t())
        dh_pre = m.gelu_bwd(dy.mm(ps["w2"]), pre)
    tol = _reorder_tol(rows, dh_pre.float().abs().sum(0), g0["b1"], passes)
    diff = (g1["b1"].double() - g0["b1"].double()).abs()
    print(f"[db1] rows={rows} max diff {diff.max().item():.3e} "
          f"min slack {(tol - diff).min().item():.3e}")
    assert torch.all(diff <= tol)


# ---------------------------------------------------------------------------
# 6. graph capture of the new paths
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [10, 130])
def test_graph_capture_mlp_and_add_norm(rows, monkeypatch):
    from distributedtraining_amd import ops
    from distributedtraining_amd.ops import droprng
    monkeypatch.setitem(ops._lt_fused_shape_ok, (rows, HID, E), False)
    droprng.counter(DEV).fill_(5)
    ps, plane = _mlp_params(flat=True)
    nw = N.randn_bf16(E, seed=90, scale=0.5).to(DEV).requires_grad_(True)
    nb = N.randn_bf16(E, seed=91, scale=0.5).to(DEV).requires_grad_(True)
    nplane = torch.zeros(2 * E + 1, dtype=torch.bfloat16, device=DEV)
    nw.main_grad, nb.main_grad = nplane[1:1 + E], nplane[1 + E:]
    x = N.randn_bf16(rows, E, seed=80).to(DEV).requires_grad_(True)
    res = N.randn_bf16(rows, E, seed=82).to(DEV).requires_grad_(True)
    dy = N.randn_bf16(rows, E, seed=81).to(DEV)
    was = ops.mlp_node_enable(True)

    def step():
        x.grad = res.grad = None
        s, h = ops.add_layer_norm(x, res, nw, nb, 1e-5, 0.1, 3)
        y = ops.mlp_gelu(h, *(ps[n] for n in MLP_NAMES)) + s
        y.backward(dy)
        return y.detach(), x.grad, res.grad

    try:
        for _ in range(2):
            want = [t.clone() for t in step()]
        want_planes = plane.clone(), nplane.clone()
        plane.zero_(); nplane.zero_()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        plane.zero_(); nplane.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            got = step()
        g.replay()
        g.replay()
        torch.cuda.synchronize()
    finally:
        ops.mlp_node_enable(was)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert torch.equal(plane, want_planes[0])
    assert torch.equal(nplane, want_planes[1])
