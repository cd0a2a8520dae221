"""The weight-gradient kernel (hip/wgrad.hip) on the GPU: accuracy of dW and
db against the fp64 references of tests/_wgrad_cases.py under the bounds of
tests/_numerics.py (tests/test_wgrad_cpu.py shows on the CPU that these bounds
reject the kernel's possible mistakes on these inputs), bit-repeatability,
the routing switch on a two-layer model, and one captured replay.

The library path (addmm_ + colsum) is measured on the same inputs and recorded
beside the kernel in the accuracy report; it is not asserted here."""

import pytest
import torch

import _numerics as N
import _wgrad_cases as W

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from distributedtraining_amd.ops.backend import require_ext
    return require_ext()


@pytest.fixture(scope="module", autouse=True)
def _accuracy_report():
    yield
    N.dump_report()


def test_tile_constants():
    assert tuple(_ext().wgrad.tile()) == (W.BM, W.BN, W.BK)


def _operand(t, pad):
    """t on the GPU as a view whose row stride is pad elements larger than
    its width (16 B aligned base, the packed-qkv layout)."""
    if not pad:
        return t.to(DEV)
    buf = torch.full((t.shape[0], t.shape[1] + pad), 7.0,
                     dtype=torch.bfloat16, device=DEV)
    v = buf[:, :t.shape[1]]
    v.copy_(t)
    return v


def _dest(t, off):
    """(buffer, view): t on the GPU as a view starting off elements into a
    buffer with one guard element on either side."""
    buf = torch.full((t.numel() + off + 1,), 3.0, dtype=torch.bfloat16,
                     device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return buf, v


def _run(c, nsplit=None):
    """One kernel call on fresh copies -> (dw view, db bf16 view or fp32
    tensor or None)."""
    m = _ext()
    cc = c["c"]
    dy, x = _operand(c["dy"], cc["pad"]), _operand(c["x"], cc["pad"])
    wbuf, dw = _dest(c["dst_w"], cc["off"])
    bbuf, db = _dest(c["dst_b"], cc["off"])
    ns = cc["ns"] if nsplit is None else nsplit
    if cc["bias"] == "dst":
        ret = m.wgrad.bias(dy, x, dw, db, False, ns)
        assert ret is None or not ret.numel()
        bias = db
    elif cc["bias"] == "f32":
        bias = m.wgrad.bias(dy, x, dw, None, True, ns)
        assert bias.dtype == torch.float32 and bias.shape == (cc["out"],)
    else:
        ret = m.wgrad.bias(dy, x, dw, None, False, ns)
        assert ret is None or not ret.numel()
        bias = None
    torch.cuda.synchronize()
    # guards and, where no bias goes to db, db itself are untouched
    assert float(wbuf[-1]) == 3.0 and (cc["off"] == 0 or float(wbuf[0]) == 3.0)
    assert float(bbuf[-1]) == 3.0 and (cc["off"] == 0 or float(bbuf[0]) == 3.0)
    if cc["bias"] != "dst":
        assert torch.equal(db.cpu(), c["dst_b"])
    return dw, bias


def _record(op, case, tensor, got, exact, rounded, row_dim, fp32_out=False):
    """A report row without an assertion (the library arm)."""
    base, bound = N.bounds(exact, rounded, row_dim, None, fp32_out)
    kern = N.errors(got, exact, row_dim)
    N.REPORT.append(dict(op=op, case=case, tensor=tensor, fp32=fp32_out,
                         base_l2=base[0], base_worst=base[1], kern_l2=kern[0],
                         kern_worst=kern[1], bound_l2=bound[0],
                         bound_worst=bound[1]))
    print(f"[acc] {op} {case} {tensor}: base {base[0]:.3e}/{base[1]:.3e} "
          f"kernel {kern[0]:.3e}/{kern[1]:.3e} "
          f"bound {bound[0]:.3e}/{bound[1]:.3e}")


def _library(c, cid):
    """addmm_ + colsum on the same inputs, recorded beside the kernel."""
    m = _ext()
    cc = c["c"]
    dy, x = c["dy"].to(DEV), c["x"].to(DEV)
    dw = c["dst_w"].to(DEV)
    dw.addmm_(dy.t(), x)
    _record("wgrad_lib", cid, "dw", dw, c["exact"]["dw"], c["rounded"]["dw"],
            -1)
    if cc["bias"] == "dst":
        db = c["dst_b"].to(DEV)
        m.colsum(dy, db)
        _record("wgrad_lib", cid, "db", db, c["exact"]["db"],
                c["rounded"]["db"], None)
    elif cc["bias"] == "f32":
        _record("wgrad_lib", cid, "db32", m.colsum(dy), c["db32_exact"],
                c["db32_rounded"], None, fp32_out=True)


@pytest.mark.parametrize("cr", W.CASE_REGIMES,
                         ids=[W.case_id(cr) for cr in W.CASE_REGIMES])
def test_accuracy(cr):
    c = W.case(*cr)
    cid = W.case_id(cr)
    dw, bias = _run(c)
    _library(c, cid)
    N.check("wgrad", cid, "dw", dw, c["exact"]["dw"], c["rounded"]["dw"],
            row_dim=-1)
    if c["c"]["bias"] == "dst":
        N.check("wgrad", cid, "db", bias, c["exact"]["db"],
                c["rounded"]["db"], row_dim=None)
    elif c["c"]["bias"] == "f32":
        N.check("wgrad", cid, "db32", bias, c["db32_exact"],
                c["db32_rounded"], row_dim=None, fp32_out=True)


# cases 3 / 4: 6 BK + 17 rows with a bf16 and an fp32 bias
@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("i", [3, 4])
def test_bit_repeatable(i, nsplit):
    c = W.case(i, "randn")
    dw0, b0 = _run(c, nsplit)
    dw1, b1 = _run(c, nsplit)
    assert torch.equal(dw0, dw1)
    assert torch.equal(b0, b1)


# ---------------------------------------------------------------------------
# routing: a two-layer model, linear -> GELU MLP, gradients into a flat plane
# ---------------------------------------------------------------------------
E, HID, ROWS = 2 * W.BM, 4 * W.BM, 300
NAMES = ("wa", "ba", "w1", "b1", "w2", "b2")
SHAPES = dict(wa=(E, E), ba=(E,), w1=(HID, E), b1=(HID,), w2=(E, HID),
              b2=(E,))


def _params():
    """bf16 leaves with main_grad views carved out of one zeroed plane,
    unpadded and starting at an odd element as parallel.flat lays them out."""
    ps = {n: N.randn_bf16(*SHAPES[n], seed=1300 + i, scale=0.05).to(DEV)
          .requires_grad_(True) for i, n in enumerate(NAMES)}
    plane = torch.zeros(1 + sum(p.numel() for p in ps.values()),
                        dtype=torch.bfloat16, device=DEV)
    o = 1
    for n in NAMES:
        ps[n].main_grad = plane[o:o + ps[n].numel()].view(SHAPES[n])
        o += ps[n].numel()
    return ps, plane


def _model_inputs():
    x = N.randn_bf16(ROWS, E, seed=1310, scale=0.5).to(DEV)
    dy = N.randn_bf16(ROWS, E, seed=1311, scale=0.05).to(DEV)
    return x.requires_grad_(True), dy


def _forward(ops, ps, x):
    h = ops.linear(x, ps["wa"], ps["ba"])
    return h, ops.mlp_gelu(h, ps["w1"], ps["b1"], ps["w2"], ps["b2"])


@pytest.fixture()
def composed_mlp(monkeypatch):
    """Both settings on the composed MLP node, whatever hipBLASLt offers."""
    from distributedtraining_amd import ops
    monkeypatch.setitem(ops._lt_fused_shape_ok, (ROWS, HID, E), False)
    was = ops.mlp_node_enable(True)
    yield ops
    ops.mlp_node_enable(was)


def _model_run(ops, mode):
    ps, plane = _params()
    x, dy = _model_inputs()
    was = ops.wgrad_route(mode)
    try:
        h, y = _forward(ops, ps, x)
        h.retain_grad()
        y.backward(dy)
        torch.cuda.synchronize()
    finally:
        ops.wgrad_route(was)
    assert all(ps[n].grad is None for n in NAMES)
    return dict(ps=ps, x=x, dy=dy, h=h.detach(), dh=h.grad, y=y.detach(),
                dx=x.grad, g={n: ps[n].main_grad for n in NAMES})


def test_routing_switch(composed_mlp):
    ops = composed_mlp
    m = _ext()
    on, off = _model_run(ops, "1"), _model_run(ops, "0")
    # wgrad feeds neither the forward nor dx
    assert torch.equal(on["y"], off["y"])
    assert torch.equal(on["dx"], off["dx"])
    assert torch.equal(on["dh"], off["dh"])
    # (dy, x) of every linear, rebuilt from the run's own tensors
    ps = on["ps"]
    with torch.no_grad():
        pre = torch.addmm(ps["b1"], on["h"], ps["w1"].t())
        act = m.gelu_fwd(pre)
        dh_pre = m.gelu_bwd(on["dy"].mm(ps["w2"]), pre)
    lin = dict(wa=(on["dh"], on["x"].detach()), w1=(dh_pre, on["h"]),
               w2=(on["dy"], act))
    bias_of = dict(wa="ba", w1="b1", w2="b2")
    for tag, run in (("on", on), ("off", off)):
        for wn, (dyl, xl) in lin.items():
            exact = N.d(dyl).t() @ N.d(xl)
            N.check("wgrad_route", tag, wn, run["g"][wn], exact,
                    N.bf16(exact), row_dim=-1)
            bexact = N.d(dyl).sum(0)
            N.check("wgrad_route", tag, bias_of[wn], run["g"][bias_of[wn]],
                    bexact, N.bf16(bexact), row_dim=None)
    # the switch did change the path: the library sums in another order
    assert not all(torch.equal(on["g"][n], off["g"][n])
                   for n in ("wa", "w1", "w2"))


def test_out_of_contract_falls_back(composed_mlp):
    """64-wide layers are outside the tile contract: the forced route leaves
    them to the library, bit for bit."""
    ops = composed_mlp
    m = _ext()
    x = N.randn_bf16(40, 64, seed=1320).to(DEV)
    assert not m.wgrad.supported(x, x)
    res = []
    for mode in ("1", "0"):
        w = N.randn_bf16(64, 64, seed=1321, scale=0.1).to(DEV) \
            .requires_grad_(True)
        b = N.randn_bf16(64, seed=1322).to(DEV).requires_grad_(True)
        w.main_grad = torch.zeros_like(w)
        b.main_grad = torch.zeros_like(b)
        was = ops.wgrad_route(mode)
        try:
            ops.linear(x, w, b).backward(x)
        finally:
            ops.wgrad_route(was)
        res.append((w.main_grad, b.main_grad))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    with pytest.raises(RuntimeError):
        m.wgrad.bias(x, x, torch.zeros(64, 64, dtype=torch.bfloat16,
                                       device=DEV))


def test_graph_capture(composed_mlp):
    ops = composed_mlp
    ps, plane = _params()
    x, dy = _model_inputs()
    was = ops.wgrad_route("1")

    def step():
        x.grad = None
        _, y = _forward(ops, ps, x)
        y.backward(dy)
        return y.detach(), x.grad

    try:
        for _ in range(2):
            want = [t.clone() for t in step()]
        want_plane = plane.clone()      # two accumulating passes
        assert bool(want_plane.float().abs().sum() > 0)
        plane.zero_()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        plane.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            got = step()
        g.replay()
        g.replay()
        torch.cuda.synchronize()
    finally:
        ops.wgrad_route(was)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert torch.equal(plane, want_plane)
