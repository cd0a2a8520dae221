"""The forward projection GEMM (hip/gemm.hip) on the GPU: accuracy of its three
epilogues against the fp64 references of tests/_gemm_cases.py under the bounds
of tests/_numerics.py, h bit for bit against gelu_fwd of the stored pre, the
routing switch on a two-layer model with its backward, and a captured replay."""

import pytest
import torch

import _gemm_cases as G
import _numerics as N

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
    assert tuple(_ext().gemm.tile()) == (G.BM, G.BN, G.BK)


def _operand(t, pad):
    """t on the GPU as a view whose row stride is pad elements larger than
    its width (16 B aligned base)."""
    if not pad:
        return t.to(DEV)
    buf = torch.full((t.shape[0], t.shape[1] + pad), 7.0,
                     dtype=torch.bfloat16, device=DEV)
    v = buf[:, :t.shape[1]]
    v.copy_(t)
    return v


@pytest.mark.parametrize("p", G.PARAMS, ids=[G.param_id(p) for p in G.PARAMS])
def test_accuracy(p):
    m = _ext()
    i, regime, epi = p
    c = G.case(i, regime)
    x, w = _operand(c["x"], c["pad"]), c["w"].to(DEV)
    out = m.gemm.fwd(x, w, None if epi == "none" else c["b"].to(DEV), epi)
    y, h = out if epi == "bias_gelu" else (out, None)
    exact = c["none" if epi == "none" else "bias"]
    assert y.shape == exact.shape and y.is_contiguous()
    N.check("gemm", G.param_id(p), "pre" if h is not None else "y", y, exact,
            N.bf16(exact), row_dim=-1)
    if h is not None:
        assert torch.equal(h, m.gelu_fwd(y))
    # both K-loop pipelines feed each accumulator the same MFMA sequence
    for pipe in (1, 2):
        o2 = m.gemm.fwd(x, w, None if epi == "none" else c["b"].to(DEV), epi,
                        pipe)
        for a, b in zip(o2 if h is not None else (o2,), (y, h)):
            assert torch.equal(a, b), f"pipe {pipe}"


# ---------------------------------------------------------------------------
# routing: a two-layer model, linear -> GELU MLP, gradients into a flat plane
# ---------------------------------------------------------------------------
E, HID, ROWS = 2 * G.BN, 4 * G.BN, 300
NAMES = ("wa", "ba", "w1", "b1", "w2", "b2")
SHAPES = dict(wa=(E, E), ba=(E,), w1=(HID, E), b1=(HID,), w2=(E, HID),
              b2=(E,))


def _params():
    """bf16 leaves (their own allocations, as the working copy's 16 B aligned
    weights) with main_grad views carved out of one zeroed plane."""
    ps = {n: N.randn_bf16(*SHAPES[n], seed=1500 + i, scale=0.05).to(DEV)
          .requires_grad_(True) for i, n in enumerate(NAMES)}
    plane = torch.zeros(1 + sum(p.numel() for p in ps.values()),
                        dtype=torch.bfloat16, device=DEV)
    o = 1
    for n in NAMES:
        ps[n].main_grad = plane[o:o + ps[n].numel()].view(SHAPES[n])
        o += ps[n].numel()
    return ps, plane


def _model_inputs():
    x = N.randn_bf16(ROWS, E, seed=1510, scale=0.5).to(DEV)
    dy = N.randn_bf16(ROWS, E, seed=1511, scale=0.05).to(DEV)
    return x.requires_grad_(True), dy


def _forward(ops, ps, x):
    h = ops.linear(x, ps["wa"], ps["ba"])
    return h, ops.mlp_gelu(h, ps["w1"], ps["b1"], ps["w2"], ps["b2"])


@pytest.fixture()
def composed_mlp(monkeypatch):
    """The composed MLP node, whatever hipBLASLt offers."""
    from distributedtraining_amd import ops
    monkeypatch.setitem(ops._lt_fused_shape_ok, (ROWS, HID, E), False)
    monkeypatch.setitem(ops._lt_fused_shape_ok, (40, 64, 64), False)
    was = ops.mlp_node_enable(True)
    yield ops
    ops.mlp_node_enable(was)


def _model_run(ops, mode):
    ps, _plane = _params()
    x, dy = _model_inputs()
    was = ops.gemm_route(mode)
    try:
        h, y = _forward(ops, ps, x)
        h.retain_grad()
        y.backward(dy)
        torch.cuda.synchronize()
    finally:
        ops.gemm_route(was)
    return dict(ps=ps, x=x.detach(), dy=dy, h=h.detach(), dh=h.grad,
                y=y.detach(), g={n: ps[n].main_grad for n in NAMES})


def test_routing(composed_mlp):
    ops = composed_mlp
    m = _ext()
    on, off = _model_run(ops, "1"), _model_run(ops, "0")
    ps = on["ps"]
    # (a) the routed ops are the kernel: the same chain written with it
    with torch.no_grad():
        h0 = m.gemm.fwd(on["x"], ps["wa"], ps["ba"], "bias")
        pre, act = m.gemm.fwd(h0, ps["w1"], ps["b1"], "bias_gelu")
        y = m.gemm.fwd(act, ps["w2"], ps["b2"], "bias")
    assert torch.equal(on["h"], h0) and torch.equal(on["y"], y)
    # (b) both routes against fp64 with the bf16 roundings at h0, pre and h
    w = {n: N.d(ps[n]) for n in NAMES}
    r_h0 = N.bf16(N.d(on["x"]) @ w["wa"].t() + w["ba"])
    r_pre = N.bf16(r_h0 @ w["w1"].t() + w["b1"])
    exact = N.bf16(N.gelu(r_pre, r_pre)["y"]) @ w["w2"].t() + w["b2"]
    for tag, run in (("on", on), ("off", off)):
        N.check("gemm_route", tag, "y", run["y"], exact, N.bf16(exact))
    # (c) the backward of the routed run, rebuilt from its own tensors: the
    # kernel's pre, dh = bf16(dy w2)
    dh = N.bf16(N.d(on["dy"]) @ w["w2"])
    dh_pre = N.bf16(N.gelu(N.d(pre), dh)["dx"])
    for name, got, ex, row in (
            ("dx", on["dh"], dh_pre @ w["w1"], -1),
            ("w1", on["g"]["w1"], dh_pre.t() @ N.d(h0), -1),
            ("b1", on["g"]["b1"], dh_pre.sum(0), None)):
        N.check("gemm_route", "on", name, got, ex, N.bf16(ex), row_dim=row)


def test_out_of_contract_falls_back(composed_mlp):
    """(d) 64-wide layers are outside the tile contract: the forced route
    leaves them to the library, bit for bit."""
    ops = composed_mlp
    m = _ext()
    x = N.randn_bf16(40, 64, seed=1520).to(DEV)
    w = N.randn_bf16(64, 64, seed=1521, scale=0.1).to(DEV)
    b = N.randn_bf16(64, seed=1522).to(DEV)
    assert not m.gemm.supported(x, w)
    res = []
    for mode in ("1", "0"):
        was = ops.gemm_route(mode)
        try:
            with torch.no_grad():
                res.append((ops.linear(x, w, b), ops.mlp_gelu(x, w, b, w, b)))
        finally:
            ops.gemm_route(was)
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    with pytest.raises(RuntimeError):
        m.gemm.fwd(x, w, b, "bias")


def test_graph_capture(composed_mlp):
    ops = composed_mlp
    ps, plane = _params()
    x, dy = _model_inputs()
    was = ops.gemm_route("1")

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
        ops.gemm_route(was)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert torch.equal(plane, want_plane)
