"""Accuracy of every HIP kernel against an fp64 reference, at bounds that are
measured and not chosen (tests/_numerics.py): a bf16 output may be 3 x as far
from the fp64 truth as the same computation rounded to bf16 where the kernel
rounds; an fp32 output 16 x as far as the formula in fp32 torch, never held to
less than 4 fp32 ulp. tests/test_numerics_selfcheck.py shows on the CPU, on
these very inputs, that the bounds reject a scale wrong by 3%, one lost
probability, one wrong dropout draw, and the other mutants listed there.

Every check prints its figures before it asserts; with DTA_ACCURACY_REPORT
set to a file name the rows are also written there as JSON
(tools/accuracy_table.py turns them into docs/test_accuracy.md).

Run on the MI355X box: python -m pytest tests/test_kernel_accuracy_gpu.py -m gpu
"""

import os
import re

import pytest
import torch

import _numerics as N

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from distributedtraining_amd.ops.backend import require_ext
    return require_ext()


def _i32(*vals):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


def _empty(dtype):
    return torch.empty(0, dtype=dtype, device=DEV)


@pytest.fixture(scope="module", autouse=True)
def _accuracy_report():
    yield
    N.dump_report()


# ---------------------------------------------------------------------------
# Training attention: ops.causal_attention on strided views of the packed
# projection and ops.qkv_attention on the packed layout itself
# ---------------------------------------------------------------------------
def _pack(c, B, H, Hk, S, D):
    """[B, S, (H + 2 Hk) D] projection buffer holding the case's q, k, v."""
    parts = [c[n].permute(0, 2, 1, 3).reshape(B, S, -1) for n in "qkv"]
    return torch.cat(parts, dim=-1).contiguous().to(DEV)


def _unpack(t, H, Hk, D):
    """q/k/v [B,heads,S,D] strided views of a packed tensor."""
    B, S, _ = t.shape
    E, kvd = H * D, Hk * D
    return (t[..., :E].view(B, S, H, D).transpose(1, 2),
            t[..., E:E + kvd].view(B, S, Hk, D).transpose(1, 2),
            t[..., E + kvd:].view(B, S, Hk, D).transpose(1, 2))


@pytest.mark.parametrize("entry", ["views", "packed"])
@pytest.mark.parametrize("case", N.ATTN_CASES, ids=N.case_id)
def test_attention_fwd_bwd_accuracy(case, entry):
    from distributedtraining_amd import ops
    from distributedtraining_amd.ops import droprng
    shape, _regime, kv, p = case
    B, H, Hk, S, D = shape
    c = N.attn_case(case)
    m = _ext()
    kvlen = None if kv is None else c["kvlen"].to(DEV)
    qkv = _pack(c, B, H, Hk, S, D)
    droprng.counter(DEV).fill_(N.DROP_CTR)
    was = m.attn_bwd_fused_enable(True)
    try:
        n0 = m.attn_bwd_fused_calls()
        if entry == "packed":
            qkv.requires_grad_(True)
            o = ops.qkv_attention(qkv, H, Hk, scale=c["scale"], kvlen=kvlen,
                                  p_drop=p, site=N.DROP_SITE)
            o.backward(c["do"].permute(0, 2, 1, 3).reshape(B, S, H * D)
                       .contiguous().to(DEV))
            o = o.view(B, S, H, D).transpose(1, 2)
            dq, dk, dv = _unpack(qkv.grad, H, Hk, D)
        else:
            q, k, v = (t.detach().requires_grad_(True)
                       for t in _unpack(qkv, H, Hk, D))
            assert not q.is_contiguous() or S == 1
            o = ops.causal_attention(q, k, v, c["scale"], kvlen=kvlen,
                                     p_drop=p, site=N.DROP_SITE)
            o.backward(c["do"].to(DEV))
            dq, dk, dv = q.grad, k.grad, v.grad
        torch.cuda.synchronize()
        n_fused = m.attn_bwd_fused_calls() - n0
    finally:
        m.attn_bwd_fused_enable(was)
    # the cases meant for the single-tile fused backward took it
    assert n_fused == (1 if N.attn_fused_expected(shape) else 0)
    if shape in N.ATTN_FUSED_SHAPES:
        assert n_fused == 1
    got = dict(o=o.detach(), dq=dq, dk=dk, dv=dv)
    for name in N.ATTN_TENSORS:
        assert bool(torch.isfinite(got[name].float()).all()), name
    failures = []
    for name in N.ATTN_TENSORS:
        try:
            N.check("attention", f"{N.case_id(case)}/{entry}", name,
                    got[name], c["exact"][name], c["rounded"][name],
                    live=N.attn_live(c, name))
        except AssertionError as e:      # report every tensor, then fail
            failures.append(str(e))
    assert not failures, "\n".join(failures)
    if kv is not None:
        # padded keys receive exactly zero gradient
        for b in range(B):
            L = min(kv[b], S)
            assert torch.all(dk[b, :, L:] == 0)
            assert torch.all(dv[b, :, L:] == 0)


# ---------------------------------------------------------------------------
# Decode attention
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.DECODE_CASES, ids=str)
def test_decode_attention_accuracy(case):
    from distributedtraining_amd import ops
    _B, _H, _Hk, L, _D, _regime = case
    c = N.decode_case(case)
    kc, vc = c["kc"].to(DEV), c["vc"].to(DEV)
    assert kc.shape[2] > L                  # cache longer than the prefix
    out = ops.decode_attention(c["q"].to(DEV), kc, vc, L, c["scale"])
    N.check("decode_attention", str(case), "o", out, c["exact"],
            c["rounded"])
    # the device-counter form (cache position BEFORE the token) agrees
    out2 = ops.decode_attention(c["q"].to(DEV), kc, vc, 0, c["scale"],
                                kv_len_dev=_i32(L - 1))
    assert torch.equal(out, out2)


# ---------------------------------------------------------------------------
# Cross entropy: ce_fwd + ce_bwd, ce_fwd_bwd (default and LDS-row variant)
# ---------------------------------------------------------------------------
def _ce_check(case, variant, c, loss_sum, lse, count, dlogits):
    tg = c["tg"]
    ex, rd = c["exact"], c["rounded"]
    name = f"{case}/{variant}"
    fails = []

    def chk(*a, **kw):
        try:
            N.check("cross_entropy", name, *a, **kw)
        except AssertionError as e:
            fails.append(str(e))

    chk("lse", lse, ex["lse"], rd["lse"], row_dim=None, fp32_out=True)
    chk("loss_sum", loss_sum.reshape(1), ex["loss_sum"].reshape(1),
        rd["loss_sum"].reshape(1), row_dim=None, fp32_out=True,
        ulp_of=N.ce_valid_lse(c))
    assert int(count) == ex["count"]
    chk("dlogits", dlogits, ex["dlogits"], rd["dlogits"])
    # the target column alone, so a large vocabulary cannot dilute it
    chk("dlogits[target]", N.ce_target_entries(dlogits, tg),
        N.ce_target_entries(ex["dlogits"], tg),
        N.ce_target_entries(rd["dlogits"], tg), row_dim=None)
    assert not fails, "\n".join(fails)
    # ignored rows get exactly no gradient
    assert torch.all(dlogits.cpu()[tg == -100] == 0)


@pytest.mark.parametrize("case", N.CE_CASES, ids=str)
def test_cross_entropy_accuracy(case):
    m = _ext()
    c = N.ce_case(case)
    x, tg = c["x"].to(DEV), c["tg"].to(DEV)
    loss_sum, lse, count = m.ce_fwd(x, tg, -100)
    sdev = torch.tensor([c["scale"]], dtype=torch.float32, device=DEV)
    assert float(sdev) == c["scale"]
    dl = m.ce_bwd(x, tg, lse, _empty(torch.float32), c["scale"], -100, 0,
                  True)
    # device-scale and host-scale backward stay equal
    dl_dev = m.ce_bwd(x, tg, lse, sdev, 0.0, -100, 0, True)
    assert torch.equal(dl, dl_dev)
    _ce_check(case, "ce_fwd+ce_bwd", c, loss_sum, lse, count, dl)
    for lds_row in (False, True):
        buf = x.clone()
        loss2, lse2, count2 = m.ce_fwd_bwd(buf, tg, -100, sdev, 0, lds_row)
        _ce_check(case, "ce_fwd_bwd" + ("(lds)" if lds_row else ""), c,
                  loss2, lse2, count2, buf)


def test_head_loss_accuracy():
    m = _ext()
    c = N.head_loss_case()
    loss_sum, lse, count, _tl = m.head_loss_fwd(
        c["x"].to(DEV), c["w"].to(DEV), c["tg"].to(DEV), -100, 0)
    ex, rd = c["exact"], c["rounded"]
    name = str(N.HEAD_LOSS_SHAPE)
    N.check("head_loss_fwd", name, "lse", lse, ex["lse"], rd["lse"],
            row_dim=None, fp32_out=True)
    N.check("head_loss_fwd", name, "loss_sum", loss_sum.reshape(1),
            ex["loss_sum"].reshape(1), rd["loss_sum"].reshape(1),
            row_dim=None, fp32_out=True, ulp_of=N.ce_valid_lse(c))
    assert int(count) == ex["count"]


# ---------------------------------------------------------------------------
# LayerNorm / RMSNorm through the ops layer (as the models call them)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.NORM_CASES, ids=str)
def test_norm_fwd_bwd_accuracy(case):
    from distributedtraining_amd import ops
    from distributedtraining_amd.ops import droprng
    _rows, _cols, kind, _regime, form = case
    c = N.norm_case(case)
    t = {k: v.to(DEV) for k, v in c["t"].items()}
    x, res, w = (t[n].requires_grad_(True) for n in ("x", "res", "w"))
    b = t["b"].requires_grad_(True) if kind == "layer" else None
    s = None
    if form == "plain":
        y = (ops.layer_norm(x, w, b, N.NORM_EPS) if kind == "layer"
             else ops.rms_norm(x, w, N.NORM_EPS))
        y.backward(t["dy"])
    else:
        p, site, ctr = N.NORM_DROP if form == "dropout" else (0.0, 0, 0)
        droprng.counter(DEV).fill_(ctr)
        if kind == "layer":
            s, y = ops.add_layer_norm(x, res, w, b, N.NORM_EPS, p, site)
        else:
            s, y = ops.add_rms_norm(x, res, w, N.NORM_EPS, p, site)
        torch.autograd.backward([s, y], [t["ds"], t["dy"]])
    got = dict(y=y.detach(), dx=x.grad, dw=w.grad,
               db=None if b is None else b.grad,
               s=None if s is None else s.detach(), dres=res.grad)
    fails = []
    for name, row_dim in N.norm_tensors(case):
        try:
            N.check("norm", str(case), name, got[name], c["exact"][name],
                    c["rounded"][name], row_dim=row_dim)
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)
    if form == "dropout":
        # dropped branch positions get exactly zero gradient
        assert torch.all(res.grad.cpu()[~c["keep"]] == 0)


# ---------------------------------------------------------------------------
# GELU / SwiGLU
# ---------------------------------------------------------------------------
def _ew_check(case_name, parts, got, exact, rounded):
    fails = []
    for op, names in (("gelu", ("y", "dx")),
                      ("swiglu", ("y", "dgate", "dup"))):
        for name in names:
            for label, sl in parts:
                try:
                    N.check(op, f"{case_name}/{label}", name,
                            got[op][name][sl], exact[op][name][sl],
                            rounded[op][name][sl], row_dim=None)
                except AssertionError as e:
                    fails.append(str(e))
    assert not fails, "\n".join(fails)


def _ew_run(x, up, dy):
    m = _ext()
    x, up, dy = x.to(DEV), up.to(DEV), dy.to(DEV)
    dg, du = m.swiglu_bwd(dy, x, up)
    return dict(gelu=dict(y=m.gelu_fwd(x), dx=m.gelu_bwd(dy, x)),
                swiglu=dict(y=m.swiglu_fwd(x, up), dgate=dg, dup=du))


@pytest.mark.parametrize("case", N.EW_CASES, ids=str)
def test_gelu_swiglu_accuracy(case):
    c = N.ew_case(case)
    got = _ew_run(c["x"], c["up"], c["dy"])
    _ew_check(str(case), N.ew_parts(case), got,
              dict(gelu=c["gelu_exact"], swiglu=c["swiglu_exact"]),
              dict(gelu=c["gelu_rounded"], swiglu=c["swiglu_rounded"]))


def _max_resident_blocks() -> int:
    from distributedtraining_amd import ops
    path = os.path.join(os.path.dirname(ops.__file__), "hip", "dta_common.h")
    with open(path) as f:
        mt = re.search(r"MAX_RESIDENT_BLOCKS\s*=\s*(\d+)", f.read())
    return int(mt.group(1))


def test_gelu_swiglu_grid_loop_accuracy():
    """A length past MAX_RESIDENT_BLOCKS x 256 threads x 16 elements: the
    capped grid makes the threads of both maps go round again (SwiGLU, at 8
    elements per thread, twice)."""
    n = N.ew_loop_n(_max_resident_blocks())
    case = (n, "randn2")
    c = N.ew_case.__wrapped__(case)        # too large to keep cached
    got = _ew_run(c["x"], c["up"], c["dy"])
    _ew_check(f"({n}, 'loop')", N.ew_parts(case), got,
              dict(gelu=c["gelu_exact"], swiglu=c["swiglu_exact"]),
              dict(gelu=c["gelu_rounded"], swiglu=c["swiglu_rounded"]))


# ---------------------------------------------------------------------------
# RoPE: forward and backward each against the explicit rotation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.ROPE_CASES, ids=str)
def test_rope_accuracy(case):
    m = _ext()
    _bh, S, _D, pos = case
    c = N.rope_case(case)
    x = c["x"].to(DEV)
    cos, sin = c["cos"].to(DEV), c["sin"].to(DEV)
    assert cos.shape[0] >= pos + S
    # a device position offset that points at a nonzero table row
    pos_t = _i32(pos) if pos else _empty(torch.int32)
    N.check("rope", str(case), "fwd", m.rope_fwd(x, cos, sin, pos_t),
            c["fwd_exact"], c["fwd_rounded"])
    N.check("rope", str(case), "bwd", m.rope_bwd(x, cos, sin, pos_t),
            c["bwd_exact"], c["bwd_rounded"])


# ---------------------------------------------------------------------------
# Embedding
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.EMB_CASES, ids=str)
def test_embedding_accuracy(case):
    m = _ext()
    V, P, _E, _B, _S, _kind, pos = case
    c = N.emb_case(case)
    ids = c["ids"].to(DEV)
    pos_t = _i32(pos) if pos else _empty(torch.int32)
    y = m.embedding_fwd(ids, c["wte"].to(DEV), c["wpe"].to(DEV), pos_t)
    N.check("embedding", str(case), "y", y, c["exact"]["y"],
            c["rounded"]["y"])
    dwte, dwpe = m.embedding_bwd(c["dy"].to(DEV), ids, V, P)
    for name, got in (("dwte", dwte), ("dwpe", dwpe)):
        N.check("embedding", str(case), name, got, c["exact"][name],
                c["rounded"][name], fp32_out=True)


# ---------------------------------------------------------------------------
# Flat plane
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bias_correction", ["host", "device"])
def test_adamw_accuracy(bias_correction):
    """Three steps; the reference receives the bf16 gradient the kernel
    reads. ``device``: the bias correction comes from the adamw_tick buffer
    (the hipGraph-capturable path)."""
    from distributedtraining_amd import ops
    c = N.adamw_case()
    hp = N.ADAMW_HP
    master = c["master"].to(DEV)
    mm, vv = torch.zeros_like(master), torch.zeros_like(master)
    work = torch.empty(N.ADAMW_N, dtype=torch.bfloat16, device=DEV)
    t_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    bc = torch.zeros(2, dtype=torch.float32, device=DEV)
    for t, g in enumerate(c["grads"], start=1):
        if bias_correction == "device":
            ops.adamw_tick(t_dev, bc, hp["beta1"], hp["beta2"])
        ops.adamw_step(master, g.to(DEV), mm, vv, work, t, hp["lr"],
                       hp["beta1"], hp["beta2"], hp["eps"], hp["wd"],
                       bc=bc if bias_correction == "device" else None)
    got = dict(master=master, m=mm, v=vv, work=work)
    for name, fp32 in N.ADAMW_TENSORS:
        N.check("adamw", bias_correction, name, got[name], c["exact"][name],
                c["rounded"][name], row_dim=None, fp32_out=fp32)


@pytest.mark.parametrize("n", [1, 1023, 100_003, (1 << 21) + 5])
def test_l2norm_sq_accuracy(n):
    m = _ext()
    x = torch.randn(n, generator=torch.Generator().manual_seed(22))
    got = torch.tensor([m.l2norm_sq(x.to(DEV))], dtype=N.F64)
    N.check("l2norm_sq", str(n), "sum", got, N.l2norm_sq(N.d(x)).reshape(1),
            N.l2norm_sq(N.d(x), "rounded").reshape(1), row_dim=None,
            fp32_out=True)


@pytest.mark.parametrize("rows,cols", [(1, 8), (333, 520), (4099, 24)])
def test_colsum_accuracy(rows, cols):
    m = _ext()
    x = N.randn_bf16(rows, cols, seed=23)
    N.check("colsum", f"({rows}, {cols})", "sum", m.colsum(x.to(DEV)),
            N.colsum(N.d(x)), N.colsum(N.d(x), "rounded"), row_dim=None,
            fp32_out=True)


@pytest.mark.parametrize("n,alpha", [(4099, -0.37), (1, 2.5),
                                     ((1 << 21) + 3, 1e-3)])
def test_axpy_accuracy(n, alpha):
    m = _ext()
    g = torch.Generator().manual_seed(24)
    w, x = torch.randn(n, generator=g), torch.randn(n, generator=g)
    wd = w.to(DEV)
    m.axpy(wd, x.to(DEV), alpha)
    N.check("axpy", f"({n}, {alpha})", "w", wd,
            N.axpy(N.d(w), N.d(x), alpha),
            N.axpy(N.d(w), N.d(x), alpha, "rounded"), row_dim=None,
            fp32_out=True)


@pytest.mark.parametrize("n", [1, 3, 4, 4099])
def test_delta_sub_equals_torch(n):
    """One fp32 subtraction per element: torch.sub's bits (a scalar tail and
    whole 4-wide vectors)."""
    m = _ext()
    g = torch.Generator().manual_seed(26)
    w, base = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
    out = torch.full((n,), float("nan"), device=DEV)
    m.delta_sub(w.to(DEV), base.to(DEV), out)
    assert torch.equal(out.cpu(), torch.sub(w, base))


ACCUM_GUARD = 8     # elements in front of the slice: a 16 B aligned start


def _accum_loop_n():
    # 8 elements per lane and iteration: the capped grid goes round again
    return _max_resident_blocks() * 256 * 8 + 4099


@pytest.mark.parametrize("n,offs", [(1, (0, 1, 3)), (7, (0, 1, 3)),
                                    (8, (0, 1, 3)), (4099, (0, 1, 3)),
                                    ("loop", (1,))])
def test_accum_f32_into_bf16_accuracy(n, offs):
    """dst += src on a slice of a larger bf16 plane that starts 0, 1 and 3
    elements off a 16 B boundary (a flat-grad view of any parameter); the
    neighbours on both sides keep their bits."""
    m = _ext()
    n = _accum_loop_n() if n == "loop" else n
    src = torch.randn(n, generator=torch.Generator().manual_seed(27))
    for off in offs:
        plane = N.randn_bf16(ACCUM_GUARD + off + n + 9, seed=28 + off)
        lo, hi = ACCUM_GUARD + off, ACCUM_GUARD + off + n
        exact = N.d(plane[lo:hi]) + N.d(src)
        dev = plane.to(DEV)
        assert dev.data_ptr() % 16 == 0
        m.accum_f32_into_bf16(dev[lo:hi], src.to(DEV))
        got = dev.cpu()
        assert torch.equal(got[:lo].view(torch.int16),
                           plane[:lo].view(torch.int16))
        assert torch.equal(got[hi:].view(torch.int16),
                           plane[hi:].view(torch.int16))
        N.check("accum_f32_into_bf16", f"({n}, +{off})", "dst", got[lo:hi],
                exact, N.bf16(exact), row_dim=None)


# ---------------------------------------------------------------------------
# Serving GEMV
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.GEMV_CASES, ids=str)
def test_gemv_accuracy(case):
    m = _ext()
    c = N.gemv_case(case)
    b = (_empty(torch.bfloat16) if c["b"] is None else c["b"].to(DEV))
    y = m.gemv(c["x"].to(DEV), c["w"].to(DEV), b)
    assert y.shape == (case[0], case[1]) and y.dtype == torch.bfloat16
    N.check("gemv", str(case), "y", y, c["exact"], c["rounded"])


@pytest.mark.parametrize("M,K", [(1, 8200), (3, 2056)])
def test_linear_routes_small_m_to_gemv(M, K):
    """ops.linear under no_grad on a non-contiguous [M, 1, K] input returns
    gemv's bits: the routing and its .contiguous() copy."""
    from distributedtraining_amd import ops
    m = _ext()
    x, w, b = (t.to(DEV) for t in N.gemv_inputs(M, 5, K, "bf16", "randn"))
    wide = torch.zeros(M, 1, K + 8, dtype=torch.bfloat16, device=DEV)
    wide[..., :K] = x[:, None]
    xv = wide[..., :K]
    assert not xv.is_contiguous() or M == 1
    with torch.no_grad():
        y = ops.linear(xv, w, b)
        y_nobias = ops.linear(xv, w)
    assert y.shape == (M, 1, 5)
    assert torch.equal(y.view(M, 5), m.gemv(x, w, b))
    assert torch.equal(y_nobias.view(M, 5),
                       m.gemv(x, w, _empty(torch.bfloat16)))


# ---------------------------------------------------------------------------
# Merge plane on fp32 deltas (the packed kernels are held bit-identical to
# these in tests/test_packed_merge_gpu.py)
# ---------------------------------------------------------------------------
def _merge_run(c):
    m = _ext()
    out = torch.full((c["P"],), float("nan"), device=DEV)
    m.weighted_merge(c["base"].to(DEV), c["deltas"].to(DEV), c["W"].to(DEV),
                     c["offsets"].to(DEV), out)
    return out


@pytest.mark.parametrize("case", N.MERGE_CASES, ids=str)
def test_weighted_merge_accuracy(case):
    c = N.merge_case(case)
    N.check("weighted_merge", str(case), "merged", _merge_run(c), c["exact"],
            c["rounded"], row_dim=None, fp32_out=True)


def test_weighted_merge_grid_loop_accuracy():
    """A plane past MAX_RESIDENT_BLOCKS x 256 elements: the capped grid goes
    round a second time."""
    mrb = _max_resident_blocks()
    c = N.merge_case_uncached(N.merge_loop_table(mrb), 3, "rand")
    assert c["P"] > mrb * 256
    N.check("weighted_merge", f"({c['P']}, 'loop')", "merged", _merge_run(c),
            c["exact"], c["rounded"], row_dim=None, fp32_out=True)


@pytest.mark.parametrize("case", N.GRADW_CASES, ids=str)
def test_grad_merge_weights_accuracy(case):
    """grad_W with ``merged`` given (the fp64 merge rounded to fp32), against
    fp64 and an fp32 baseline that sums in the kernel's order. The d1e-3 and
    d1e-5 regimes are the production ones, W = 1/N, where the summand
    cancels: (base + d) - merged, the order grad_w_k used to have, measured
    1e-5 to 1e-4 and 1e-3 to 8e-3 there against bounds of 1.5e-6 to 2e-5
    (docs/test_accuracy.md)."""
    m = _ext()
    big = case[0] == "big"
    c = N.gradw_case_uncached(case) if big else N.gradw_case(case)
    gw = m.grad_merge_weights(c["g_in"].to(DEV), c["base"].to(DEV),
                              c["deltas"].to(DEV), c["merged"].to(DEV),
                              c["offsets"].to(DEV))
    assert gw.shape == c["exact"].shape and gw.dtype == torch.float32
    N.check("grad_merge_weights", str(case), "grad_W", gw, c["exact"],
            c["rounded"], row_dim=None, fp32_out=True)


def test_merge_bindings_reject_bad_arguments():
    """Every bad argument raises before anything is launched."""
    m = _ext()
    P, n = 1024, 2
    base = torch.zeros(P, device=DEV)
    deltas = torch.zeros(n, P, device=DEV)
    W = torch.ones(n, 1, device=DEV)
    offs = torch.tensor([0, P], device=DEV)
    out = torch.empty(P, device=DEV)
    g = torch.ones(P, device=DEV)
    m.weighted_merge(base, deltas, W, offs, out)
    ref = m.grad_merge_weights(g, base + 1, deltas, base, offs)
    assert ref.tolist() == [[float(P)], [float(P)]]
    # an int32 table is converted, not read as int64
    offs32 = torch.tensor([0, 1000, P], dtype=torch.int32, device=DEV)
    W2 = torch.tensor([[1.0, 2.0], [0.0, 0.0]], device=DEV)
    m.weighted_merge(base + 1, deltas, W2, offs32, out)
    assert out[:1000].eq(1).all() and out[1000:].eq(2).all()
    gw = m.grad_merge_weights(g, base + 1, deltas, base, offs32)
    assert gw.tolist() == [[1000.0, 24.0], [1000.0, 24.0]]

    def bad(fn, *a):
        with pytest.raises(RuntimeError):
            fn(*a)

    wm, gm = m.weighted_merge, m.grad_merge_weights
    bad(wm, base, deltas, torch.ones(1, n, device=DEV), offs, out)   # W^T
    bad(wm, base, deltas, W[:1], offs, out)             # W rows != models
    S = 1024                                    # [32, 1024] W: 128 KB of LDS
    bad(wm, base, torch.zeros(32, P, device=DEV), torch.ones(32, S, device=DEV),
        torch.arange(S + 1, device=DEV), out)
    bad(wm, base, torch.zeros(33, P, device=DEV), torch.ones(33, 1, device=DEV),
        offs, out)                              # more models than MAX_MODELS
    bad(wm, base, deltas[:, :1000].contiguous(), W, offs, out)  # not [N, P]
    bad(wm, base, deltas.view(-1), W, offs, out)
    bad(wm, base, deltas, W, offs, out[:1000])          # out of another size
    bad(wm, base.bfloat16(), deltas, W, offs, out)
    bad(wm, base, deltas, W, offs.float(), out)         # float offsets
    bad(wm, base, deltas, W, offs.view(1, 2), out)
    bad(gm, g, base, deltas, base[:1000].contiguous(), offs)    # merged short
    bad(gm, g, base, deltas, base.bfloat16(), offs)
    bad(gm, g, base.bfloat16(), deltas, base, offs)
    bad(gm, g[:1000].contiguous(), base, deltas, base, offs)    # g short
    bad(gm, g.double(), base, deltas, base, offs)
    bad(gm, g, base, deltas[:, :1000].contiguous(), base, offs)
    bad(gm, g, base, deltas, base, offs.float())
    bad(gm, g, base, deltas, base, torch.tensor([0, P + 1], device=DEV))
    bad(gm, g, base, deltas, base, torch.tensor([0, 600, 500, P], device=DEV))


# ---------------------------------------------------------------------------
# ce_chunk + ce_finalize, the pipelined head's online softmax, driven
# directly over column tiles
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["fresh", "view"])
@pytest.mark.parametrize("case", N.CE_TILE_CASES, ids=str)
def test_ce_chunk_finalize_accuracy(case, how):
    """fresh: every tile a contiguous tensor of its own, as _LMHeadCEFn
    allocates them (leading dimension = tile width, odd where that is odd:
    rows 2 B aligned under the 16 B loads). view: a column view of the full
    logits (leading dimension V, v0 no multiple of 8)."""
    m = _ext()
    rows, vocab, _regime, tiles, _peak = case
    c = N.ce_tile_case(case)
    x, tg = c["x"].to(DEV), c["tg"].to(DEV)
    mr = torch.full((rows,), float("-inf"), device=DEV)
    sr = torch.zeros(rows, device=DEV)
    tl = torch.zeros(rows, device=DEV)
    v0 = 0
    for wd in tiles:
        tile = x[:, v0:v0 + wd]
        if how == "fresh":
            tile = tile.contiguous()
        assert tile.stride() == ((wd if how == "fresh" else vocab), 1)
        m.ce_chunk(tile, tg, v0, tl, mr, sr)
        v0 += wd
    loss_sum, lse, count = m.ce_finalize(tg, mr, sr, tl, -100)
    ex, rd = c["exact"], c["rounded"]
    name = f"{case[:3]}/{'+'.join(map(str, tiles))}/{case[4]}/{how}"
    fails = []
    for a, kw in (
            (("lse", lse, ex["lse"], rd["lse"]), {}),
            (("loss_sum", loss_sum.reshape(1), ex["loss_sum"].reshape(1),
              rd["loss_sum"].reshape(1)),
             dict(ulp_of=ex["lse"][c["tg"] != -100]))):
        try:
            N.check("ce_chunk", name, *a, row_dim=None, fp32_out=True, **kw)
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)
    assert int(count) == ex["count"]
    # the recorded target logit is the bf16 input, bit for bit; ignored rows
    # keep their initial 0
    valid = c["tg"] != -100
    want = torch.zeros(rows)
    want[valid] = c["x"].float()[valid].gather(
        1, c["tg"][valid][:, None])[:, 0]
    assert torch.equal(tl.cpu(), want)


# ---------------------------------------------------------------------------
# KV-cache append at a device position
# ---------------------------------------------------------------------------
def _sentinel(shape, add):
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n) % 251) + add).to(torch.bfloat16).view(shape)


# (B, H, Hk, Lmax, D); the last has B Hk D > 1024 x 256: the capped grid loops
@pytest.mark.parametrize("shape", [(2, 4, 2, 5, 64), (3, 2, 2, 4, 128),
                                   (33, 64, 64, 2, 128)], ids=str)
def test_kv_append_and_i32_inc(shape):
    """k / v as strided slices of one packed projection into sentinel-filled
    caches at device row 0, a middle row and Lmax - 1: exactly the addressed
    rows change and equal the source; after i32_inc the next append lands
    one row on."""
    m = _ext()
    B, H, Hk, Lmax, D = shape
    E, kvd = H * D, Hk * D

    def proj(seed):
        p = N.randn_bf16(B, 1, E + 2 * kvd, seed=seed).to(DEV)
        k, v = p[..., E:E + kvd], p[..., E + kvd:]
        assert k.stride(0) == E + 2 * kvd
        return k, v

    k0, v0 = proj(30)
    k1, v1 = proj(31)
    sk, sv = _sentinel((B, Hk, Lmax, D), 0), _sentinel((B, Hk, Lmax, D), 300)
    for p0 in sorted({0, Lmax // 2, Lmax - 1}):
        kc, vc = sk.to(DEV), sv.to(DEV)
        pos = _i32(p0)
        m.kv_append(k0, v0, kc, vc, pos)
        want_k, want_v = sk.clone(), sv.clone()
        want_k[:, :, p0] = k0.cpu().reshape(B, Hk, D)
        want_v[:, :, p0] = v0.cpu().reshape(B, Hk, D)
        assert int(pos) == p0
        assert torch.equal(kc.cpu(), want_k) and torch.equal(vc.cpu(), want_v)
        m.i32_inc(pos)
        assert int(pos) == p0 + 1
        if p0 + 1 < Lmax:
            m.kv_append(k1, v1, kc, vc, pos)
            want_k[:, :, p0 + 1] = k1.cpu().reshape(B, Hk, D)
            want_v[:, :, p0 + 1] = v1.cpu().reshape(B, Hk, D)
            assert torch.equal(kc.cpu(), want_k)
            assert torch.equal(vc.cpu(), want_v)


def test_kv_append_rejects_bad_caches():
    m = _ext()
    B, Hk, Lmax, D = 2, 2, 4, 64
    p = torch.zeros(B, 1, 4 * Hk * D, dtype=torch.bfloat16, device=DEV)
    k, v = p[..., :Hk * D], p[..., Hk * D:2 * Hk * D]
    kc = torch.zeros(B, Hk, Lmax, D, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    pos = _i32(1)
    m.kv_append(k, v, kc, vc, pos)
    wide = torch.zeros(B, Hk, 2 * Lmax, D, dtype=torch.bfloat16, device=DEV)
    for bad_k, bad_v in ((kc.float(), vc.float()),          # not bf16
                         (kc, vc.float()),
                         (wide[:, :, ::2], wide[:, :, ::2]),   # row stride 2D
                         (kc.transpose(2, 3), vc.transpose(2, 3)),
                         (kc, torch.zeros_like(wide)),          # other shape
                         (kc[:1], vc[:1])):                     # other batch
        with pytest.raises(RuntimeError):
            m.kv_append(k, v, bad_k, bad_v, pos)
    with pytest.raises(RuntimeError):       # rows of another width
        m.kv_append(p[..., :D], p[..., D:2 * D], kc, vc, pos)


@pytest.mark.parametrize("n", [3, 4099, (1 << 21) + 3])
def test_has_nan_tail_and_last_vector(n):
    """The NaN in the scalar tail (n is no multiple of the 4-wide vector),
    then in the last full vector, then nowhere."""
    m = _ext()
    x = torch.randn(n, generator=torch.Generator().manual_seed(25)).to(DEV)
    assert not m.has_nan(x)
    tail = x.clone()
    tail[n - 1] = float("nan")
    assert m.has_nan(tail)
    if n >= 8:
        last_vec = x.clone()
        last_vec[(n // 4) * 4 - 1] = float("nan")
        assert m.has_nan(last_vec)
        first = x.clone()
        first[0] = float("nan")
        assert m.has_nan(first)
    inf = x.clone()
    inf[n - 1] = float("inf")
    assert not m.has_nan(inf)
