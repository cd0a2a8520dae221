"""The accuracy measure of tests/_numerics.py, checked on the CPU before it
is trusted on a kernel: on the shapes and input regimes of
tests/test_kernel_accuracy_gpu.py every ``rounded`` reference passes its own
bounds (the bounds are feasible), and every mutant -- a subtly wrong result
built from the ``exact`` reference alone -- is rejected on at least one
asserted tensor.

A mutant that perturbs ONE probability (a zeroed probability, a flipped
dropout draw, a kvlen off by one) can only be seen where that probability
matters at bf16 precision. It moves one row of ``o`` by p * |v_k|; rejection
is REQUIRED wherever that exceeds the bound of the row, and such cases must
exist in the regimes named below. Elsewhere (a peaked or saturated softmax
that puts 1e-4 on the key) the mutant equals the exact result to within the
bf16 floor, and nothing is asserted.
"""

import math

import pytest
import torch

import _numerics as N


def _rejected(got, exact, rounded, tensors):
    """Names of the (name, row_dim, live, fp32[, ulp_of]) tensors that reject
    ``got``."""
    return [name for name, *spec in tensors
            if got[name] is not None and not N.passes(
                got[name], exact[name], rounded[name], *spec)]


def _feasible(exact, rounded, tensors):
    for name, *spec in tensors:
        if exact[name] is None:
            continue
        base, bound = N.bounds(exact[name], rounded[name], *spec)
        assert all(math.isfinite(b) for b in base + bound), (name, base)
        assert N.passes(rounded[name], exact[name], rounded[name],
                        *spec), name


# ---------------------------------------------------------------------------
# The measure itself
# ---------------------------------------------------------------------------
def test_errors_definition():
    exact = torch.tensor([[3.0, 4.0], [0.0, 0.0], [6.0, 8.0]], dtype=N.F64)
    got = exact.clone()
    got[1, 0] = 0.5          # error on the exactly-zero row
    got[2, 1] = 9.0
    rel, worst = N.errors(got, exact)
    norms = torch.tensor([5.0, 0.0, 10.0])
    rms = float(norms.pow(2).mean().sqrt())
    assert rel == pytest.approx(math.sqrt(0.25 + 1.0) / float(norms.norm()))
    # the zero row is judged against the rms row norm, not left out
    assert worst == pytest.approx(max(0.5 / rms, 1.0 / 10.0))
    # every element its own row
    rel1, worst1 = N.errors(got, exact, row_dim=None)
    assert rel1 == pytest.approx(rel)
    assert worst1 == pytest.approx(1.0 / 8.0)
    # rows outside the contract are the only thing left out
    live = torch.tensor([True, False, True])
    assert N.errors(got, exact, live=live)[1] == pytest.approx(0.1)
    # non-finite output is infinitely wrong
    got[0, 0] = float("nan")
    assert N.errors(got, exact) == (float("inf"), float("inf"))


def test_fp32_bound_has_ulp_floor():
    exact = torch.tensor([1.0, 100.0], dtype=N.F64)
    # a perfect baseline still leaves room for 4 fp32 ulp
    _, bound = N.bounds(exact, exact, row_dim=None, fp32_out=True)
    assert bound[0] > 0 and bound[1] > 0
    ulp = torch.tensor([2.0 ** -23, 2.0 ** -17], dtype=N.F64)
    assert N.passes(exact + 3 * ulp, exact, exact, None, None, True)
    assert not N.passes(exact + 6 * ulp, exact, exact, None, None, True)
    # and a bf16 quantity gets no floor at all
    assert not N.passes(exact + ulp, exact, exact, None, None, False)


# ---------------------------------------------------------------------------
# Attention
# ---------------------------------------------------------------------------
def _attn_tensors(c):
    return [(n, -1, N.attn_live(c, n), False) for n in N.ATTN_TENSORS]


def _attn_mut(c, **kw):
    q, k, v, do, scale, kvlen, keep, inv = c["args"]
    a = dict(scale=scale, kvlen=kvlen, keep=keep, mut=None)
    a.update(kw)
    return N.attention(q, k, v, do, a["scale"], a["kvlen"], a["keep"], inv,
                       mut=a["mut"])


def _full_row(case):
    """(b, rows) of the batch row with the most visible keys."""
    (B, _H, _Hk, S, _D), _r, kv, _p = case
    if kv is None:
        return 0, S
    b = max(range(B), key=lambda i: min(kv[i], S))
    return b, min(kv[b], S)


def _row_harm_exceeds_bound(c, b, h, qrow, key, mass):
    """Does moving probability ``mass`` of key ``key`` in or out of row
    (b, h, qrow) of o exceed that row's worst_row bound?"""
    o = c["exact"]["o"]
    _, bound = N.bounds(o, c["rounded"]["o"], -1, c["live"])
    norms = o.norm(dim=-1)[c["live"]]
    rms = float(norms.pow(2).mean().sqrt())
    v = c["args"][2]
    hk = h // (o.shape[1] // v.shape[1])
    harm = mass * float(v[b, hk, key].norm())
    return harm > bound[1] * max(float(o[b, h, qrow].norm()), rms)


@pytest.mark.parametrize("case", N.ATTN_CASES, ids=N.case_id)
def test_attention_rounded_is_feasible(case):
    c = N.attn_case(case)
    _feasible(c["exact"], c["rounded"], _attn_tensors(c))


@pytest.mark.parametrize("case", N.ATTN_CASES, ids=N.case_id)
def test_attention_mutant_scale(case):
    """scale x 1.03. A softmax over one key does not depend on the scale,
    and neither does one that is saturated in every row (S = 17, large):
    there the mutant IS the exact result."""
    c = N.attn_case(case)
    q, k, _v, _do, scale, kvlen, _keep, _inv = c["args"]
    A = N.attention_probs(q, k, scale, kvlen)
    unsaturated = float((1.0 - A.amax(-1))[c["live"]].max())
    rej = _rejected(_attn_mut(c, scale=scale * 1.03), c["exact"],
                    c["rounded"], _attn_tensors(c))
    if unsaturated < 1e-3:
        assert case[0][3] in (1, 17) and (case[0][3] == 1
                                          or case[1] == "large")
        return
    assert rej, "scale x 1.03 passed every tensor"


def test_attention_mutant_one_probability():
    """One probability zeroed at (last row, second-to-last key) of head 0,
    and with dropout the draw of that element flipped."""
    required = {"zero": [], "flip": []}
    for case in N.ATTN_CASES:
        c = N.attn_case(case)
        b, rows = _full_row(case)
        if rows < 2:
            continue
        q, k, _v, _do, scale, kvlen, keep, inv = c["args"]
        pos = (b, 0, rows - 1, rows - 2)
        P = float(N.attention_probs(q, k, scale, kvlen)[pos])
        kept = keep is None or bool(keep[pos])
        tensors = _attn_tensors(c)
        if kept and _row_harm_exceeds_bound(c, b, 0, rows - 1, rows - 2,
                                            P * inv):
            assert _rejected(_attn_mut(c, mut=dict(zero_prob=pos)),
                             c["exact"], c["rounded"], tensors), case
            required["zero"].append(case)
        if keep is not None and _row_harm_exceeds_bound(
                c, b, 0, rows - 1, rows - 2, P * inv):
            k2 = keep.clone()
            k2[pos] = ~k2[pos]
            assert _rejected(_attn_mut(c, keep=k2), c["exact"], c["rounded"],
                             tensors), case
            required["flip"].append(case)
    # the motivating cases are among those where rejection was required
    fused = (2, 2, 2, 64, 64)
    assert (fused, "diffuse", None, 0.0) in required["zero"]
    assert ((1, 2, 2, 70, 32), "diffuse", None, 0.0) in required["zero"]
    assert (fused, "diffuse", None, 0.1) in required["flip"]
    assert (fused, "diffuse", (64, 17), 0.25) in required["flip"]
    assert ((1, 2, 2, 70, 32), "diffuse", None, 0.25) in required["flip"]
    assert len(required["zero"]) >= 8 and len(required["flip"]) >= 4


@pytest.mark.parametrize("case", N.ATTN_DROP, ids=N.case_id)
def test_attention_mutant_dv_without_inv_keep(case):
    c = N.attn_case(case)
    rej = _rejected(_attn_mut(c, mut=dict(dv_no_inv_keep=True)), c["exact"],
                    c["rounded"], _attn_tensors(c))
    assert rej == ["dv"]


def test_attention_mutant_kvlen_off_by_one():
    """kvlen - 1: row kvlen - 1 loses its diagonal key. Required wherever
    some head gives that key a mass above the row's bound."""
    n_required = 0
    cases = [c for c in N.ATTN_CASES if c[2] is not None]
    for case in cases:
        c = N.attn_case(case)
        (B, H, _Hk, S, _D) = case[0]
        q, k, _v, _do, scale, kvlen, _keep, inv = c["args"]
        A = N.attention_probs(q, k, scale, kvlen)
        kk = kvlen.clamp(max=S)
        need = any(_row_harm_exceeds_bound(
            c, b, h, int(kk[b]) - 1, int(kk[b]) - 1,
            float(A[b, h, kk[b] - 1, kk[b] - 1]))
            for b in range(B) for h in range(H) if kk[b] > 1
            and (c["keep"] is None
                 or bool(c["keep"][b, h, kk[b] - 1, kk[b] - 1])))
        if need:
            rej = _rejected(_attn_mut(c, kvlen=(kk - 1).clamp(min=1)),
                            c["exact"], c["rounded"], _attn_tensors(c))
            assert rej, case
            n_required += 1
    assert n_required >= len(cases) - 2


@pytest.mark.parametrize("case", [c for c in N.ATTN_CASES
                                  if c[0][1] != c[0][2]], ids=N.case_id)
def test_attention_mutant_gqa_wrong_head(case):
    c = N.attn_case(case)
    rej = _rejected(_attn_mut(c, mut=dict(gqa_mod=True)), c["exact"],
                    c["rounded"], _attn_tensors(c))
    assert set(rej) == set(N.ATTN_TENSORS)


@pytest.mark.parametrize("case", N.DECODE_CASES, ids=str)
def test_decode_rounded_is_feasible_and_rejects_scale(case):
    c = N.decode_case(case)
    t = [("o", -1, None, False)]
    _feasible(dict(o=c["exact"]), dict(o=c["rounded"]), t)
    if case[3] == 1:
        return          # one key: the scale drops out
    mut = N.decode_attention(N.d(c["q"]), N.d(c["kc"]), N.d(c["vc"]),
                             case[3], c["scale"] * 1.03)
    assert not N.passes(mut, c["exact"], c["rounded"])


# ---------------------------------------------------------------------------
# Cross entropy
# ---------------------------------------------------------------------------
def _ce_views(c, out):
    """The asserted CE quantities as a dict of tensors."""
    return dict(lse=out["lse"], loss_sum=out["loss_sum"].reshape(1),
                dlogits=out["dlogits"],
                dtarget=N.ce_target_entries(out["dlogits"], c["tg"]))


def _ce_tensors(c):
    return [("lse", None, None, True),
            ("loss_sum", None, None, True, N.ce_valid_lse(c)),
            ("dlogits", -1, None, False), ("dtarget", None, None, False)]


@pytest.mark.parametrize("case", N.CE_CASES, ids=str)
def test_ce_rounded_feasible_and_mutants_rejected(case):
    c = N.ce_case(case)
    exact, rounded = _ce_views(c, c["exact"]), _ce_views(c, c["rounded"])
    CE_TENSORS = _ce_tensors(c)
    _feasible(exact, rounded, CE_TENSORS)
    assert c["exact"]["count"] == c["rounded"]["count"] == c["n_valid"]

    def mutant(**mut):
        return _ce_views(c, N.cross_entropy(*c["args"], mut=mut))

    rej = _rejected(mutant(grad_mul=1.04), exact, rounded, CE_TENSORS)
    assert "dlogits" in rej and "dtarget" in rej
    rej = _rejected(mutant(lse_add=0.05), exact, rounded, CE_TENSORS)
    assert "lse" in rej and "loss_sum" in rej
    assert "dlogits" in _rejected(mutant(grad_ignored=True), exact, rounded,
                                  CE_TENSORS)
    assert _rejected(mutant(count_all=True), exact, rounded, CE_TENSORS)


def test_head_loss_rounded_feasible():
    c = N.head_loss_case()
    t = [("lse", None, None, True),
         ("loss_sum", None, None, True, N.ce_valid_lse(c))]
    ex = dict(lse=c["exact"]["lse"],
              loss_sum=c["exact"]["loss_sum"].reshape(1))
    rd = dict(lse=c["rounded"]["lse"],
              loss_sum=c["rounded"]["loss_sum"].reshape(1))
    _feasible(ex, rd, t)
    mut = dict(lse=ex["lse"] + 0.05, loss_sum=ex["loss_sum"] * 1.0001)
    assert _rejected(mut, ex, rd, t) == ["lse", "loss_sum"]


# ---------------------------------------------------------------------------
# Norms
# ---------------------------------------------------------------------------
def _norm_t(case):
    return [(n, rd, None, False) for n, rd in N.norm_tensors(case)]


@pytest.mark.parametrize("case", N.NORM_CASES, ids=str)
def test_norm_rounded_feasible_and_mutants_rejected(case):
    c = N.norm_case(case)
    t = _norm_t(case)
    _feasible(c["exact"], c["rounded"], t)
    rej = _rejected(N.norm(**c["kw"], mut=dict(no_mean_term=True)),
                    c["exact"], c["rounded"], t)
    if case[3:] == ("offset100", "residual"):
        # the one regime that hides it: dx = ds + the norm's gradient, and
        # at x = 100 + noise that gradient is 1/100 of ds for RMSNorm
        # (rstd = 0.01) and for LayerNorm made of an xhat that the bf16 sum
        # has already lost (baseline 2e-2). Nothing is asserted here; the
        # plain form at the same inputs sees it.
        pass
    else:
        assert "dx" in rej
    rej = _rejected(N.norm(**c["kw"], mut=dict(dw_skip_last_row=True)),
                    c["exact"], c["rounded"], t)
    if case[2:] == ("layer", "offset100", "residual"):
        # the bf16 sum of 100 + noise keeps one step of 0.5 of the noise:
        # xhat, and with it dw, is already 25% off in the rounded reference,
        # and the missing row shows in db (which has no xhat in it) alone
        assert rej == ["db"]
    else:
        assert "dw" in rej
    if case[3] == "lowvar" and case[4] == "plain":
        # eps omitted: seen on the row whose variance is of the size of eps
        rej = _rejected(N.norm(**c["kw"], mut=dict(no_eps=True)),
                        c["exact"], c["rounded"], t)
        assert "y" in rej and "dx" in rej


# ---------------------------------------------------------------------------
# GELU / SwiGLU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.EW_CASES, ids=str)
def test_elementwise_rounded_feasible(case):
    c = N.ew_case(case)
    for op, names in (("gelu", ("y", "dx")),
                      ("swiglu", ("y", "dgate", "dup"))):
        for label, sl in N.ew_parts(case):
            ex = {n: c[f"{op}_exact"][n][sl] for n in names}
            rd = {n: c[f"{op}_rounded"][n][sl] for n in names}
            _feasible(ex, rd, [(n, None, None, False) for n in names])


def test_gelu_mutant_erf_form():
    """The erf form differs from the tanh form by at most 5e-4 absolute:
    inside the bf16 floor wherever GELU is of order one, and 3% to 40% of
    the value in the negative tail. The tail regime is there to see it."""
    c = N.ew_case((4099, "tail"))
    x, dy = N.d(c["x"]), N.d(c["dy"])
    mut = N.gelu(x, dy, mut=dict(erf=True))
    t = [("y", None, None, False), ("dx", None, None, False)]
    assert _rejected(mut, c["gelu_exact"], c["gelu_rounded"], t) == ["y", "dx"]


# ---------------------------------------------------------------------------
# RoPE, embedding, AdamW, flat plane
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.ROPE_CASES, ids=str)
def test_rope_rounded_feasible_and_mutants_rejected(case):
    c = N.rope_case(case)
    _bh, _S, _D, pos = case
    x, cos, sin = N.d(c["x"]), N.d(c["cos"]), N.d(c["sin"])
    for name in ("fwd", "bwd"):
        _feasible(dict(y=c[f"{name}_exact"]), dict(y=c[f"{name}_rounded"]),
                  [("y", -1, None, False)])
    # the backward with the forward's sign. Position 0 is the identity
    # rotation either way, so a case holding only that row cannot see it.
    if not (case[1] == 1 and pos == 0):
        mut = N.rope(x, cos, sin, pos, True, mut=dict(bwd_fwd_sign=True))
        assert not N.passes(mut, c["bwd_exact"], c["bwd_rounded"])
    if pos:
        for name, bwd in (("fwd", False), ("bwd", True)):
            mut = N.rope(x, cos, sin, pos, bwd, mut=dict(row_off=1))
            assert not N.passes(mut, c[f"{name}_exact"],
                                c[f"{name}_rounded"])
            mut = N.rope(x, cos, sin, 0, bwd)      # offset ignored
            assert not N.passes(mut, c[f"{name}_exact"],
                                c[f"{name}_rounded"])


EMB_TENSORS = [("y", -1, None, False), ("dwte", -1, None, True),
               ("dwpe", -1, None, True)]


@pytest.mark.parametrize("case", N.EMB_CASES, ids=str)
def test_embedding_rounded_feasible_and_mutants_rejected(case):
    c = N.emb_case(case)
    _feasible(c["exact"], c["rounded"], EMB_TENSORS)
    pos = case[-1]
    ids, wte, wpe, dy = c["ids"], N.d(c["wte"]), N.d(c["wpe"]), N.d(c["dy"])
    # position row off by one; one token's gradient dropped
    mut = N.embedding(ids, wte, wpe, dy, pos + 1)
    assert "y" in _rejected(mut, c["exact"], c["rounded"], EMB_TENSORS)
    dy2 = dy.clone()
    dy2[0, 0] = 0
    mut = N.embedding(ids, wte, wpe, dy2, pos)
    rej = _rejected(mut, c["exact"], c["rounded"], EMB_TENSORS)
    assert "dwte" in rej and "dwpe" in rej


def _adamw_t():
    return [(n, None, None, fp32) for n, fp32 in N.ADAMW_TENSORS]


def test_adamw_rounded_feasible_and_mutants_rejected():
    c = N.adamw_case()
    _feasible(c["exact"], c["rounded"], _adamw_t())
    a = (N.d(c["master"]), [N.d(g) for g in c["grads"]])
    for mut in (dict(bc_prev_step=True), dict(coupled=True)):
        rej = _rejected(N.adamw(*a, **N.ADAMW_HP, mut=mut), c["exact"],
                        c["rounded"], _adamw_t())
        assert "master" in rej, (mut, rej)
    # the gradient in fp32 where the kernel reads its bf16 rounding: what
    # test_adamw_matches_cpu_reference used to allow
    g0 = torch.Generator().manual_seed(21)
    torch.randn(N.ADAMW_N, generator=g0)
    g32 = [N.d(torch.randn(N.ADAMW_N, generator=g0)) for _ in range(3)]
    rej = _rejected(N.adamw(a[0], g32, **N.ADAMW_HP), c["exact"],
                    c["rounded"], _adamw_t())
    assert "master" in rej and "m" in rej and "v" in rej


def test_flat_references_feasible():
    g = torch.Generator().manual_seed(22)
    x = N.d(torch.randn(100_003, generator=g))
    ex, rd = N.l2norm_sq(x).reshape(1), N.l2norm_sq(x, "rounded").reshape(1)
    assert N.passes(rd, ex, rd, None, None, True)
    assert not N.passes(ex * (1 + 1e-5), ex, rd, None, None, True)
    m = N.d(N.randn_bf16(333, 520, seed=23))
    ex, rd = N.colsum(m), N.colsum(m, "rounded")
    assert N.passes(rd, ex, rd, None, None, True)
    assert not N.passes(N.colsum(m[:-1]), ex, rd, None, None, True)
    w = N.d(torch.randn(4099, generator=g))
    y = N.d(torch.randn(4099, generator=g))
    ex, rd = N.axpy(w, y, -0.37), N.axpy(w, y, -0.37, "rounded")
    assert N.passes(rd, ex, rd, None, None, True)
    assert not N.passes(N.axpy(w, y, 1.0), ex, rd, None, None, True)


# ---------------------------------------------------------------------------
# Serving GEMV
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.GEMV_CASES, ids=str)
def test_gemv_rounded_feasible_and_mutants_rejected(case):
    """A mutant must be rejected wherever it changes the value, with these
    exceptions, each for the reason given.

    drop_last8, and drop_last_chunk where the last chunk IS those 8 elements
    (K = 4104 = KC + 8 or 2 KC + 8): 8 of K >= 4096 products are sqrt(8 / K)
    <= 4.4 % of the dot product's rms, one to two bf16 steps of the result;
    on the one or five numbers of such a row that is inside 3 x the floor as
    often as not. It is required up to K = 2056 and in the cancelling regime
    at every K, where each of the 8 products is 8 / (K / 2) x 50 of the
    result. Under a bias of 100 x the product nothing about 8 elements shows.

    bf16_between_chunks: one more bf16 rounding, of a partial sum no larger
    than the result, is below 3 x the floor in the randn regime. The
    cancelling regime is there for it: the partial at the chunk boundary is
    50 x the result at (1, 14336) and (4, 4104). At (2, 4104) and (3, 2056)
    the boundary falls 8 elements before the end, where the two halves have
    cancelled already.

    skip_last_col at (1, 2051, 64): one column in 2051 that happens to hold
    a value of a fifth of the rms; (4, 2051, 64) has four rows of it."""
    M, Ncol, K, bias, regime = case
    c = N.gemv_case(case)
    ex, rd = c["exact"], c["rounded"]
    assert N.passes(rd, ex, rd)

    def rejected(**mut):
        return not N.passes(N.gemv(*c["args"], mut=mut), ex, rd)

    last = K - ((K - 1) // N.gemv_kc(M)) * N.gemv_kc(M)
    eight = regime == "cancel" or (K <= 2056 and bias != "x100")
    if eight:
        assert rejected(drop_last8=True)
    if last > 8 or eight:
        assert rejected(drop_last_chunk=True)
    if bias != "none":
        assert rejected(no_bias=True)
    if case in ((1, 5, 14336, "none", "cancel"), (4, 5, 4104, "none", "cancel")):
        assert rejected(bf16_between_chunks=True)
    if M > 1:
        assert rejected(row_shift=True)
    if case != (1, 2051, 64, "bf16", "randn"):
        assert rejected(skip_last_col=True)


# ---------------------------------------------------------------------------
# Merge plane
# ---------------------------------------------------------------------------
_F32 = (None, None, True)       # row_dim, live, fp32_out of an fp32 plane


@pytest.mark.parametrize("case", N.MERGE_CASES, ids=str)
def test_weighted_merge_rounded_feasible_and_mutants_rejected(case):
    """Every mutant is rejected wherever it changes the value in exact
    arithmetic. It does not: a neighbouring segment's weight and W read as
    [seg, i] under uniform W, with one model, or with one segment; base
    added once where the columns of W sum to 1 (uniform, signed: the same
    number up to fp32 rounding)."""
    table, n, wkind = case
    c = N.merge_case(case)
    ex, rd = c["exact"], c["rounded"]
    assert N.passes(rd, ex, rd, *_F32)

    def rejected(**mut):
        return not N.passes(N.weighted_merge(*c["args"], mut=mut), ex, rd,
                            *_F32)

    assert rejected(drop_last_model=True)
    varied = wkind == "rand" or (wkind == "signed" and n > 1)
    segs = sum(1 for s in N.MERGE_TABLES[table] if s)
    if varied and segs > 1:
        assert rejected(boundary_prev_weight=True)
        if n > 1:
            assert rejected(w_transposed=True)
    if wkind == "rand":
        assert rejected(base_once=True)


def test_weighted_merge_loop_plane_feasible():
    mrb = N.max_resident_blocks()
    t = N.merge_case_uncached(N.merge_loop_table(mrb), 3, "rand")
    assert t["P"] > mrb * 256
    assert N.passes(t["rounded"], t["exact"], t["rounded"], *_F32)


def _np32(t):
    return N.d(t).to(torch.float32).numpy()


@pytest.mark.parametrize("case", N.GRADW_CASES, ids=str)
def test_grad_w_rounded_feasible_and_mutants_rejected(case):
    """The summand order grad_w_k had, (base + d) - merged, summed in the
    kernel's own lane order, is rejected in both cancelling regimes (it is
    the same number where W does not cancel). The other mutants are rejected
    wherever they change the value: next_seg does not with one segment."""
    table, _n, regime, gd = case
    c = N.gradw_case(case) if table != "big" else N.gradw_case_uncached(case)
    ex, rd = c["exact"], c["rounded"]
    assert N.passes(rd, ex, rd, *_F32)
    parent = torch.from_numpy(N.grad_w_fp32(
        _np32(c["g_in"]), _np32(c["base"]), _np32(c["deltas"]),
        _np32(c["merged"]), c["offsets"], order="parent")).to(N.F64)
    e_par, e_rd = N.errors(parent, ex, None), N.errors(rd, ex, None)
    print(f"[selfcheck] grad_W {case}: (base+d)-merged {e_par[0]:.2e}/"
          f"{e_par[1]:.2e}, (base-merged)+d {e_rd[0]:.2e}/{e_rd[1]:.2e}")
    if regime in ("d1e-3", "d1e-5"):
        assert not N.passes(parent, ex, rd, *_F32)
    else:
        assert N.passes(parent, ex, rd, *_F32)

    def rejected(**mut):
        return not N.passes(N.grad_merge_weights(*c["args"], mut=mut), ex,
                            rd, *_F32)

    assert rejected(no_merged=True)
    assert rejected(drop_seg_last=True)
    if len(N.MERGE_TABLES[table]) > 1:
        assert rejected(next_seg=True)
    if gd == "bf16":
        # bf16 g read as the fp32 plane it was rounded from
        a = (N.d(c["g_src"]),) + c["args"][1:]
        assert not N.passes(N.grad_merge_weights(*a), ex, rd, *_F32)


def test_lane_sum32_is_the_kernel_order():
    """256 strided serial fp32 chains, then a serial fold, on numbers where
    the order shows: 1 followed by 2^-24 s gives 1 in a chain of its own
    and more in any pairwise order."""
    import numpy as np
    t = np.zeros(512, np.float32)
    t[0] = 1.0
    t[256] = 2.0 ** -24          # same lane as t[0]: lost
    t[1], t[257] = 2.0 ** -24, 2.0 ** -24     # lane 1: kept, 2^-23
    assert float(N.lane_sum32(t)) == 1.0 + 2.0 ** -23
    assert float(N.lane_sum32(np.zeros(0, np.float32))) == 0.0


# ---------------------------------------------------------------------------
# ce_chunk + ce_finalize
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.CE_TILE_CASES, ids=str)
def test_ce_tiles_model_and_mutants(case):
    """The tile-by-tile model equals the one-shot reference, and its mutants
    are rejected, except: no_rescale with one tile, or where the maximum of
    every row arrives with the first tile (peak first at (5, 7); the other
    shapes have row 1's target, 30 above the rest, in a later tile);
    drop_tail where no tile has a tail (widths 640, 360, 1000), and at
    (8, 50257), whose tail is one column in 50257: 2e-5 of the row's sum,
    below the fp32 bound of an lse of 10 to 90."""
    rows, vocab, _regime, tiles, peak = case
    c = N.ce_tile_case(case)
    ex, rd = c["exact"], c["rounded"]
    x, tg = N.d(c["x"]), c["tg"]
    u = ex["lse"][tg != -100]
    got = N.ce_tiles(x, tg, tiles, -100)
    assert torch.allclose(got["lse"], ex["lse"], rtol=1e-12, atol=0)
    assert float(got["loss_sum"]) == pytest.approx(float(ex["loss_sum"]),
                                                   rel=1e-10)
    assert got["count"] == ex["count"]
    valid = tg != -100
    assert torch.equal(got["tlogit"][valid],
                       x[valid].gather(1, tg[valid][:, None])[:, 0])
    assert N.passes(rd["lse"], ex["lse"], rd["lse"], *_F32)
    assert N.passes(rd["loss_sum"].reshape(1), ex["loss_sum"].reshape(1),
                    rd["loss_sum"].reshape(1), None, None, True, u)

    def rej(**mut):
        g = N.ce_tiles(x, tg, tiles, -100, mut=mut)
        out = set()
        if not N.passes(g["lse"], ex["lse"], rd["lse"], *_F32):
            out.add("lse")
        if not N.passes(g["loss_sum"].reshape(1), ex["loss_sum"].reshape(1),
                        rd["loss_sum"].reshape(1), None, None, True, u):
            out.add("loss_sum")
        if g["count"] != ex["count"]:
            out.add("count")
        if not torch.equal(g["tlogit"], got["tlogit"]):
            out.add("tlogit")
        return out

    if len(tiles) > 1 and not (vocab == 7 and peak == "first"):
        assert "lse" in rej(no_rescale=True)
    assert {"loss_sum", "tlogit"} <= rej(v0_off=True)
    if any(w % 8 for w in tiles) and vocab != 50257:
        assert {"lse", "loss_sum"} <= rej(drop_tail=True)
    assert {"loss_sum", "count"} <= rej(count_ignored=True)


# ---------------------------------------------------------------------------
# Completeness: every export of the extension has an entry in N.EXPORTS
# ---------------------------------------------------------------------------
def test_every_export_has_a_reference():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hip = os.path.join(root, "distributedtraining_amd", "ops", "hip")
    names = []
    for src in ("bindings.cpp", "lt_fused.cpp"):
        with open(os.path.join(hip, src)) as f:
            names += re.findall(r'm\.def\(\s*"(\w+)"', f.read())
    assert len(names) > 50 and len(set(names)) == len(names)
    missing = [n for n in names if n not in N.EXPORTS]
    assert not missing, f"exports without an entry in _numerics.EXPORTS: " \
                        f"{missing}"
    stale = [n for n in N.EXPORTS if n not in names]
    assert not stale, f"entries of _numerics.EXPORTS that are no export: " \
                      f"{stale}"
    for name, where in N.EXPORTS.items():
        if where.startswith("tests/"):
            assert os.path.isfile(os.path.join(root, where)), (name, where)
        else:
            assert where.startswith("not numeric: "), (name, where)
