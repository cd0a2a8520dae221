"""The accuracy bound of tests/test_wgrad_gpu.py, checked on the CPU before
any GPU run: on the very inputs of the GPU cases the rounded reference passes
and every mistake the weight-gradient kernel (hip/wgrad.hip) can make fails.
Each wrong result is built from the fp64 reference and rounded as the kernel
rounds (once, to bf16)."""

import pytest
import torch

import _numerics as N
import _wgrad_cases as W


def _ids(crs):
    return [W.case_id(cr) for cr in crs]


def _passes(c, got, which="dw"):
    return N.passes(got[which], c["exact"][which], c["rounded"][which],
                    row_dim=-1 if which == "dw" else None)


def _mutant(c, **mut):
    m = W.reference(c["dy"], c["x"], c["dst_w"], c["dst_b"], mut)
    return dict(dw=N.bf16(m["dw"]), db=N.bf16(m["db"]))


@pytest.mark.parametrize("cr", W.CASE_REGIMES, ids=_ids(W.CASE_REGIMES))
def test_reference_passes(cr):
    c = W.case(*cr)
    assert _passes(c, c["rounded"], "dw")
    assert _passes(c, c["rounded"], "db")
    # the fp32 store against its fp32-torch baseline
    assert N.passes(c["db32_rounded"], c["db32_exact"], c["db32_rounded"],
                    row_dim=None, fp32_out=True)


@pytest.mark.parametrize("cr", W.CASE_REGIMES, ids=_ids(W.CASE_REGIMES))
def test_last_row_dropped(cr):
    c = W.case(*cr)
    m = _mutant(c, drop_last_row=True)
    assert not _passes(c, m, "dw")
    assert not _passes(c, m, "db")
    db32 = N.colsum(N.d(c["dy"])[:-1], mode="rounded")
    assert not N.passes(db32, c["db32_exact"], c["db32_rounded"],
                        row_dim=None, fp32_out=True)


@pytest.mark.parametrize("cr", W.CASE_REGIMES, ids=_ids(W.CASE_REGIMES))
def test_dst_overwritten(cr):
    c = W.case(*cr)
    m = _mutant(c, overwrite=True)
    assert not _passes(c, m, "dw")
    assert not _passes(c, m, "db")


SPLIT = [cr for cr in W.CASE_REGIMES if W.CASES[cr[0]]["ns"] > 1]


@pytest.mark.parametrize("cr", SPLIT, ids=_ids(SPLIT))
def test_one_slice_dropped(cr):
    """Every non-empty slice in turn."""
    c = W.case(*cr)
    T, ns = c["c"]["T"], c["c"]["ns"]
    seen = 0
    for s in range(ns):
        lo, hi = W.slice_rows(T, ns, s)
        if hi == lo:
            continue
        seen += 1
        m = _mutant(c, drop_slice=(lo, hi))
        assert not _passes(c, m, "dw"), s
        assert not _passes(c, m, "db"), s
    assert seen >= 1
    assert W.slice_rows(T, ns, ns - 1)[1] == T


RAGGED = [cr for cr in W.CASE_REGIMES if W.CASES[cr[0]]["T"] % W.BK]


@pytest.mark.parametrize("cr", RAGGED, ids=_ids(RAGGED))
def test_ragged_tail_read_as_garbage(cr):
    """The padding rows of the last K-step hold values of the inputs' own
    size instead of zeros."""
    c = W.case(*cr)
    T, out, inp = c["c"]["T"], c["c"]["out"], c["c"]["inp"]
    pad = W.BK - T % W.BK
    g = (N.randn_bf16(pad, out, seed=77, scale=0.05),
         N.randn_bf16(pad, inp, seed=78, scale=0.5))
    m = _mutant(c, garbage_tail=g)
    assert not _passes(c, m, "dw")
    assert not _passes(c, m, "db")


TWO_TILES = [cr for cr in W.CASE_REGIMES
             if W.CASES[cr[0]]["out"] > W.BM and W.CASES[cr[0]]["bias"] != "none"]


@pytest.mark.parametrize("cr", TWO_TILES, ids=_ids(TWO_TILES))
def test_bias_from_neighbouring_tile(cr):
    c = W.case(*cr)
    m = _mutant(c, bias_next_tile=True)
    assert _passes(c, m, "dw")          # dW is untouched by this mistake
    assert not _passes(c, m, "db")


def test_case_list_covers_the_issue():
    ts = {(c["T"], c["ns"]) for c in W.CASES}
    assert {(W.BK - 1, 1), (2 * W.BK + 5, 1), (1, 1), (6 * W.BK + 17, 3),
            (W.BK, 4)} <= ts
    assert {(c["out"], c["inp"]) for c in W.CASES} == {
        (2 * W.BM, W.BN), (W.BM, 3 * W.BN)}
    assert {c["bias"] for c in W.CASES} == {"dst", "f32", "none"}
    assert {c["off"] for c in W.CASES} == {0, 1}
    assert any(c["pad"] for c in W.CASES)
    # the cancel regime does cancel: the halves are ~50 x the result
    c = W.case(3, "cancel")
    h = c["c"]["T"] // 2
    half = (N.d(c["dy"])[:h].t() @ N.d(c["x"])[:h]).norm()
    full = (c["exact"]["dw"] - N.d(c["dst_w"])).norm()
    assert 20 * float(full) < float(half)


# ---------------------------------------------------------------------------
# routing gate (ops._wgrad_accum), with a stub in place of the extension
# ---------------------------------------------------------------------------
class _StubWgrad:
    def __init__(self, supported=True):
        self.calls, self.ok = [], supported

    def supported(self, dy, x):
        return self.ok

    def bias(self, dy, x, dw, db, bias_f32):
        self.calls.append((tuple(dy.shape), tuple(x.shape), db is not None,
                           bias_f32))
        return torch.zeros(dy.shape[1]) if bias_f32 else None


class _StubExt:
    def __init__(self, supported=True):
        self.wgrad = _StubWgrad(supported)


def _gate(mode, T, out, inp, *, wgrad=True, bgrad=True, want_bias=True,
          supported=True, dtype=torch.bfloat16):
    from distributedtraining_amd import ops
    m = _StubExt(supported)
    # meta tensors: the gate looks at shapes and dtypes only
    dy = torch.empty(T, out, dtype=dtype, device="meta")
    x = torch.empty(T, inp, dtype=dtype, device="meta")
    dw = torch.empty(out, inp, dtype=dtype, device="meta") if wgrad else None
    db = torch.empty(out, dtype=dtype, device="meta") if bgrad else None
    was = ops.wgrad_route(mode)
    try:
        done, db32 = ops._wgrad_accum(m, dy, x, dw, db, want_bias)
    finally:
        ops.wgrad_route(was)
    return done, db32, m.wgrad.calls


FLAGSHIP = [(T, o, i) for T in (65536, 32768)
            for o, i in ((2304, 768), (768, 768), (3072, 768), (768, 3072))]


def test_wins_table_is_the_measured_shapes():
    from distributedtraining_amd import ops
    assert set(ops._WGRAD_WINS) == set(FLAGSHIP)
    for s in FLAGSHIP:
        assert ops._wgrad_wins(*s)
    # in the tile contract but never measured: the library keeps them
    for s in ((65536, 768, 2304), (16384, 768, 768), (65536, 1024, 1024),
              (300, 512, 512), (65536, 50257, 768)):
        assert not ops._wgrad_wins(*s)


def test_auto_routes_listed_shapes_only():
    for s in FLAGSHIP:
        done, db32, calls = _gate("auto", *s)
        assert done and db32 is None
        assert calls == [((s[0], s[1]), (s[0], s[2]), True, False)]
    done, _, calls = _gate("auto", 300, 512, 512)
    assert not done and not calls
    done, _, calls = _gate("auto", 65536, 768, 2304)
    assert not done and not calls


def test_forced_and_off_routes():
    done, _, calls = _gate("1", 300, 512, 512)
    assert done and len(calls) == 1
    for s in FLAGSHIP[:1] + [(300, 512, 512)]:
        done, _, calls = _gate("0", *s)
        assert not done and not calls
    # outside the binding's contract: the library, in either mode
    for mode in ("1", "auto"):
        done, _, calls = _gate(mode, *FLAGSHIP[0], supported=False)
        assert not done and not calls
    # no flat-plane view, or not bf16: the library
    assert not _gate("1", *FLAGSHIP[0], wgrad=False)[0]
    assert not _gate("1", *FLAGSHIP[0], dtype=torch.float32)[0]


def test_bias_delivery_of_the_gate():
    s = FLAGSHIP[0]
    # bias wanted, no view: the fp32 sum comes back
    done, db32, calls = _gate("auto", *s, bgrad=False)
    assert done and db32 is not None and calls[0][2:] == (False, True)
    # no bias wanted (the fc weight): the no-bias kernel, a view is ignored
    done, db32, calls = _gate("auto", *s, want_bias=False)
    assert done and db32 is None and calls[0][2:] == (False, False)


def test_route_switch_rejects_other_values():
    from distributedtraining_amd import ops
    was = ops.wgrad_route("auto")
    try:
        assert ops.wgrad_route("0") == "auto"
        with pytest.raises(ValueError):
            ops.wgrad_route("yes")
        assert ops.wgrad_route("auto") == "0"
    finally:
        ops.wgrad_route(was)
