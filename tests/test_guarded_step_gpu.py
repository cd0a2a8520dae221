"""Guarded optimizer step on the GPU: the norm pass, step_ctl_k and the CTL
instantiation of adamw_k against the fp64 references, at the bounds of
tests/_numerics.py; bit-level checks of the skip and of a guard that never
fires; and a captured-graph replay with a moving lr.

The guarded-AdamW reference and its inputs come from
tests/test_guarded_step_cpu.py, whose self-check shows that these bounds
reject a kernel without clipping, with the clip factor missing from v, with
the lr of the previous step, or with t advanced on a skipped step.
"""

import os
import re

import numpy as np
import pytest
import torch

import _numerics as N
import test_guarded_step_cpu as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HP = N.ADAMW_HP


def _ops():
    from distributedtraining_amd import ops
    from distributedtraining_amd.ops.backend import require_ext
    require_ext()
    return ops


def _max_resident_blocks() -> int:
    from distributedtraining_amd import ops
    path = os.path.join(os.path.dirname(ops.__file__), "hip", "dta_common.h")
    with open(path) as f:
        mt = re.search(r"MAX_RESIDENT_BLOCKS\s*=\s*(\d+)", f.read())
    return int(mt.group(1))


def _ctl():
    return (torch.zeros(6, dtype=torch.float32, device=DEV),
            torch.zeros(4, dtype=torch.int32, device=DEV))


def _norm(ops, x, ctl_f, ctl_i, **kw):
    """Norm pass + control kernel on ``x``; returns the partials."""
    part = torch.full((ops.grad_sumsq_blocks(x.numel(), x.dtype, x.device),),
                      float("nan"), dtype=torch.float32, device=DEV)
    ops.grad_sumsq_partials(x, part)
    ops.step_control(part, ctl_f, ctl_i, HP["beta1"], HP["beta2"], **kw)
    return part


class _State:
    """master, m, v, work and a control block on the device, stepped through
    the three guarded ops."""

    def __init__(self, ops, master, **kw):
        self.ops, self.kw = ops, kw
        self.master = master.to(DEV).clone()
        self.m = torch.zeros_like(self.master)
        self.v = torch.zeros_like(self.master)
        self.work = self.master.to(torch.bfloat16)
        self.ctl_f, self.ctl_i = _ctl()

    def step(self, g):
        g = g.to(DEV)
        _norm(self.ops, g, self.ctl_f, self.ctl_i, **self.kw)
        self.ops.adamw_step_guarded(self.master, g, self.m, self.v,
                                    self.work, self.ctl_f, self.ctl_i,
                                    HP["beta1"], HP["beta2"], HP["eps"],
                                    HP["wd"])

    def tensors(self):
        return dict(master=self.master, m=self.m, v=self.v, work=self.work)

    def bits(self):
        out = {k: t.clone().view(torch.int16 if t.dtype == torch.bfloat16
                                 else torch.int32)
               for k, t in self.tensors().items()}
        out["t"] = self.ctl_i[self.ops.CTL_T].clone()
        return out


def _guard_kw(skip=False):
    return dict(max_norm=C.GUARD["max_norm"], skip_nonfinite=skip,
                schedule=C.GUARD["schedule"], lr_max=HP["lr"],
                min_lr=C.GUARD["min_lr"],
                warmup_steps=C.GUARD["warmup_steps"],
                total_steps=C.GUARD["total_steps"])


# ---------------------------------------------------------------------------
# 8. norm accuracy / 9. the norm repeats
# ---------------------------------------------------------------------------
def _norm_sizes():
    return [1, 7, 4099, N.ew_loop_n(_max_resident_blocks())]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", _norm_sizes())
def test_grad_norm_accuracy(n, dtype):
    """Sum of squares (the partials, folded in double as step_ctl_k folds
    them) against N.l2norm_sq, and grad_norm against its square root. The
    largest n makes the capped grid go round more than once."""
    ops = _ops()
    x = torch.randn(n, generator=torch.Generator().manual_seed(22)).to(dtype)
    ctl_f, ctl_i = _ctl()
    part = _norm(ops, x.to(DEV), ctl_f, ctl_i, max_norm=1.0)
    assert bool(torch.isfinite(part).all()), "a partial was not stored"
    exact = N.l2norm_sq(N.d(x)).reshape(1)
    rounded = N.l2norm_sq(N.d(x), "rounded").reshape(1)
    case = f"{n}-{str(dtype).split('.')[-1]}"
    N.check("grad_sumsq", case, "sum", part.double().sum().reshape(1).cpu(),
            exact, rounded, row_dim=None, fp32_out=True)
    N.check("grad_sumsq", case, "norm", ctl_f[ops.CTL_NORM].reshape(1),
            exact.sqrt(), N.f32(rounded.sqrt()), row_dim=None, fp32_out=True)
    # coef is the clip formula on that norm, evaluated in fp32
    norm = np.float32(ctl_f[ops.CTL_NORM].item())
    c = np.float32(1.0) / (norm + np.float32(1e-6))
    assert ctl_f[ops.CTL_COEF].item() == (np.float32(1.0) if c > 1 else c)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
def test_grad_norm_repeats_bit_for_bit(dtype):
    ops = _ops()
    x = torch.randn(4099, generator=torch.Generator().manual_seed(23)
                    ).to(dtype).to(DEV)
    runs = []
    for _ in range(2):
        ctl_f, ctl_i = _ctl()
        part = _norm(ops, x, ctl_f, ctl_i, max_norm=1.0)
        runs.append((part.view(torch.int32).clone(),
                     ctl_f[ops.CTL_NORM].view(torch.int32).clone()))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])
    assert float(ctl_f[ops.CTL_NORM]) > 0


# ---------------------------------------------------------------------------
# 10. guarded AdamW accuracy
# ---------------------------------------------------------------------------
def test_guarded_adamw_accuracy():
    """Three steps that clip, do not clip, clip, under warmup 2 then cosine
    to step 4: lr, the clip factor and the bias corrections all come from
    the control block."""
    ops = _ops()
    c = C.guard_case()
    st = _State(ops, c["master"], **_guard_kw())
    coefs, lrs = [], []
    for g in c["grads"]:
        st.step(g)
        coefs.append(st.ctl_f[ops.CTL_COEF].item())
        lrs.append(st.ctl_f[ops.CTL_LR].item())
    assert coefs[0] < 0.02 and coefs[1] == 1.0 and coefs[2] < 0.01, coefs
    for s, lr in enumerate(lrs, start=1):
        want = C.closed_form_lr(C.GUARD["schedule"], s, HP["lr"],
                                C.GUARD["min_lr"], C.GUARD["warmup_steps"],
                                C.GUARD["total_steps"])
        assert abs(lr - want) <= 2.0 ** -23 * want, (s, lr, want)
    assert st.ctl_i.tolist() == [3, 3, 0, 0]
    for name, fp32 in N.ADAMW_TENSORS:
        N.check("adamw_guarded", "clip-cosine", name, st.tensors()[name],
                c["exact"][name], c["rounded"][name], row_dim=None,
                fp32_out=fp32)


# ---------------------------------------------------------------------------
# 11. a guard that never fires
# ---------------------------------------------------------------------------
def test_guard_that_never_fires_is_bit_identical_to_plain_step():
    ops = _ops()
    c = C.guard_case()
    st = _State(ops, c["master"], max_norm=1e30, skip_nonfinite=True,
                schedule="constant", lr_max=HP["lr"])
    master = c["master"].to(DEV).clone()
    m, v = torch.zeros_like(master), torch.zeros_like(master)
    work = master.to(torch.bfloat16)
    t_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    bc = torch.zeros(2, dtype=torch.float32, device=DEV)
    for g in c["grads"]:
        st.step(g)
        ops.adamw_tick(t_dev, bc, HP["beta1"], HP["beta2"])
        ops.adamw_step(master, g.to(DEV), m, v, work, 0, HP["lr"],
                       HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], bc=bc)
    assert st.ctl_f[ops.CTL_COEF].item() == 1.0
    assert st.ctl_i.tolist() == [3, 3, 0, 0]
    plain = dict(master=master, m=m, v=v, work=work)
    for name, t in st.tensors().items():
        assert torch.equal(t, plain[name]), name


# ---------------------------------------------------------------------------
# 12. skip on the device
# ---------------------------------------------------------------------------
def _poisoned(g, kind):
    g = g.clone()
    if kind == "nan_tail":
        g[-1] = float("nan")          # the scalar tail of n = 4099
    elif kind == "inf_first":
        g[3] = float("inf")           # inside the first vector
    else:
        g[1234] = 3e38                # finite; its square overflows fp32
        assert bool(torch.isfinite(g.float()).all())
    return g


def test_nonfinite_gradient_skips_on_device():
    ops = _ops()
    c = C.guard_case()
    kw = dict(_guard_kw(skip=True), total_steps=8)
    st = _State(ops, c["master"], **kw)
    g0, g1, g2 = c["grads"]
    bad = [_poisoned(g1, k) for k in ("nan_tail", "inf_first", "overflow")]
    st.step(g0)
    keep = st.bits()
    for i, g in enumerate(bad, start=1):
        st.step(g)
        now = st.bits()
        for k in keep:
            assert torch.equal(now[k], keep[k]), (i, k)
        assert st.ctl_i.tolist() == [1, 1 + i, 1, i]
    st.step(g2)
    assert st.ctl_i.tolist() == [2, 5, 0, 3]
    a = (N.d(c["master"]), [N.d(g) for g in [g0] + bad + [g2]])
    rkw = dict(HP, **C.GUARD, skip_nonfinite=True)
    rkw["total_steps"] = 8
    # the fp64 reference sees 3e38 ** 2 as finite: give it the fp32 view
    a[1][3][1234] = float("inf")
    exact = C.guarded_adamw(*a, **rkw)
    rounded = C.guarded_adamw(*a, **rkw, mode="rounded")
    assert exact["t"] == 2 and exact["skipped"] == 3
    for name, fp32 in N.ADAMW_TENSORS:
        N.check("adamw_guarded", "after-skips", name, st.tensors()[name],
                exact[name], rounded[name], row_dim=None, fp32_out=fp32)


# ---------------------------------------------------------------------------
# 13. graph replay with a moving lr
# ---------------------------------------------------------------------------
def test_graphed_guarded_step_matches_eager():
    from distributedtraining_amd.config import (Config, ModelConfig,
                                                TrainConfig)
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.parallel.flat import FlatParams
    from distributedtraining_amd.parallel.graphstep import GraphedMinerStep
    from distributedtraining_amd.roles.miner import DeltaLoop
    from distributedtraining_amd.utils.data import synthetic_batches

    cfg = Config()
    cfg.model = ModelConfig.gpt2_tiny()

    def mk(schedule):
        torch.manual_seed(0)
        model = build_model(cfg.model).to(DEV)
        fp = FlatParams(model)
        data = synthetic_batches(cfg.model.vocab_size, 4, 32, seed=1)
        # "constant" without the warmup: all eight steps of this test lie
        # inside the 16 warmup steps, where every schedule is the same ramp;
        # a constant lr is what an lr frozen at capture looks like
        warm = 0 if schedule == "constant" else 16
        tcfg = TrainConfig(lr=1e-2, lr_schedule=schedule, warmup_steps=warm,
                           total_steps=64, max_grad_norm=1.0,
                           skip_nonfinite=True)
        return DeltaLoop(model, fp, data, tcfg)

    batches = [{k: t.to(DEV) for k, t in b.items()}
               for b in [next(synthetic_batches(cfg.model.vocab_size, 4, 32,
                                                seed=9)) for _ in range(4)]]

    def graphed(schedule):
        g = mk(schedule)
        gs = GraphedMinerStep(g, batches, warmup=3)
        for i in range(5):
            gs.step(batches[i % 4])
        torch.cuda.synchronize()
        return g

    eager = mk("linear")
    start = eager.fp.master.clone()
    for _ in range(3):
        eager.train_step(batches[0])
    for i in range(5):
        eager.train_step(batches[i % 4])
    g = graphed("linear")
    torch.testing.assert_close(g.fp.master, eager.fp.master, rtol=1e-4,
                               atol=1e-4)
    assert g.step_count == eager.step_count
    assert float((g.fp.master - start).abs().max()) > 1e-3   # it trained
    assert g.opt.ctl_i.tolist() == eager.opt.ctl_i.tolist() == [8, 8, 0, 0]
    assert g.opt.lr_now.item() == np.float32(1e-2 * 8 / 16)
    assert float(g.opt.grad_norm) > 0
    # an lr frozen at capture would be caught: the constant schedule ends
    # more than ten tolerances away
    const = graphed("constant")
    assert float((const.fp.master - g.fp.master).abs().max()) > 1e-3
