"""Guarded optimizer step on the CPU path: clipping against torch, the LR
schedule against its closed form, the non-finite skip, the plumbing
(TrainConfig, flags, resume), and a self-check that the accuracy bounds of
the GPU tests (tests/test_guarded_step_gpu.py) reject wrong kernels.

The fp64 reference of guarded AdamW lives here (``guarded_adamw``): N.adamw
generalised to a per-step lr and clip factor. The GPU tests import it.
"""

import functools
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import _numerics as N

from distributedtraining_amd import ops
from distributedtraining_amd.config import (Config, ModelConfig, TrainConfig,
                                            from_args)
from distributedtraining_amd.parallel.flat import FlatParams, FusedAdamW


# ---------------------------------------------------------------------------
# References
# ---------------------------------------------------------------------------
def closed_form_lr(schedule, s, lr_max, min_lr, warmup_steps, total_steps):
    """The schedule at step s (from 1), in Python doubles."""
    if s <= warmup_steps:
        return lr_max * s / warmup_steps
    p = min(1, (s - warmup_steps) / max(1, total_steps - warmup_steps))
    if schedule == "constant":
        return lr_max
    if schedule == "linear":
        return lr_max + (min_lr - lr_max) * p
    return min_lr + 0.5 * (lr_max - min_lr) * (1 + math.cos(math.pi * p))


def guarded_adamw(master, grads, lr, beta1, beta2, eps, wd, max_norm=0.0,
                  schedule="constant", warmup_steps=0, total_steps=0,
                  min_lr=0.0, skip_nonfinite=False, mode="exact", mut=None):
    """N.adamw with a per-step lr and clip factor. master fp64 (fp32
    values); grads: fp64 tensors holding the values the kernel reads, from
    which the norm is taken. ``rounded``: the same in fp32 torch, lr rounded
    to fp32. Returns master, m, v, work and the counters t, skipped.
    Mutants: no_clip; coef_m_only (clip factor on m, raw gradient in v);
    lr_prev (lr of step s - 1); t_on_skip (t advanced on a skipped step)."""
    mut = mut or {}
    rounded = mode == "rounded"
    dt = torch.float32 if rounded else N.F64
    w = master.to(dt).clone()
    m = torch.zeros_like(w)
    v = torch.zeros_like(w)
    t = skipped = 0
    for s, g in enumerate(grads, start=1):
        g = g.to(dt)
        sumsq = (g * g).sum()
        coef = torch.ones((), dtype=dt)
        if max_norm > 0 and not mut.get("no_clip"):
            coef = torch.clamp(max_norm / (sumsq.sqrt() + 1e-6), max=1.0)
        lr_s = closed_form_lr(schedule, s - 1 if mut.get("lr_prev") else s,
                              lr, min_lr, warmup_steps, total_steps)
        if rounded:
            lr_s = float(np.float32(lr_s))
        if skip_nonfinite and not bool(torch.isfinite(sumsq)):
            skipped += 1
            t += 1 if mut.get("t_on_skip") else 0
            continue
        t += 1
        bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
        w = w * (1.0 - lr_s * wd)
        gm = g * coef
        gv = g if mut.get("coef_m_only") else gm
        m = beta1 * m + (1.0 - beta1) * gm
        v = beta2 * v + (1.0 - beta2) * gv * gv
        w = w - (lr_s / bc1) * m / (torch.sqrt(v / bc2) + eps)
    return dict(master=w.to(N.F64), m=m.to(N.F64), v=v.to(N.F64),
                work=N.bf16(w.to(N.F64)) if rounded else w.to(N.F64),
                t=t, skipped=skipped)


# N.adamw_case's master and gradients; the gradients scaled so that their
# norms are about 64, 0.32 and 192: clip, no clip, clip at max_norm = 1
GRAD_SCALES = (1.0, 0.005, 3.0)
GUARD = dict(max_norm=1.0, schedule="cosine", warmup_steps=2, total_steps=4,
             min_lr=1e-3)


def scaled_grads():
    c = N.adamw_case()
    return [(g.float() * s).to(torch.bfloat16)
            for g, s in zip(c["grads"], GRAD_SCALES)]


@functools.lru_cache(maxsize=None)
def guard_case():
    c = N.adamw_case()
    grads = scaled_grads()
    a = (N.d(c["master"]), [N.d(g) for g in grads])
    return dict(master=c["master"], grads=grads, args=a,
                exact=guarded_adamw(*a, **N.ADAMW_HP, **GUARD),
                rounded=guarded_adamw(*a, **N.ADAMW_HP, **GUARD,
                                      mode="rounded"))


# ---------------------------------------------------------------------------
# Helpers
# ---------------------------------------------------------------------------
def _mlp():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(5, 7), nn.Tanh(), nn.Linear(7, 3))


def _mlp_opt(**kw):
    model = _mlp()
    fp = FlatParams(model)
    return model, fp, FusedAdamW(fp, lr=1e-2, weight_decay=0.05, **kw)


def _bits(t):
    return t.detach().clone().view(torch.int32)


# ---------------------------------------------------------------------------
# 1. clipping against torch
# ---------------------------------------------------------------------------
def test_clipping_matches_torch_clip_grad_norm():
    model, fp, opt = _mlp_opt(max_grad_norm=1.0)
    ref = _mlp()
    ropt = torch.optim.AdamW(ref.parameters(), lr=1e-2, betas=(0.9, 0.999),
                             eps=1e-8, weight_decay=0.05)
    g0 = torch.Generator().manual_seed(3)
    x = torch.randn(16, 5, generator=g0)
    y = torch.randn(16, 3, generator=g0)
    assert opt.guarded
    for target in (5.0, 0.2, 5.0):      # above, below, above the threshold
        for mdl in (model, ref):
            (mdl(x) - y).pow(2).mean().backward()
        raw = torch.cat([p.grad.reshape(-1) for p in ref.parameters()]).norm()
        f = float(target / raw)
        fp.grad.mul_(f)
        for p in ref.parameters():
            p.grad.mul_(f)
        before = fp.grad.clone()
        total = torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
        opt.step()
        assert torch.equal(fp.grad, before), "the gradient plane was modified"
        torch.testing.assert_close(opt.grad_norm, total)
        coef = float(opt.ctl_f[ops.CTL_COEF])
        assert (coef < 1.0) == (target > 1.0), (target, coef)
        ropt.step()
        opt.zero_grad()
        ropt.zero_grad(set_to_none=False)
        o = 0
        for (_, shape, cnt), p in zip(fp.spec, ref.parameters()):
            torch.testing.assert_close(fp.master[o:o + cnt].view(shape),
                                       p.detach())
            torch.testing.assert_close(fp.work[o:o + cnt].view(shape),
                                       p.detach())
            o += cnt
    assert int(opt.ctl_i[ops.CTL_T]) == 3
    assert int(opt.skipped_steps) == 0


# ---------------------------------------------------------------------------
# 2. schedule against the closed form
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["constant", "linear", "cosine"])
def test_schedule_matches_closed_form(schedule):
    warmup, total, lr, min_lr = 4, 12, 1e-2, 1e-3
    _, _, opt = _mlp_opt(lr_schedule=schedule, warmup_steps=warmup,
                         total_steps=total, min_lr=min_lr)
    assert opt.guarded and opt.grad_norm is None
    for s in (1, warmup, warmup + 1, (warmup + total) // 2, total,
              total + 5):
        opt.set_schedule_step(s - 1)
        opt.step()
        want = np.float32(closed_form_lr(schedule, s, lr, min_lr, warmup,
                                         total))
        got = opt.lr_now
        assert got.dtype == torch.float32
        assert np.float32(got.item()) == want, (schedule, s, got.item(), want)
        assert int(opt.ctl_i[ops.CTL_SCHED]) == s
    if schedule != "constant":
        assert opt.lr_now.item() == np.float32(min_lr)


def test_schedule_runs_step_by_step():
    """Without set_schedule_step the clock advances one per step()."""
    _, _, opt = _mlp_opt(lr_schedule="linear", warmup_steps=2, total_steps=6)
    for s in range(1, 9):
        opt.step()
        assert np.float32(opt.lr_now.item()) == np.float32(
            closed_form_lr("linear", s, 1e-2, 0.0, 2, 6)), s


# ---------------------------------------------------------------------------
# 3. skip
# ---------------------------------------------------------------------------
def test_nonfinite_gradient_skips_the_step():
    g0 = torch.Generator().manual_seed(5)
    _, fp, opt = _mlp_opt(skip_nonfinite=True, lr_schedule="linear",
                          warmup_steps=2, total_steps=10)
    n = fp.numel
    grads = [torch.randn(n, generator=g0) for _ in range(2)]
    master0 = fp.master.clone()

    fp.grad.copy_(grads[0])
    opt.step()
    assert int(opt.ctl_i[ops.CTL_T]) == 1 and int(opt.skipped_steps) == 0
    keep = {k: _bits(t) for k, t in dict(master=fp.master, m=opt.m, v=opt.v,
                                         work=fp.work).items()}

    bad = grads[1].clone()
    bad[n // 2] = float("nan")
    fp.grad.copy_(bad)
    opt.step()
    now = dict(master=fp.master, m=opt.m, v=opt.v, work=fp.work)
    for k, t in now.items():
        assert torch.equal(_bits(t), keep[k]), k
    assert int(opt.ctl_i[ops.CTL_T]) == 1
    assert int(opt.skipped_steps) == 1
    assert int(opt.ctl_i[ops.CTL_SCHED]) == 2
    assert int(opt.ctl_i[ops.CTL_SKIP_NOW]) == 1

    # the next finite step is step t = 2 of AdamW at the schedule's s = 3
    fp.grad.copy_(grads[1])
    opt.step()
    assert int(opt.ctl_i[ops.CTL_T]) == 2 and int(opt.skipped_steps) == 1
    assert opt.ctl_f[ops.CTL_BC1].item() == np.float32(1.0 - 0.9 ** 2)
    assert opt.ctl_f[ops.CTL_BC2].item() == np.float32(1.0 - 0.999 ** 2)
    ref = guarded_adamw(N.d(master0), [N.d(grads[0]), N.d(bad),
                                       N.d(grads[1])],
                        lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.05,
                        schedule="linear", warmup_steps=2, total_steps=10,
                        skip_nonfinite=True)
    assert ref["t"] == 2 and ref["skipped"] == 1
    for k, t in dict(master=fp.master, m=opt.m, v=opt.v).items():
        torch.testing.assert_close(t, ref[k].float())


def test_skip_off_is_torch_semantics():
    """skip_nonfinite off: nothing is special-cased. A NaN norm makes the
    clip factor NaN and the whole update with it, as clip_grad_norm_ +
    AdamW would."""
    _, fp, opt = _mlp_opt(max_grad_norm=1.0)
    fp.grad.fill_(1.0)
    fp.grad[0] = float("nan")
    opt.step()
    assert math.isnan(float(opt.grad_norm))
    assert bool(torch.isnan(fp.master).all())
    assert int(opt.skipped_steps) == 0 and int(opt.ctl_i[ops.CTL_T]) == 1


# ---------------------------------------------------------------------------
# 4. defaults change nothing
# ---------------------------------------------------------------------------
def test_defaults_change_nothing():
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.roles.miner import DeltaLoop
    from distributedtraining_amd.utils.data import synthetic_batches

    mcfg = ModelConfig.gpt2_tiny()

    def run(tcfg):
        torch.manual_seed(0)
        model = build_model(mcfg)
        fp = FlatParams(model)
        miner = DeltaLoop(model, fp,
                          synthetic_batches(mcfg.vocab_size, 2, 16, seed=1),
                          tcfg)
        assert not miner.opt.guarded and miner.opt.ctl_f is None
        assert miner.opt.grad_norm is None and miner.opt.lr_now is None
        losses = [miner.train_step().clone() for _ in range(3)]
        return fp.master.clone(), miner.opt.m.clone(), miner.opt.v.clone(), \
            torch.stack(losses), miner.opt.t

    a = run(TrainConfig())
    b = run(TrainConfig(max_grad_norm=0.0, skip_nonfinite=False,
                        lr_schedule="constant", warmup_steps=0,
                        total_steps=0, min_lr=0.0))
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert a[4] == b[4] == 3


# ---------------------------------------------------------------------------
# 5. flags
# ---------------------------------------------------------------------------
def test_flag_parsing_and_validation():
    cfg = from_args(["--train.max-grad-norm", "1.0",
                     "--train.skip-nonfinite", "true",
                     "--train.lr-schedule", "cosine",
                     "--train.warmup-steps", "10",
                     "--train.total-steps", "100",
                     "--train.min-lr", "1e-5"])
    t = cfg.train
    assert (t.max_grad_norm, t.skip_nonfinite, t.lr_schedule, t.warmup_steps,
            t.total_steps, t.min_lr) == (1.0, True, "cosine", 10, 100, 1e-5)
    d0 = from_args([]).train
    assert (d0.max_grad_norm, d0.skip_nonfinite, d0.lr_schedule,
            d0.warmup_steps, d0.total_steps, d0.min_lr) == (
        0.0, False, "constant", 0, 0, 0.0)

    bad = [["--train.lr-schedule", "cosine"],                 # no total
           ["--train.lr-schedule", "linear", "--train.warmup-steps", "10",
            "--train.total-steps", "10"],                     # total = warmup
           ["--train.lr-schedule", "step"],
           ["--train.warmup-steps", "-1"],
           ["--train.max-grad-norm", "-1.0"],
           ["--train.min-lr", "1.0"]]                         # above lr
    for argv in bad:
        with pytest.raises(ValueError):
            from_args(argv)
    fp = FlatParams(_mlp())
    for kw in (dict(lr_schedule="cosine", warmup_steps=5, total_steps=5),
               dict(lr_schedule="linear"), dict(min_lr=1.0),
               dict(lr_schedule="exp"), dict(max_grad_norm=-1.0),
               dict(warmup_steps=-2)):
        with pytest.raises(ValueError):
            FusedAdamW(fp, **kw)


def test_delta_loop_passes_the_fields_through():
    from distributedtraining_amd.roles.miner import DeltaLoop
    model = _mlp()
    tcfg = TrainConfig(max_grad_norm=0.5, skip_nonfinite=True,
                       lr_schedule="linear", warmup_steps=3, total_steps=9,
                       min_lr=1e-5)
    opt = DeltaLoop(model, FlatParams(model), iter(()), tcfg).opt
    assert (opt.max_grad_norm, opt.skip_nonfinite, opt.lr_schedule,
            opt.warmup_steps, opt.total_steps, opt.min_lr) == (
        0.5, True, "linear", 3, 9, 1e-5)
    assert opt.guarded and opt.grad_norm is not None


# ---------------------------------------------------------------------------
# 6. resume; base install keeps the schedule clock
# ---------------------------------------------------------------------------
def test_set_schedule_step_resumes_the_schedule():
    kw = dict(lr_schedule="cosine", warmup_steps=3, total_steps=20,
              min_lr=1e-4)
    _, _, opt = _mlp_opt(**kw)
    opt.set_schedule_step(11)
    opt.step()
    assert np.float32(opt.lr_now.item()) == np.float32(
        closed_form_lr("cosine", 12, 1e-2, 1e-4, 3, 20))
    # unguarded optimizer: a no-op, as the miner calls it unconditionally
    _, _, plain = _mlp_opt()
    plain.set_schedule_step(11)
    plain.step()
    assert plain.t == 1


def test_reset_state_keeps_schedule_and_skip_count():
    _, fp, opt = _mlp_opt(skip_nonfinite=True, lr_schedule="linear",
                          warmup_steps=2, total_steps=10)
    fp.grad.fill_(0.5)
    opt.step()
    fp.grad[1] = float("inf")
    opt.step()
    fp.grad.fill_(0.5)
    opt.step()
    opt.reset_state()
    assert int(opt.ctl_i[ops.CTL_T]) == 0
    assert float(opt.m.abs().sum()) == 0.0 and float(opt.v.abs().sum()) == 0.0
    assert int(opt.ctl_i[ops.CTL_SCHED]) == 3 and int(opt.skipped_steps) == 1
    opt.step()
    assert int(opt.ctl_i[ops.CTL_T]) == 1
    assert opt.ctl_f[ops.CTL_BC1].item() == np.float32(1.0 - 0.9)
    assert np.float32(opt.lr_now.item()) == np.float32(
        closed_form_lr("linear", 4, 1e-2, 0.0, 2, 10))


def test_cli_miner_logs_the_guard_and_resumes_the_schedule(tmp_path):
    import json
    from distributedtraining_amd import cli
    common = ["--tiny", "--comm.root", str(tmp_path / "ex"),
              "--metrics-dir", str(tmp_path / "metrics"),
              "--train.batch-size", "2", "--train.seq-len", "16",
              "--train.lr", "1e-2", "--train.max-grad-norm", "1.0",
              "--train.skip-nonfinite", "true",
              "--train.lr-schedule", "linear", "--train.warmup-steps", "2",
              "--train.total-steps", "10"]
    assert cli.main(["miner", "--hotkey", "m0", "--steps", "3", *common]) == 0
    assert cli.main(["miner", "--hotkey", "m0", "--steps", "2", "--resume",
                     *common]) == 0
    with open(tmp_path / "metrics" / "miner_m0.jsonl") as f:
        rows = [json.loads(l) for l in f]
    rows = [r for r in rows if "grad_norm" in r]
    assert [r["step"] for r in rows] == [3, 5]
    for r in rows:
        assert r["grad_norm"] > 0 and r["skipped_steps"] == 0
        assert np.float32(r["lr"]) == np.float32(
            closed_form_lr("linear", r["step"], 1e-2, 0.0, 2, 10))


# ---------------------------------------------------------------------------
# 7. the bounds reject wrong kernels
# ---------------------------------------------------------------------------
def _rejected(got, exact, rounded):
    return [name for name, fp32 in N.ADAMW_TENSORS
            if not N.passes(got[name], exact[name], rounded[name],
                            row_dim=None, fp32_out=fp32)]


def test_guarded_adamw_rounded_feasible_and_mutants_rejected():
    c = guard_case()
    assert _rejected(c["rounded"], c["exact"], c["rounded"]) == []
    for name, fp32 in N.ADAMW_TENSORS:
        base, bound = N.bounds(c["exact"][name], c["rounded"][name],
                               row_dim=None, fp32_out=fp32)
        assert all(math.isfinite(b) for b in base + bound), name
    want = dict(no_clip=("m", "v"), coef_m_only=("v",), lr_prev=("master",))
    for mut, names in want.items():
        got = guarded_adamw(*c["args"], **N.ADAMW_HP, **GUARD,
                            mode="rounded", mut={mut: True})
        rej = _rejected(got, c["exact"], c["rounded"])
        assert rej, mut
        for nm in names:
            assert nm in rej, (mut, rej)

    # t advanced on a skipped step: a NaN gradient between two clean ones
    master, gs = c["args"]
    nan_g = gs[1].clone()
    nan_g[-1] = float("nan")
    seq = [gs[0], nan_g, gs[2]]
    kw = dict(N.ADAMW_HP, **GUARD, skip_nonfinite=True)
    exact = guarded_adamw(master, seq, **kw)
    rounded = guarded_adamw(master, seq, **kw, mode="rounded")
    assert exact["t"] == 2 and exact["skipped"] == 1
    assert _rejected(rounded, exact, rounded) == []
    got = guarded_adamw(master, seq, **kw, mode="rounded",
                        mut=dict(t_on_skip=True))
    assert got["t"] == 3
    assert "master" in _rejected(got, exact, rounded)


def test_cpu_ops_match_the_reference():
    """The CPU paths of the three ops against the fp64 reference, at the
    bounds the GPU kernels are held to."""
    c = guard_case()
    master = c["master"].clone()
    m, v = torch.zeros_like(master), torch.zeros_like(master)
    work = torch.empty(N.ADAMW_N, dtype=torch.bfloat16)
    ctl_f = torch.zeros(6)
    ctl_i = torch.zeros(4, dtype=torch.int32)
    hp = N.ADAMW_HP
    coefs = []
    for g in c["grads"]:
        part = torch.empty(ops.grad_sumsq_blocks(g.numel(), g.dtype,
                                                 g.device))
        ops.grad_sumsq_partials(g, part)
        ops.step_control(part, ctl_f, ctl_i, hp["beta1"], hp["beta2"],
                         GUARD["max_norm"], False, GUARD["schedule"],
                         hp["lr"], GUARD["min_lr"], GUARD["warmup_steps"],
                         GUARD["total_steps"])
        ops.adamw_step_guarded(master, g, m, v, work, ctl_f, ctl_i,
                               hp["beta1"], hp["beta2"], hp["eps"], hp["wd"])
        coefs.append(float(ctl_f[ops.CTL_COEF]))
    assert coefs[0] < 0.02 and coefs[1] == 1.0 and coefs[2] < 0.01, coefs
    got = dict(master=master, m=m, v=v, work=work)
    for name, fp32 in N.ADAMW_TENSORS:
        N.check("adamw_guarded", "cpu", name, got[name], c["exact"][name],
                c["rounded"][name], row_dim=None, fp32_out=fp32)
