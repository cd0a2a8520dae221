#!/usr/bin/env python3
"""Cost of the guarded optimizer step (clip / non-finite skip / LR schedule)
against the plain one, kernel group by kernel group, on bf16 gradients and a
bf16 working copy as the training step has them.

  plain step     adamw_tick_k + adamw_k<true, true, false>
  guarded step   gradnorm_part_k + step_ctl_k + adamw_k<true, true, true>
  schedule only  step_ctl_k (no partials) + adamw_k<true, true, true>

at the flat-plane size of GPT-2-small (124,439,808 elements) and at 4099
elements (launch floor). Device-event times, median and min over --rounds
rounds of --iters calls. Compare only within one run of this script.

    python tools/guarded_step_ab.py [--rounds 9] [--iters 20] [--md out.md]
"""
import argparse
import json
import os
import statistics
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)


def gpt2_small_numel() -> int:
    from distributedtraining_amd.config import ModelConfig
    c = ModelConfig.gpt2_small()
    e = c.n_embd
    return (c.vocab_size * e + c.n_positions * e
            + c.n_layer * (12 * e * e + 13 * e) + 2 * e)


def _time(fn, rounds, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out)


ROWS = ("plain: tick + adamw_k", "plain: adamw_k alone",
        "guarded: norm pass", "guarded: step_ctl_k (with partials)",
        "guarded: step_ctl_k (schedule only)", "guarded: adamw_k<CTL>",
        "guarded step, all three", "schedule-only step, two kernels")


def measure(n, args):
    import torch
    from distributedtraining_amd import ops
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    master = torch.randn(n, device=dev, generator=g)
    grad = (torch.randn(n, device=dev, generator=g) * 0.02).to(torch.bfloat16)
    m, v = torch.zeros_like(master), torch.zeros_like(master)
    work = master.to(torch.bfloat16)
    t_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    bc = torch.zeros(2, dtype=torch.float32, device=dev)
    ctl_f = torch.zeros(6, dtype=torch.float32, device=dev)
    ctl_i = torch.zeros(4, dtype=torch.int32, device=dev)
    part = torch.zeros(ops.grad_sumsq_blocks(n, grad.dtype, grad.device),
                       dtype=torch.float32, device=dev)
    b1, b2, eps, wd, lr = 0.9, 0.999, 1e-8, 0.01, 5e-4
    sched = dict(schedule="cosine", lr_max=lr, min_lr=lr / 10,
                 warmup_steps=100, total_steps=100000)

    def tick():
        ops.adamw_tick(t_dev, bc, b1, b2)

    def plain():
        ops.adamw_step(master, grad, m, v, work, 0, lr, b1, b2, eps, wd,
                       bc=bc)

    def norm():
        ops.grad_sumsq_partials(grad, part)

    def ctl():
        ops.step_control(part, ctl_f, ctl_i, b1, b2, max_norm=1.0,
                         skip_nonfinite=True, **sched)

    def ctl_sched():
        ops.step_control(None, ctl_f, ctl_i, b1, b2, **sched)

    def guarded():
        ops.adamw_step_guarded(master, grad, m, v, work, ctl_f, ctl_i, b1,
                               b2, eps, wd)

    fns = (lambda: (tick(), plain()), plain, norm, ctl, ctl_sched, guarded,
           lambda: (norm(), ctl(), guarded()),
           lambda: (ctl_sched(), guarded()))
    t = (args.rounds, args.iters, args.warmup)
    tick(), norm(), ctl()        # a valid control block before adamw_k<CTL>
    _time(fns[0], *t)            # clocks up before the first figure
    res = {name: _time(fn, *t) for name, fn in zip(ROWS, fns)}
    torch.cuda.synchronize()
    assert int(ctl_i[2]) == 0 and bool(torch.isfinite(master).all())
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--md", help="also write the table to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("guarded_step_ab.py times kernels: it needs the GPU")
    from distributedtraining_amd.ops.backend import require_ext
    require_ext()
    sizes = (gpt2_small_numel(), 4099)
    res = {n: measure(n, args) for n in sizes}
    lines = ["| kernels | " + " | ".join(
        f"n = {n:,}: ms median / min" for n in sizes) + " |",
        "|---|" + "---|" * len(sizes)]
    for name in ROWS:
        lines.append(f"| {name} | " + " | ".join(
            "{:.4f} / {:.4f}".format(*res[n][name]) for n in sizes) + " |")
    n0 = sizes[0]
    base = res[n0][ROWS[0]][0]
    add = res[n0][ROWS[6]][0] - base
    lines += ["", f"At n = {n0:,}: the guarded step adds {add:.4f} ms to the "
              f"plain step's {base:.4f} ms ({100 * add / base:.1f} %); the "
              f"byte model (2 of 28 B per parameter) says 7.1 %."]
    text = "\n".join(lines)
    print(text)
    print(json.dumps({str(n): {k: list(v) for k, v in r.items()}
                      for n, r in res.items()}))
    if args.md:
        with open(args.md, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
