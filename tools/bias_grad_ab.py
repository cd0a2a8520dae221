#!/usr/bin/env python3
"""A/B of the bias and norm-parameter gradient kernels at the flagship
shapes, each DTA_MLP_NODE setting in a fresh child process (the switch is
read once per process). Every gradient is delivered into a bf16 flat-plane
view, as the training step does.

  GELU backward + fc bias:  [65536, 3072] bf16. DTA_MLP_NODE=1:
      gelu_bwd_colsum (one pass); 0: gelu_bwd, then colsum over dh_pre
  colsum:       [65536, 768], [65536, 2304], [65536, 3072]
  LN backward:  [65536, 768], dγ/dβ into their views

--root DIR loads another checkout's build. One from before the finisher
(no gelu_bwd_colsum binding) is timed with what it runs per parameter:
zero-fill + atomic reduce inside colsum / layernorm_bwd, then
accum_f32_into_bf16.

Device-event times, median and min over --rounds rounds of --iters calls.
Compare only within one run of this script.

    python tools/bias_grad_ab.py [--rounds 7] [--iters 5] [--md out.md]
    python tools/bias_grad_ab.py --root ../parent-checkout
    python tools/bias_grad_ab.py --gelu-stripes 341 682 1024 1365 2048
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROWS = 65536
COLSUM_COLS = (768, 2304, 3072)


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


def child(args):
    sys.path.insert(0, os.path.abspath(args.root) if args.root else _root)
    import torch
    from distributedtraining_amd import ops
    from distributedtraining_amd.ops import droprng
    from distributedtraining_amd.ops.backend import require_ext
    m = require_ext()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    new = hasattr(m, "gelu_bwd_colsum")
    node = new and getattr(ops, "_MLP_NODE", False)
    res = {"build": "finisher" if new else "atomic reduce", "node": bool(node)}
    t = (args.rounds, args.iters, args.warmup)

    def rand(*shape):
        return torch.randn(*shape, device=dev, generator=g).to(torch.bfloat16)

    def colsum_into(x, dst):
        if new:
            m.colsum(x, dst)
        else:
            m.accum_f32_into_bf16(dst, m.colsum(x))

    # one element in: flat-plane views are unpadded
    plane = torch.zeros(2 * 3072 + 1, dtype=torch.bfloat16, device=dev)
    dh, pre = rand(ROWS, 3072), rand(ROWS, 3072).mul_(2.0)
    dst = plane[1:1 + 3072]
    _time(lambda: m.gelu_bwd(dh, pre), *t)   # clocks up before the first figure
    if node:
        res["gelu_ms"] = _time(lambda: m.gelu_bwd_colsum(dh, pre, dst), *t)
        res["gelu_stripes_ms"] = {
            st: _time(lambda st=st: m.gelu_bwd_colsum(dh, pre, dst, st), *t)
            for st in args.gelu_stripes}
    else:
        res["gelu_ms"] = _time(
            lambda: colsum_into(m.gelu_bwd(dh, pre), dst), *t)
    del pre
    res["colsum_ms"] = {}
    for cols in COLSUM_COLS:
        x = dh.view(-1)[:ROWS * cols].view(ROWS, cols)
        d = plane[1:1 + cols]
        res["colsum_ms"][cols] = _time(lambda: colsum_into(x, d), *t)
    del dh

    x, dy = rand(ROWS, 768), rand(ROWS, 768)
    w, b = rand(768), rand(768)
    rng = droprng.counter(dev)
    e = x.new_empty(0)
    _y, mean, rstd, _s = m.layernorm_fwd(x, e, w, b, 1e-5, rng, 0, 0.0)
    dw, db = plane[1:769], plane[769:1537]

    def ln_bwd():
        if new:
            m.layernorm_bwd(dy, e, x, w, mean, rstd, rng, 0, 0.0, dw, db)
        else:
            o = m.layernorm_bwd(dy, e, x, w, mean, rstd, rng, 0, 0.0)
            m.accum_f32_into_bf16(dw, o[1])
            m.accum_f32_into_bf16(db, o[2])

    res["ln_bwd_ms"] = _time(ln_bwd, *t)
    print("AB_RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gelu-stripes", type=int, nargs="*", default=[],
                    help="also time gelu_bwd_colsum at these row-stripe "
                         "counts (automatic: 1023 at [65536, 3072])")
    ap.add_argument("--root", default=None,
                    help="also time the build of this checkout")
    ap.add_argument("--md", default=None, help="also write the table here")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bias_grad_ab needs a GPU: nothing is measured without one")
    runs = [("1", None), ("0", None)] + ([("1", args.root)] if args.root
                                         else [])
    rows = []
    for node, root in runs:
        env = dict(os.environ, DTA_MLP_NODE=node)
        env.pop("PYTHONPATH", None)
        cmd = [sys.executable, os.path.abspath(__file__), "--child",
               "--rounds", str(args.rounds), "--iters", str(args.iters),
               "--warmup", str(args.warmup)]
        if root:
            cmd += ["--root", root]
        elif node == "1" and args.gelu_stripes:
            cmd += ["--gelu-stripes"] + [str(v) for v in args.gelu_stripes]
        out = subprocess.run(cmd, env=env, check=True, timeout=600,
                             cwd=os.path.abspath(root) if root else _root,
                             stdout=subprocess.PIPE, text=True).stdout
        line = [ln for ln in out.splitlines()
                if ln.startswith("AB_RESULT ")][-1]
        rows.append(json.loads(line[len("AB_RESULT "):]))
    head = ["build", "DTA_MLP_NODE", "GELU bwd + fc dbias"] + [
        f"colsum {c}" for c in COLSUM_COLS] + ["LN bwd 768"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]

    def f(mm):
        return f"{mm[0]:.3f} / {mm[1]:.3f}"

    for r in rows:
        lines.append("| " + " | ".join(
            [r["build"], str(int(r["node"])), f(r["gelu_ms"])]
            + [f(r["colsum_ms"][str(c)]) for c in COLSUM_COLS]
            + [f(r["ln_bwd_ms"])]) + " |")
    for r in rows:
        for st, mm in r.get("gelu_stripes_ms", {}).items():
            lines.append(f"| gelu_bwd_colsum, {st} row stripes | | {f(mm)} |"
                         + " |" * (len(head) - 3))
    table = "\n".join(lines)
    print(f"device: {torch.cuda.get_device_name(0)}; rows={ROWS}; ms, "
          f"median / min; rounds={args.rounds} iters={args.iters} "
          f"warmup={args.warmup}")
    print(table)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
