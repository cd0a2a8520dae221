#!/usr/bin/env python3
"""A/B of the whole weight-gradient op, gradients delivered into bf16
flat-plane views as the training step does:

  kernel   m.wgrad.bias(dy, x, dW, db)            (hip/wgrad.hip)
  library  dW.addmm_(dy.t(), x) + m.colsum(dy, db), TunableOp on with the
           committed selections of tuning/ (read only: tuning stays off)

at the four flagship linears (T = 65536) and at T = 32768. mlp fc is timed
without a bias in both arms: its bias comes from gelu_bwd_colsum.

The rounds alternate between the arms in ONE process; device-event times over
--iters calls per round; median / min / max over --rounds rounds. A shape
belongs in ops._WGRAD_WINS only if the kernel's median beats the library's
median by more than the library's own spread (max - min). Compare only within
one run of this script.

    python tools/wgrad_ab.py [--rounds 9] [--iters 5] [--md out.md]
    python tools/wgrad_ab.py --nsplit 4 7 9 14 18 28     # forced split sweep
"""
import argparse
import os
import statistics
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)
if os.path.exists(os.path.join(_root, "tuning", "tunableop0.csv")):
    os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
    os.environ.setdefault("PYTORCH_TUNABLEOP_TUNING", "0")
    os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME",
                          os.path.join(_root, "tuning", "tunableop.csv"))
    os.environ.setdefault("PYTORCH_TUNABLEOP_VERBOSE", "0")

# name, out, in, bias delivered by this op
LINEARS = (("qkv", 2304, 768, True), ("attn proj", 768, 768, True),
           ("mlp fc", 3072, 768, False), ("mlp proj", 768, 3072, True))
TS = (65536, 32768)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nsplit", type=int, nargs="*", default=[],
                    help="also time the kernel at these forced split counts")
    ap.add_argument("--T", type=int, nargs="*", default=list(TS))
    ap.add_argument("--md", default=None, help="also write the table here")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("wgrad_ab needs a GPU: nothing is measured without one")
    from distributedtraining_amd.ops.backend import require_ext
    m = require_ext()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)

    def rand(r, c, scale):
        return (torch.randn(r, c, device=dev, generator=g) * scale) \
            .to(torch.bfloat16)

    def ev_time(fn):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.iters

    head = ["T", "linear", "out x in", "arm", "splits", "median ms", "min",
            "max", "TFLOP/s (median)", "verdict"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for T in args.T:
        for name, out, inp, bias in LINEARS:
            dy, x = rand(T, out, 0.05), rand(T, inp, 0.5)
            # one element in: flat-plane views are unpadded
            plane = torch.zeros(out * inp + out + 1, dtype=torch.bfloat16,
                                device=dev)
            dw = plane[1:1 + out * inp].view(out, inp)
            db = plane[1 + out * inp:] if bias else None

            def lib():
                dw.addmm_(dy.t(), x)
                if bias:
                    m.colsum(dy, db)

            arms = [("library", 0, lib)]
            for ns in [0] + list(args.nsplit):
                arms.append(("kernel", ns, lambda ns=ns: m.wgrad.bias(
                    dy, x, dw, db, False, ns)))
            for _n, _s, fn in arms:
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            times = [[] for _ in arms]
            for _ in range(args.rounds):          # arms alternate per round
                for i, (_n, _s, fn) in enumerate(arms):
                    times[i].append(ev_time(fn))
                plane.zero_()
            lmed = statistics.median(times[0])
            lspread = max(times[0]) - min(times[0])
            for (arm, ns, _f), ts in zip(arms, times):
                med = statistics.median(ts)
                shown = ns if ns else (m.wgrad.nsplit(T, out, inp)
                                       if arm == "kernel" else "")
                verdict = ""
                if arm == "kernel":
                    verdict = ("wins" if lmed - med > lspread else
                               "library stays")
                lines.append(
                    f"| {T} | {name} | {out} x {inp} | {arm} | {shown} | "
                    f"{med:.4f} | {min(ts):.4f} | {max(ts):.4f} | "
                    f"{2.0 * T * out * inp / med / 1e9:.0f} | {verdict} |")
            del dy, x, plane
    table = "\n".join(lines)
    print(f"device: {torch.cuda.get_device_name(0)}; ms per call; "
          f"rounds={args.rounds} iters={args.iters} warmup={args.warmup}")
    print(table)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
