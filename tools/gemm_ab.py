#!/usr/bin/env python3
"""A/B of the forward projections, per shape:

  kernel   m.gemm.fwd(x, w, b, epi)                       (hip/gemm.hip)
  library  torch.addmm(b, x, w.t()) (+ m.gelu_fwd for mlp fc), TunableOp on
           with the committed selections of tuning/ (read only: tuning off)

at the four flagship linears (T = 65536) and at T = 32768. mlp fc is one
"bias_gelu" call against addmm + gelu_fwd; the others carry the bias.

The rounds alternate between the arms in ONE process; device-event times over
--iters calls per round; median / min / max over --rounds rounds. A shape
belongs in ops._GEMM_WINS only if the kernel's median beats the library's
median by more than the library's own spread (max - min). --pipes 1 2 times
both K-loop pipelines of gemm.hip; the verdict column is the default one's.
Compare only within one run of this script. The checksums of tuning/ are
printed before and after: they must be equal.

    python tools/gemm_ab.py [--rounds 9] [--iters 5] [--pipes 1 2] [--md out.md]
"""
import argparse
import glob
import hashlib
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

# name, N, K, epilogue
LINEARS = (("qkv", 2304, 768, "bias"), ("attn proj", 768, 768, "bias"),
           ("mlp fc", 3072, 768, "bias_gelu"), ("mlp proj", 768, 3072, "bias"))
TS = (65536, 32768)
PIPE_NAMES = {0: "default", 1: "2x32", 2: "3x64"}


def tuning_sums():
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(_root, "tuning", "*"))):
        with open(f, "rb") as fh:
            h.update(os.path.basename(f).encode() + b"\0" + fh.read())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pipes", type=int, nargs="*", default=[],
                    help="also time the kernel with these forced pipelines")
    ap.add_argument("--T", type=int, nargs="*", default=list(TS))
    ap.add_argument("--md", default=None, help="also write the table here")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gemm_ab needs a GPU: nothing is measured without one")
    from distributedtraining_amd.ops.backend import require_ext
    m = require_ext()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    before = tuning_sums()

    def rand(*shape, scale):
        return (torch.randn(*shape, device=dev, generator=g) * scale) \
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

    head = ["T", "linear", "N x K", "epilogue", "arm", "median ms", "min",
            "max", "TFLOP/s (median)", "verdict"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for T in args.T:
        for name, N, K, epi in LINEARS:
            x, w = rand(T, K, scale=0.5), rand(N, K, scale=0.05)
            b = rand(N, scale=0.1)

            def lib():
                pre = torch.addmm(b, x, w.t())
                return m.gelu_fwd(pre) if epi == "bias_gelu" else pre

            arms = [("library", lib)]
            for pipe in [0] + list(args.pipes):
                arms.append((f"kernel {PIPE_NAMES[pipe]}",
                             lambda pipe=pipe: m.gemm.fwd(x, w, b, epi, pipe)))
            for _n, fn in arms:
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            times = [[] for _ in arms]
            for _ in range(args.rounds):          # arms alternate per round
                for i, (_n, fn) in enumerate(arms):
                    times[i].append(ev_time(fn))
            lmed = statistics.median(times[0])
            lspread = max(times[0]) - min(times[0])
            for (arm, _f), ts in zip(arms, times):
                med = statistics.median(ts)
                verdict = ""
                if arm != "library":
                    verdict = ("wins" if lmed - med > lspread else
                               "library stays")
                lines.append(
                    f"| {T} | {name} | {N} x {K} | {epi} | {arm} | "
                    f"{med:.4f} | {min(ts):.4f} | {max(ts):.4f} | "
                    f"{2.0 * T * N * K / med / 1e9:.0f} | {verdict} |")
            del x, w, b
    after = tuning_sums()
    table = "\n".join(lines)
    print(f"device: {torch.cuda.get_device_name(0)}; ms per call; "
          f"rounds={args.rounds} iters={args.iters} warmup={args.warmup}")
    print(f"tuning/ sha256 before {before[:16]} after {after[:16]} "
          f"{'equal' if before == after else 'CHANGED'}")
    print(table)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
