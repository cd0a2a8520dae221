#!/usr/bin/env python3
"""Cost of the robust merge (merge.hip, trimmed_merge_k) next to the mean
merge on the same deltas, at GPT-2-small P: ops.trimmed_merge with trim 1 and
with the median's trim against ops.weighted_merge with uniform W, for
N = 4 / 8 / 16 / 32 deltas stored as fp32, bf16 and int8.

The mean merge is the yardstick because it moves the same bytes; there is no
pass ratio, the robust merge replaces nothing. Device-event times, median
and min over --rounds rounds of --iters calls, the three variants alternated
inside every round. Bytes moved are (N * bytes per stored delta element +
8) * P: every row once, base once, out once. Compare only within one run of
this script.

    python tools/robust_merge_ab.py [--rounds 7] [--iters 3] [--md out.md]
"""
import argparse
import os
import statistics
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)

GPT2_SMALL_P = 124_439_808      # parameters of the flat plane, tied head
BLOCK = 4096
ELEM_BYTES = {"fp32": 4.0, "bf16": 2.0, "int8": 1.0 + 4.0 / BLOCK}


def _time_alternating(fns, rounds, iters, warmup):
    """{name: (median ms, min ms)}; every round times each variant once."""
    import torch
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) / iters)
    return {k: (statistics.median(v), min(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--numel", type=int, default=GPT2_SMALL_P)
    ap.add_argument("--models", type=int, nargs="+", default=[4, 8, 16, 32])
    ap.add_argument("--md", default=None, help="also write the table here")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("robust_merge_ab needs a GPU: nothing is measured without "
                 "one")
    from distributedtraining_amd import ops
    from distributedtraining_amd.parallel.comm import PackedDeltas
    dev = "cuda:0"
    P, n_max = args.numel, max(args.models)
    g = torch.Generator(device=dev).manual_seed(0)
    base = torch.randn(P, device=dev, generator=g)
    out = torch.empty_like(base)
    offsets = torch.tensor([0, P], device=dev)

    dense = torch.empty(n_max, P, device=dev)
    for i in range(n_max):
        dense[i] = torch.randn(P, device=dev, generator=g) * 1e-3
    bf16 = dense.to(torch.bfloat16)
    nb = (P + BLOCK - 1) // BLOCK
    codes = torch.empty(n_max, nb * BLOCK, dtype=torch.int8, device=dev)
    scales = torch.empty(n_max, nb, device=dev)
    for i in range(n_max):
        codes[i], scales[i] = ops.quantize_blockwise_int8(dense[i], BLOCK)

    def stored(kind, n):
        if kind == "fp32":
            return dense[:n]
        if kind == "bf16":
            return PackedDeltas("bf16", bf16[:n], P)
        return PackedDeltas("int8", codes[:n], P, scales[:n], BLOCK)

    lines = [f"device: {torch.cuda.get_device_name(0)}; P={P} int8 block="
             f"{BLOCK}; rounds={args.rounds} iters={args.iters} "
             f"warmup={args.warmup}", "",
             "| N | storage | GB moved | mean merge ms (median / min) | GB/s "
             "| trim 1 ms | GB/s | x mean | median ms | GB/s | x mean |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in args.models:
        W = torch.full((n, 1), 1.0 / n, device=dev)
        for kind in ("fp32", "bf16", "int8"):
            d = stored(kind, n)
            outside = torch.zeros(n, dtype=torch.int64, device=dev)
            t = _time_alternating({
                "mean": lambda: ops.weighted_merge(base, d, W, offsets, out),
                "trim1": lambda: ops.trimmed_merge(base, d, min(1, (n - 1) // 2),
                                                   out, outside),
                "median": lambda: ops.trimmed_merge(
                    base, d, ops.median_trim(n), out, outside),
            }, args.rounds, args.iters, args.warmup)
            nbytes = (n * ELEM_BYTES[kind] + 8) * P
            row = f"| {n} | {kind} | {nbytes / 1e9:.2f} "
            for name in ("mean", "trim1", "median"):
                med, mn = t[name]
                row += f"| {med:.3f} / {mn:.3f} | {nbytes / med / 1e6:.0f} "
                if name != "mean":
                    row += f"| {med / t['mean'][0]:.2f} "
            lines.append(row + "|")
            print(lines[-1], flush=True)
    text = "\n".join(lines)
    print(text)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
