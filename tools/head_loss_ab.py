#!/usr/bin/env python3
"""A/B in ONE process: fused no-logits head loss (ops.lm_head_loss, the
hand-written MFMA GEMM + online CE of hip/head_loss.hip) vs the existing
no-grad path (ops.lm_head_ce: library GEMM -> [T,V] bf16 logits -> ce_fwd).

Both arms see the same random inputs; rounds alternate between the arms and
the table reports median and min of the per-round mean (device events), the
peak allocator rise of one call of each arm, and the loss both arms return.
Compare only within one run: box-to-box spread is about +-4 %
(docs/notes_round3.md).

The library arm gets what the benchmark gives it: TunableOp on, tuned
during the warm-up calls (--no-tune leaves hipBLASLt on its heuristics).

    python tools/head_loss_ab.py [--rounds 7] [--iters 5] [--md out.md]
"""
import argparse
import os
import statistics
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)
if "--no-tune" not in sys.argv:
    os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
    os.environ.setdefault("PYTORCH_TUNABLEOP_TUNING", "1")
    os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME",
                          os.path.join(_root, "tuning", "tunableop.csv"))
    os.environ.setdefault("PYTORCH_TUNABLEOP_VERBOSE", "0")

import torch  # noqa: E402

SHAPES = [
    ("validator 8x511, gpt2", 8 * 511, 768, 50257),
    ("large-batch gpt2 eval", 65536 - 1024, 768, 50257),
    ("llama-3 eval 8x511", 8 * 511, 4096, 128256),
]


def _time_round(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters    # ms per call


def _peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    return rise, float(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-tune", action="store_true",
                    help="library GEMM on heuristics, no TunableOp")
    ap.add_argument("--md", default=None, help="also write the table here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("head_loss_ab needs a GPU: nothing is measured without one")

    from distributedtraining_amd import ops
    from distributedtraining_amd.ops.backend import require_ext
    require_ext()
    dev = "cuda:0"
    rows = []
    for name, T, K, V in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(T, K, device=dev, generator=g).to(torch.bfloat16)
        w = (torch.randn(V, K, device=dev, generator=g) * 0.02).to(
            torch.bfloat16)
        t = torch.randint(0, V, (T,), device=dev, generator=g)

        def fused():
            return ops.lm_head_loss(x, w, t)

        def lib():
            with torch.no_grad():
                return ops.lm_head_ce(x, w, t)[0]

        for _ in range(args.warmup):
            fused()
            lib()
        torch.cuda.synchronize()
        tf, tl = [], []
        for _ in range(args.rounds):       # interleaved rounds
            tf.append(_time_round(fused, args.iters))
            tl.append(_time_round(lib, args.iters))
        pf, lf = _peak_rise(fused)
        pl, ll = _peak_rise(lib)
        tflop = 2.0 * T * K * V / 1e12
        rows.append((name, T, K, V, statistics.median(tf), min(tf),
                     statistics.median(tl), min(tl), pf, pl, lf, ll,
                     tflop / (statistics.median(tf) / 1e3)))
        del x, w, t
        torch.cuda.empty_cache()

    lines = [
        "| shape | T | K | V | fused ms (median / min) | lm_head_ce ms "
        "(median / min) | fused / lib | fused peak MiB | lib peak MiB | "
        "fused TFLOP/s | loss fused / lib |",
        "|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    for (name, T, K, V, fm, fmin, lm, lmin, pf, pl, lf, ll, tfs) in rows:
        lines.append(
            f"| {name} | {T} | {K} | {V} | {fm:.3f} / {fmin:.3f} | "
            f"{lm:.3f} / {lmin:.3f} | {fm / lm:.2f}x | {pf / 2**20:.1f} | "
            f"{pl / 2**20:.1f} | {tfs:.0f} | {lf:.5f} / {ll:.5f} |")
    table = "\n".join(lines)
    print(f"device: {torch.cuda.get_device_name(0)}; rounds={args.rounds} "
          f"iters={args.iters} warmup={args.warmup} "
          f"tunableop={os.environ.get('PYTORCH_TUNABLEOP_ENABLED', '0')}")
    print(table)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
