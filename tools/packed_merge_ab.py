#!/usr/bin/env python3
"""A/B of the merge plane on packed deltas (merge.hip) at GPT-2-small P with
N = 8 gathered deltas: weighted_merge and grad_merge_weights on fp32, bf16
and int8 storage, and the fused int8 quantiser against the eager torch chain
of parallel/comm.py run on the same GPU.

Device-event times, median and min over --rounds rounds of --iters calls,
the variants of one op alternated inside every round. GB/s is the bytes the
variant must move (computed from the shapes, below) over the median time.
Compare only within one run of this script. The fp32 rows are the kernels
of before the packed storage existed: their instantiation is unchanged.

    python tools/packed_merge_ab.py [--rounds 7] [--iters 5] [--md out.md]
"""
import argparse
import os
import statistics
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)

GPT2_SMALL_P = 124_439_808      # parameters of the flat plane, tied head
N_MODELS = 8
BLOCK = 4096


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


def delta_bytes(kind, P, block=BLOCK):
    """Bytes of one stored delta row."""
    nb = (P + block - 1) // block
    return {"fp32": 4 * P, "bf16": 2 * P, "int8": nb * block + 4 * nb}[kind]


def merge_bytes(kind, N, P):
    return 4 * P + N * delta_bytes(kind, P) + 4 * P        # base, rows, out


def grad_w_bytes(kind, N, P, g_bytes=2):
    # every (chunk, model) block reads g, base and merged again
    return N * ((g_bytes + 4 + 4) * P + delta_bytes(kind, P))


def quant_bytes(P, fused, block=BLOCK):
    nb = (P + block - 1) // block
    return (8 if fused else 4) * P + nb * block + 4 * nb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--numel", type=int, default=GPT2_SMALL_P)
    ap.add_argument("--models", type=int, default=N_MODELS)
    ap.add_argument("--md", default=None, help="also write the tables here")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("packed_merge_ab needs a GPU: nothing is measured without "
                 "one")
    from distributedtraining_amd import ops
    from distributedtraining_amd.ops.backend import require_ext
    from distributedtraining_amd.parallel import comm
    from distributedtraining_amd.parallel.comm import PackedDeltas
    m = require_ext()
    dev = "cuda:0"
    N, P = args.models, args.numel
    g = torch.Generator(device=dev).manual_seed(0)

    # GPT-2-small-like segment table: 148 tensors of uneven sizes
    S = 148
    cuts = torch.linspace(0, P, S + 1).long()
    cuts[1:-1] += torch.arange(1, S) % 7        # off the vector boundaries
    offsets = cuts.to(dev)
    base = torch.randn(P, device=dev, generator=g)
    W = torch.full((N, S), 1.0 / N, device=dev)
    grad = torch.randn(P, device=dev, generator=g).to(torch.bfloat16)
    packed = {}
    rows = [torch.randn(P, device=dev, generator=g) * 1e-3 for _ in range(N)]
    packed["bf16"] = PackedDeltas(
        "bf16", torch.stack([r.to(torch.bfloat16) for r in rows]), P)
    qs = [ops.quantize_blockwise_int8(r, BLOCK) for r in rows]
    packed["int8"] = PackedDeltas("int8", torch.stack([q for q, _ in qs]), P,
                                  torch.stack([s for _, s in qs]), BLOCK)
    del qs
    dense = torch.stack(rows)                  # the fp32 gather
    w_plane = base + rows[0]
    del rows
    out = torch.empty_like(base)

    # same seeded inputs, same results: packed against fp32 on its own rows
    for kind in ("int8", "bf16"):
        dq = packed[kind].dequantize()
        ref = torch.empty_like(base)
        m.weighted_merge(base, dq, W, offsets, ref)
        got = ops.weighted_merge(base, packed[kind], W, offsets)
        assert torch.equal(got, ref), f"{kind} merge differs from fp32"
        del dq, ref, got
    merged = ops.weighted_merge(base, dense, W, offsets)

    lines = [f"device: {torch.cuda.get_device_name(0)}; N={N} P={P} "
             f"block={BLOCK} segments={S}; rounds={args.rounds} "
             f"iters={args.iters} warmup={args.warmup}", ""]

    def table(title, times, nbytes):
        lines.extend([f"### {title}", "",
                      "| variant | ms (median / min) | bytes moved | GB/s |",
                      "|---|---|---|---|"])
        for name, (med, mn) in times.items():
            b = nbytes[name]
            lines.append(f"| {name} | {med:.3f} / {mn:.3f} | {b / 1e9:.3f} GB"
                         f" | {b / med / 1e6:.0f} |")
        lines.append("")

    t = _time_alternating({
        "fp32": lambda: m.weighted_merge(base, dense, W, offsets, out),
        "bf16": lambda: ops.weighted_merge(base, packed["bf16"], W, offsets,
                                           out),
        "int8": lambda: ops.weighted_merge(base, packed["int8"], W, offsets,
                                           out),
    }, args.rounds, args.iters, args.warmup)
    table("weighted_merge", t, {k: merge_bytes(k, N, P) for k in t})

    t = _time_alternating({
        "fp32": lambda: m.grad_merge_weights(grad, base, dense, merged,
                                             offsets),
        "bf16": lambda: ops.grad_merge_weights(grad, base, packed["bf16"],
                                               merged, offsets),
        "int8": lambda: ops.grad_merge_weights(grad, base, packed["int8"],
                                               merged, offsets),
    }, args.rounds, args.iters, args.warmup)
    table("grad_merge_weights (bf16 g)", t,
          {k: grad_w_bytes(k, N, P) for k in t})

    del dense
    t = _time_alternating({
        "eager torch chain (x)":
            lambda: comm.quantize_blockwise_int8(w_plane, BLOCK),
        "delta_quantize_int8_k (x)":
            lambda: ops.quantize_blockwise_int8(w_plane, BLOCK),
        "delta_sub + eager torch chain (w, base)":
            lambda: comm.quantize_blockwise_int8(
                ops.delta_sub(w_plane, base), BLOCK),
        "delta_quantize_int8_k (w, base)":
            lambda: ops.quantize_blockwise_int8(w_plane, BLOCK, base=base),
    }, args.rounds, args.iters, args.warmup)
    table("int8 quantise of one plane", t,
          {k: quant_bytes(P, "(w, base)" in k) for k in t})

    text = "\n".join(lines)
    print(text)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
