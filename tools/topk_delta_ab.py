#!/usr/bin/env python3
"""A/B of top-k sparse deltas (merge.hip) at GPT-2-small P with N = 8
gathered deltas: the compressor against the int8 quantiser, and
weighted_merge, grad_merge_weights and axpy_ on "topk" storage against the
int8 and fp32 instantiations, all in one run.

Device-event times, median and min over --rounds rounds of --iters calls,
the variants of one op alternated inside every round. Bytes moved are
computed from the shapes (below), GB/s is those bytes over the median time.
Compare only within one run of this script.

    python tools/topk_delta_ab.py [--k 128] [--block 4096] [--md out.md]
"""
import argparse
import os
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from packed_merge_ab import (GPT2_SMALL_P, N_MODELS, _time_alternating,  # noqa: E402
                             delta_bytes, grad_w_bytes, merge_bytes,
                             quant_bytes)

INT8_BLOCK = 4096


def topk_row_bytes(P, k, block):
    return (P + block - 1) // block * k * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--numel", type=int, default=GPT2_SMALL_P)
    ap.add_argument("--models", type=int, default=N_MODELS)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--block", type=int, default=4096)
    ap.add_argument("--md", default=None, help="also write the tables here")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("topk_delta_ab needs a GPU: nothing is measured without one")
    from distributedtraining_amd import ops
    from distributedtraining_amd.ops.backend import require_ext
    from distributedtraining_amd.parallel.comm import PackedDeltas
    m = require_ext()
    dev = "cuda:0"
    N, P, k, block = args.models, args.numel, args.k, args.block
    g = torch.Generator(device=dev).manual_seed(0)

    S = 148                      # GPT-2-small-like table of uneven segments
    cuts = torch.linspace(0, P, S + 1).long()
    cuts[1:-1] += torch.arange(1, S) % 7
    offsets = cuts.to(dev)
    base = torch.randn(P, device=dev, generator=g)
    W = torch.full((N, S), 1.0 / N, device=dev)
    grad = torch.randn(P, device=dev, generator=g).to(torch.bfloat16)
    rows = [torch.randn(P, device=dev, generator=g) * 1e-3 for _ in range(N)]
    qs = [ops.quantize_blockwise_int8(r, INT8_BLOCK) for r in rows]
    int8 = PackedDeltas("int8", torch.stack([q for q, _ in qs]), P,
                        torch.stack([s for _, s in qs]), INT8_BLOCK)
    del qs
    topk = PackedDeltas("topk", torch.stack(
        [ops.topk_compress_blockwise(r, k, block, update_residual=False)[0]
         for r in rows]), P, None, block, k)
    dense = torch.stack(rows)
    w_plane = base + rows[0]
    residual = torch.randn(P, device=dev, generator=g) * 1e-4
    del rows
    out = torch.empty_like(base)

    # the sparse kernels against fp32 on the densified rows, at this size
    dq = topk.dequantize()
    ref = ops.weighted_merge(base, dq, W, offsets)
    assert torch.equal(ops.weighted_merge(base, topk, W, offsets), ref)
    gw = ops.grad_merge_weights(grad, base, dq, ref, offsets)
    gw_t = ops.grad_merge_weights(grad, base, topk, ref, offsets)
    # segments of more than 2^20 elements are summed by several blocks with
    # one float atomic each: equal up to that order, here as in the fp32 path
    assert torch.allclose(gw_t, gw, rtol=1e-4, atol=1e-6)
    del dq, ref, gw, gw_t
    merged = ops.weighted_merge(base, dense, W, offsets)

    lines = [f"device: {torch.cuda.get_device_name(0)}; N={N} P={P} "
             f"topk k={k} block={block}, int8 block={INT8_BLOCK}, "
             f"segments={S}; rounds={args.rounds} iters={args.iters} "
             f"warmup={args.warmup}", "",
             f"stored row: fp32 {4 * P / 1e6:.1f} MB, int8 "
             f"{delta_bytes('int8', P) / 1e6:.1f} MB, topk "
             f"{topk_row_bytes(P, k, block) / 1e6:.1f} MB", ""]

    def table(title, times, nbytes):
        lines.extend([f"### {title}", "",
                      "| variant | ms (median / min) | bytes moved | GB/s |",
                      "|---|---|---|---|"])
        for name, (med, mn) in times.items():
            b = nbytes[name]
            lines.append(f"| {name} | {med:.3f} / {mn:.3f} | {b / 1e9:.3f} GB"
                         f" | {b / med / 1e6:.0f} |")
        lines.append("")

    tb = topk_row_bytes(P, k, block)
    t = _time_alternating({
        "delta_quantize_int8_k (w, base)":
            lambda: ops.quantize_blockwise_int8(w_plane, INT8_BLOCK,
                                                base=base),
        "delta_topk_k (w, base), no residual":
            lambda: ops.topk_compress_blockwise(w_plane, k, block, base=base,
                                                update_residual=False),
        "delta_topk_k (w, base, residual in and out)":
            lambda: ops.topk_compress_blockwise(w_plane, k, block, base=base,
                                                residual=residual),
    }, args.rounds, args.iters, args.warmup)
    table("compress one plane", t, {
        "delta_quantize_int8_k (w, base)": quant_bytes(P, True, INT8_BLOCK),
        "delta_topk_k (w, base), no residual": 8 * P + tb,
        "delta_topk_k (w, base, residual in and out)": 16 * P + tb})

    t = _time_alternating({
        "fp32": lambda: m.weighted_merge(base, dense, W, offsets, out),
        "int8": lambda: ops.weighted_merge(base, int8, W, offsets, out),
        "topk": lambda: ops.weighted_merge(base, topk, W, offsets, out),
    }, args.rounds, args.iters, args.warmup)
    table("weighted_merge", t, {
        "fp32": merge_bytes("fp32", N, P), "int8": merge_bytes("int8", N, P),
        "topk": 8 * P + N * tb})

    t = _time_alternating({
        "fp32": lambda: m.grad_merge_weights(grad, base, dense, merged,
                                             offsets),
        "int8": lambda: ops.grad_merge_weights(grad, base, int8, merged,
                                               offsets),
        "topk": lambda: ops.grad_merge_weights(grad, base, topk, merged,
                                               offsets),
    }, args.rounds, args.iters, args.warmup)
    table("grad_merge_weights (bf16 g)", t, {
        "fp32": grad_w_bytes("fp32", N, P), "int8": grad_w_bytes("int8", N, P),
        "topk": N * (10 * P + tb)})

    w = base.clone()
    t = _time_alternating({
        "fp32 row": lambda: ops.axpy_(w, dense[1], 1.0),
        "int8 row": lambda: ops.axpy_(w, (int8, 1), 1.0),
        "topk row": lambda: ops.axpy_(w, (topk, 1), 1.0),
    }, args.rounds, args.iters, args.warmup)
    # the scatter reads and writes one 4 B element per entry (the memory
    # system moves a whole sector for each: not counted here)
    table("axpy_ of one row", t, {
        "fp32 row": 12 * P, "int8 row": 8 * P + delta_bytes("int8", P),
        "topk row": 3 * tb})

    text = "\n".join(lines)
    print(text)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
