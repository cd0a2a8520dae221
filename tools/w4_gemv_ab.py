#!/usr/bin/env python3
"""A/B of int4 weight-only serving (hip/w4_gemv.hip) against the int8 and
bf16 routes, in the manner of tools/w8_gemv_ab.py (whose shape table, timer
and cache-rotation rule it imports).

Step ``kernels``: per projection / head shape of GPT-2-small and Llama-3-8B,
at M = 1, 4, 16, the median time of ``m.w4_gemv`` and ``m.w8_gemv`` on the
packed weights and of ``ops.linear`` on the bf16 weight, with the effective
TB/s on the bytes each arm reads. Each arm cycles through enough copies of its
weight that a call never finds it in the 256 MiB Infinity Cache; the three
arms alternate inside every repeat (median of ``--repeats``, min-max kept).

Step ``decode``: ms/token of cached greedy decode (graph replay) with bf16,
int8 and int4 weights, and ``torch.cuda.memory_allocated`` of the model.
Llama runs the 8B layer shapes with ``--llama-layers`` layers.

The parent starts one child process per step under its own time limit and
stops at the first step that fails; it never touches the GPU itself.

    python tools/w4_gemv_ab.py --out profiles/w4.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from w8_gemv_ab import CACHE_BYTES, DEV, SHAPES, _time_arms  # noqa: E402

ARMS = ("bf16", "int8", "int4")


def step_kernels(args):
    import torch
    from distributedtraining_amd import ops
    from distributedtraining_amd.ops.backend import require_ext
    m = require_ext()
    rows = []
    for name, N, K in SHAPES:
        # the smallest arm (int4, N K / 2 bytes) sets the number of copies
        ncopy = max(2, min(64, -(-CACHE_BYTES // (N * K // 2))))
        nbf = max(2, min(ncopy, -(-CACHE_BYTES // (N * K * 2))))
        w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16) * 0.02
        q8, q4 = ops.quantize_weight_int8(w), ops.quantize_weight_int4(w)
        ws = [w.clone() for _ in range(nbf)]
        n8 = max(2, min(ncopy, -(-CACHE_BYTES // (N * K))))
        q8s = [(q8.codes.clone(), q8.scales.clone()) for _ in range(n8)]
        q4s = [(q4.codes.clone(), q4.scales.clone()) for _ in range(ncopy)]
        ns = {"int8": int(m.w8.nsplit(N, K)), "int4": int(m.w4.nsplit(N, K))}
        for M in (1, 4, 16):
            x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
            with torch.no_grad():
                arms = {
                    "bf16": lambda i: ops.linear(x, ws[i % nbf]),
                    "int8": lambda i: m.w8_gemv(x, *q8s[i % n8], None, N),
                    "int4": lambda i: m.w4_gemv(x, *q4s[i % ncopy], None, N),
                }
                for fn in arms.values():        # warm-up of every arm
                    for i in range(3):
                        fn(i)
                torch.cuda.synchronize()
                t = _time_arms(arms, iters=max(ncopy, 20),
                               repeats=args.repeats)
            io = M * (K + N) * 2
            nbytes = {"bf16": N * K * 2 + io}
            for a, qw in (("int8", q8), ("int4", q4)):
                part = 2 * ns[a] * M * N * 4 if ns[a] > 1 else 0
                nbytes[a] = qw.nbytes() + io + part
            row = dict(shape=name, N=N, K=K, M=M, nsplit8=ns["int8"],
                       nsplit4=ns["int4"], copies=ncopy)
            for a in ARMS:
                row[f"{a}_us"], row[f"{a}_min"], row[f"{a}_max"] = t[a]
                row[f"{a}_tbs"] = nbytes[a] / t[a][0] / 1e6
            rows.append(row)
            print(f"{name:14s} M={M:2d} ns8={ns['int8']:2d} ns4={ns['int4']:2d} "
                  + "  ".join(f"{a} {row[a + '_us']:7.1f} us "
                              f"({row[a + '_tbs']:.2f} TB/s)" for a in ARMS)
                  + f"  int8/int4 x{row['int8_us'] / row['int4_us']:.2f}",
                  flush=True)
        del ws, q8s, q4s, w, q8, q4
        torch.cuda.empty_cache()
    return rows


def step_decode(args):
    import torch
    from distributedtraining_amd.config import ModelConfig
    from distributedtraining_amd.models import (build_model,
                                                quantize_for_serving)
    from distributedtraining_amd.models.generate import GraphedDecoder
    if args.family == "gpt2":
        cfg = ModelConfig.gpt2_small()
    else:
        cfg = ModelConfig.llama3_8b()
        cfg.n_layer, cfg.n_positions = args.llama_layers, 512
    rows = []
    for batch in (1, 4, 16):
        # every arm alive at once, so the timing windows can alternate
        decs, mem = {}, {}
        toks = {}
        for weights in ARMS:
            torch.manual_seed(0)
            base = torch.cuda.memory_allocated()
            with torch.device(DEV):
                model = build_model(cfg).to(torch.bfloat16).eval()
            if weights != "bf16":
                quantize_for_serving(model, weights=weights)
            torch.cuda.empty_cache()
            mem[weights] = torch.cuda.memory_allocated() - base
            ids = torch.randint(0, cfg.vocab_size, (batch, 16), device=DEV)
            with torch.no_grad():
                cache = model.new_cache(batch, 16 + 8 + args.tokens * 6, DEV,
                                        graphable=True)
                toks[weights] = model.prefill(ids, cache).argmax(
                    -1, keepdim=True)
                decs[weights] = GraphedDecoder(model, cache, batch, DEV)
        times = {a: [] for a in ARMS}
        with torch.no_grad():
            for r in range(args.repeats + 1):   # first window is warm-up
                for a in ARMS:
                    dec, tok = decs[a], toks[a]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.tokens):
                        tok = dec.step(tok).argmax(-1, keepdim=True)
                    torch.cuda.synchronize()
                    toks[a] = tok
                    times[a].append(
                        (time.perf_counter() - t0) / args.tokens * 1e3)
        for a in ARMS:
            row = dict(family=args.family, layers=cfg.n_layer, batch=batch,
                       weights=a, ms_per_token=statistics.median(times[a][1:]),
                       ms_min=min(times[a][1:]), ms_max=max(times[a][1:]),
                       model_bytes=mem[a])
            rows.append(row)
            print(json.dumps(row), flush=True)
        del decs, toks
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernels", "decode"], default=None)
    ap.add_argument("--family", choices=["gpt2", "llama"], default="gpt2")
    ap.add_argument("--llama-layers", type=int, default=4)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "this measurement needs a GPU"
        rows = (step_kernels(args) if args.step == "kernels"
                else step_decode(args))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(rows, f, indent=1)
        return 0
    # parent: one child per step, each under its own limit, stop on failure
    steps = [("kernels", []), ("decode", ["--family", "gpt2"]),
             ("decode", ["--family", "llama"])]
    for i, (step, extra) in enumerate(steps):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step,
               "--tokens", str(args.tokens), "--repeats", str(args.repeats),
               "--llama-layers", str(args.llama_layers)] + extra
        if args.out:
            stem, ext = os.path.splitext(args.out)
            cmd += ["--out", f"{stem}_{step}{i}{ext or '.json'}"]
        print("==", " ".join(cmd[2:]), flush=True)
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"step {step} exceeded {args.step_timeout} s; stopping")
            return 124
        if rc != 0:
            print(f"step {step} failed with {rc}; stopping")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
