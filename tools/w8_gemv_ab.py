#!/usr/bin/env python3
"""A/B of int8 weight-only serving (hip/w8_gemv.hip) against the bf16 route.

Step ``kernels``: per projection / head shape of GPT-2-small and Llama-3-8B,
at M = 1, 4, 16, the median time of ``m.w8_gemv`` on the packed weight
against what ``ops.linear`` does with the bf16 weight (gemv or the library),
and the effective TB/s on the bytes each side reads. Each arm cycles through
enough copies of its weight that a call never finds it in the 256 MiB
Infinity Cache; the arms alternate inside every repeat.

Step ``decode``: ms/token of cached greedy decode (graph replay), bf16 against
``quantize_for_serving``, and ``torch.cuda.memory_allocated`` of the model
before and after. Llama runs the 8B layer shapes with ``--llama-layers``
layers (weights generated on the device).

The parent starts one child process per step under its own time limit and
stops at the first step that fails; it never touches the GPU itself.

    python tools/w8_gemv_ab.py --out profiles/w8.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)
os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
os.environ.setdefault("PYTORCH_TUNABLEOP_TUNING", "0")
os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME",
                      os.path.join(_root, "tuning", "tunableop.csv"))

DEV = "cuda:0"
SHAPES = [("gpt2 qkv", 2304, 768), ("gpt2 proj", 768, 768),
          ("gpt2 fc", 3072, 768), ("gpt2 mlp-proj", 768, 3072),
          ("gpt2 head", 50257, 768), ("llama q/o", 4096, 4096),
          ("llama k/v", 1024, 4096), ("llama gate/up", 14336, 4096),
          ("llama down", 4096, 14336), ("llama head", 128256, 4096)]
CACHE_BYTES = 768 << 20     # cycle through more than the Infinity Cache holds


def _time_arms(arms, iters, repeats):
    """arms: {name: fn(i)}. Median over repeats of the mean call time (us),
    the arms alternating inside every repeat; device events."""
    import torch
    out = {k: [] for k in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            a.record()
            for i in range(iters):
                fn(i)
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def step_kernels(args):
    import torch
    from distributedtraining_amd import ops
    from distributedtraining_amd.ops.backend import require_ext
    m = require_ext()
    rows = []
    for name, N, K in SHAPES:
        ncopy = max(2, min(64, -(-CACHE_BYTES // (N * K))))
        w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16) * 0.02
        qw = ops.quantize_weight_int8(w)
        ws = [w.clone() for _ in range(ncopy)]
        qs = [(qw.codes.clone(), qw.scales.clone()) for _ in range(ncopy)]
        ns = int(m.w8.nsplit(N, K))
        for M in (1, 4, 16):
            x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
            with torch.no_grad():
                arms = {
                    "bf16": lambda i: ops.linear(x, ws[i % ncopy]),
                    "int8": lambda i: m.w8_gemv(x, *qs[i % ncopy], None, N),
                }
                for fn in arms.values():        # warm-up of both arms
                    for i in range(3):
                        fn(i)
                torch.cuda.synchronize()
                t = _time_arms(arms, iters=max(ncopy, 20), repeats=args.repeats)
            by_bf16 = N * K * 2 + M * (K + N) * 2
            by_int8 = qw.nbytes() + M * (K + N) * 2 \
                + (2 * ns * M * N * 4 if ns > 1 else 0)
            row = dict(shape=name, N=N, K=K, M=M, nsplit=ns, copies=ncopy,
                       bf16_us=t["bf16"][0], bf16_min=t["bf16"][1],
                       bf16_max=t["bf16"][2], int8_us=t["int8"][0],
                       int8_min=t["int8"][1], int8_max=t["int8"][2],
                       bf16_tbs=by_bf16 / t["bf16"][0] / 1e6,
                       int8_tbs=by_int8 / t["int8"][0] / 1e6)
            rows.append(row)
            print(f"{name:14s} M={M:2d} ns={ns:2d} bf16 {row['bf16_us']:8.1f} us "
                  f"({row['bf16_tbs']:.2f} TB/s)  int8 {row['int8_us']:8.1f} us "
                  f"({row['int8_tbs']:.2f} TB/s)  x{row['bf16_us'] / row['int8_us']:.2f}",
                  flush=True)
        del ws, qs, w, qw
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
        for weights in ("bf16", "int8"):
            torch.manual_seed(0)
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            with torch.device(DEV):
                model = build_model(cfg).to(torch.bfloat16).eval()
            mem_bf16 = torch.cuda.memory_allocated() - base
            if weights == "int8":
                quantize_for_serving(model)
            mem = torch.cuda.memory_allocated() - base
            ids = torch.randint(0, cfg.vocab_size, (batch, 16), device=DEV)
            with torch.no_grad():
                cache = model.new_cache(batch, 16 + 8 + args.tokens * 4, DEV,
                                        graphable=True)
                tok = model.prefill(ids, cache).argmax(-1, keepdim=True)
                dec = GraphedDecoder(model, cache, batch, DEV)
                times = []
                for r in range(4):          # first window is warm-up
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.tokens):
                        tok = dec.step(tok).argmax(-1, keepdim=True)
                    torch.cuda.synchronize()
                    times.append((time.perf_counter() - t0) / args.tokens * 1e3)
            row = dict(family=args.family, layers=cfg.n_layer, batch=batch,
                       weights=weights, ms_per_token=statistics.median(times[1:]),
                       ms_min=min(times[1:]), ms_max=max(times[1:]),
                       model_bytes=mem, model_bytes_bf16=mem_bf16)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del model, cache, dec
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
        rows = step_kernels(args) if args.step == "kernels" else step_decode(args)
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
