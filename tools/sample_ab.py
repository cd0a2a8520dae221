#!/usr/bin/env python3
"""A/B of the fused token sampler (hip/sample.hip) against the torch sampling
chain of ``generate`` (``seed=None``: _sample + per-token host sync).

Step ``decode``: ms/token of cached generation, same process, same model,
``seed=None`` and ``seed=0`` alternating inside every repeat, for
``temperature=0.8, top_k=50, top_p=0.9`` and for ``top_p`` alone. GPT-2-small
at batch 1 and 64; Llama-3-8B layer shapes with ``--llama-layers`` layers
(V = 128256) at batch 1 and 16. The figure is the whole ``generate`` call
(prefill, graph capture and all) over the tokens it made.

Step ``kernel``: the sampling launch alone on logits of the same shapes,
device events around back-to-back launches.

The parent starts one child process per step under its own time limit and
stops at the first step that fails; it never touches the GPU itself.

    python tools/sample_ab.py --out profiles/sample.json
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
SETTINGS = [dict(temperature=0.8, top_k=50, top_p=0.9),
            dict(temperature=1.0, top_k=0, top_p=0.9)]


def step_kernel(args):
    import torch
    from distributedtraining_amd import ops
    rows = []
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
    for V, B in ((50257, 1), (50257, 64), (128256, 1), (128256, 16)):
        logits = (3 * torch.randn(B, V, device=DEV)).bfloat16()
        tok = torch.zeros(B, dtype=torch.long, device=DEV)
        for s in SETTINGS + [dict(temperature=1.0, top_k=0, top_p=0.0)]:
            fn = lambda: ops.sample_tokens(  # noqa: E731
                logits, s["temperature"], s["top_k"], s["top_p"], ctr, tok=tok)
            for _ in range(5):
                fn()
            ts = []
            for _ in range(args.repeats):
                a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                a.record()
                for _ in range(50):
                    fn()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b) * 1e3 / 50)
            row = dict(V=V, batch=B, **s, us=statistics.median(ts),
                       us_min=min(ts), us_max=max(ts))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def step_decode(args):
    import torch
    from distributedtraining_amd.config import ModelConfig
    from distributedtraining_amd.models import build_model, generate
    if args.family == "gpt2":
        cfg, batches = ModelConfig.gpt2_small(), (1, 64)
    else:
        cfg, batches = ModelConfig.llama3_8b(), (1, 16)
        cfg.n_layer, cfg.n_positions = args.llama_layers, 512
    torch.manual_seed(0)
    with torch.device(DEV):
        model = build_model(cfg).to(torch.bfloat16).eval()
    rows = []
    for batch in batches:
        ids = torch.randint(0, cfg.vocab_size, (batch, 16), device=DEV)
        for s in SETTINGS:
            times = {"torch": [], "fused": []}
            for r in range(args.repeats + 1):      # first repeat is warm-up
                for arm, seed in (("torch", None), ("fused", 0)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = generate(model, ids, args.tokens, use_cache=True,
                                   seed=seed, **s)
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) * 1e3
                    if r:
                        times[arm].append(dt / (out.shape[1] - 16))
            row = dict(family=args.family, layers=cfg.n_layer, batch=batch,
                       tokens=args.tokens, **s)
            for arm, v in times.items():
                row[arm + "_ms"] = statistics.median(v)
                row[arm + "_min"], row[arm + "_max"] = min(v), max(v)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel", "decode"], default=None)
    ap.add_argument("--family", choices=["gpt2", "llama"], default="gpt2")
    ap.add_argument("--llama-layers", type=int, default=4)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "this measurement needs a GPU"
        rows = step_kernel(args) if args.step == "kernel" else step_decode(args)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(rows, f, indent=1)
        return 0
    steps = [("kernel", []), ("decode", ["--family", "gpt2"]),
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
