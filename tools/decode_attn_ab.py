#!/usr/bin/env python3
"""A/B of the two decode-attention routes: one block per query head
(attn_decode_k, ``split_kv=0``) against the split-KV MFMA route
(attn_decode_split_k + attn_decode_combine_k, ``split_kv=n``).

Step ``kernels``: per serving shape, both routes in one process, alternating
inside every repeat; every arm is warmed up, timed with device events around
enough calls for about 0.5 s, median of ``--repeats``. Reported per arm:
us per call, the bytes the algorithm needs (K and V once per KV head,
2 * B * Hk * L * D * 2) over that time, and its share of the 8 TB/s HBM peak
the other profiles use; and the max abs difference between the routes'
outputs on the seeded inputs. The split route runs at 1 split, at the
candidate count clamp(ceil(2 CUs / (B Hk)), 1, L / 256) and at half and twice
that. K/V are cycled through enough copies that a call never finds its cache
in the 256 MiB Infinity Cache.

Step ``e2e``: ms/token of a 256-token graph-replayed greedy decode on
``--llama-layers`` Llama-3-8B layers plus head after a prompt near 7.9k, at
batch 1 and 16: ``split_kv=0`` against what ``ops.decode_split_plan`` picks.

The parent starts one child process per step under its own time limit and
stops at the first step that fails; it never touches the GPU itself.

    python tools/decode_attn_ab.py --out profiles/decode_split.json
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

DEV = "cuda:0"
HBM_PEAK = 8.0e12
CACHE_BYTES = 768 << 20
# (name, H, Hk, D, B, L)
SHAPES = [("llama3-8b", 32, 8, 128, B, L) for B in (1, 16, 64)
          for L in (512, 2048, 8192)] \
    + [("gpt2-small", 12, 12, 64, B, L) for B in (1, 64) for L in (512, 1024)] \
    + [("qwen2-7b", 28, 4, 128, 16, 8192)]


def _time_arms(arms, repeats, window_s=0.5):
    """arms: {name: fn(i)}. Per arm (median, min, max) over ``repeats`` of the
    mean call time in us; arms alternate inside every repeat."""
    import torch
    iters = {}
    for name, fn in arms.items():          # warm-up, then size the window
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(10):
            fn(i)
        torch.cuda.synchronize()
        per = (time.perf_counter() - t0) / 10
        iters[name] = max(20, min(20000, int(window_s / per)))
    out = {k: [] for k in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            a.record()
            for i in range(iters[name]):
                fn(i)
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / iters[name])
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def step_kernels(args):
    import torch
    from distributedtraining_amd import ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = []
    for name, H, Hk, D, B, L in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(L + B)

        def randn(*shape):
            return torch.randn(*shape, generator=g, device=DEV,
                               dtype=torch.bfloat16)
        q = randn(B, H, D)
        nbytes = 2 * B * Hk * L * D * 2
        ncopy = max(1, min(16, -(-CACHE_BYTES // nbytes)))
        kc, vc = randn(B, Hk, L, D), randn(B, Hk, L, D)
        ks = [kc] + [kc.clone() for _ in range(ncopy - 1)]
        vs = [vc] + [vc.clone() for _ in range(ncopy - 1)]
        cand = ops._decode_split_candidate(B, Hk, L, cus)
        splits = sorted({1, max(1, cand // 2), cand,
                         min(2 * cand, max(1, L // 128))})

        def arm(n):
            return lambda i: ops.decode_attention(
                q, ks[i % ncopy], vs[i % ncopy], L, split_kv=n)
        arms = {"head": arm(0), **{f"split{n}": arm(n) for n in splits}}
        with torch.no_grad():
            ref = arms["head"](0).float()
            diff = {k: float((fn(0).float() - ref).abs().max())
                    for k, fn in arms.items() if k != "head"}
            t = _time_arms(arms, args.repeats)
        for k, (med, lo, hi) in t.items():
            row = dict(shape=name, H=H, Hk=Hk, D=D, B=B, L=L, arm=k,
                       candidate=cand, copies=ncopy, us=med, us_min=lo,
                       us_max=hi, tbs=nbytes / med / 1e6,
                       hbm_share=nbytes / (med * 1e-6) / HBM_PEAK,
                       max_abs_diff=diff.get(k))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del ks, vs, kc, vc
        torch.cuda.empty_cache()
    return rows


def step_e2e(args):
    import torch
    from distributedtraining_amd import ops
    from distributedtraining_amd.config import ModelConfig
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.models.generate import GraphedDecoder
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cfg = ModelConfig.llama3_8b()
    prompt, tokens = args.prompt, args.tokens
    cfg.n_layer, cfg.n_positions = args.llama_layers, prompt + 4 * tokens + 8
    torch.manual_seed(0)
    with torch.device(DEV):
        model = build_model(cfg).to(torch.bfloat16).eval()
    rows = []
    for batch in (1, 16):
        ids = torch.randint(0, cfg.vocab_size, (batch, prompt), device=DEV)
        Lmax = prompt + 4 * tokens + 8
        plan = ops.decode_split_plan(batch, cfg.n_head, cfg.n_kv_head, Lmax,
                                     cfg.n_embd // cfg.n_head, cus)
        for split in (0, None):     # the old kernel, the rule
            with torch.no_grad():
                cache = model.new_cache(batch, Lmax, DEV, graphable=True,
                                        split_kv=split)
                tok = model.prefill(ids, cache).argmax(-1, keepdim=True)
                dec = GraphedDecoder(model, cache, batch, DEV)
                times = []
                for r in range(4):          # first window is warm-up
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(tokens):
                        tok = dec.step(tok).argmax(-1, keepdim=True)
                    torch.cuda.synchronize()
                    times.append((time.perf_counter() - t0) / tokens * 1e3)
            row = dict(layers=cfg.n_layer, batch=batch, prompt=prompt,
                       split_kv=split if split is not None else plan,
                       ms_per_token=statistics.median(times[1:]),
                       ms_min=min(times[1:]), ms_max=max(times[1:]))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del cache, dec
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernels", "e2e"], default=None)
    ap.add_argument("--llama-layers", type=int, default=4)
    ap.add_argument("--prompt", type=int, default=7900)
    ap.add_argument("--tokens", type=int, default=64,
                    help="tokens per timed window (4 windows: 256 tokens)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "this measurement needs a GPU"
        rows = step_kernels(args) if args.step == "kernels" else step_e2e(args)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(rows, f, indent=1)
        return 0
    for step in ("kernels", "e2e"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step,
               "--tokens", str(args.tokens), "--repeats", str(args.repeats),
               "--prompt", str(args.prompt),
               "--llama-layers", str(args.llama_layers)]
        if args.out:
            stem, ext = os.path.splitext(args.out)
            cmd += ["--out", f"{stem}_{step}{ext or '.json'}"]
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
