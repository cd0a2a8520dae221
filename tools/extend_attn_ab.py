#!/usr/bin/env python3
"""A/B of extend attention (attn_extend_k, ``ops.extend_attention``): Sq new
queries per head on a prefix of P cached keys, against what the code without
it has to do.

Step ``kernels``: per shape all arms in one process, alternating inside every
repeat; every arm is warmed up, timed with device events around enough calls
for about ``--window`` s, median of ``--repeats``. Arms:
  ext<n>     the kernel with n KV splits: 1, and half, once, twice and four
             times ``ops.extend_split_plan``'s count (in splits >= 128 keys)
  reprefill  ``ops.causal_attention`` over all P + Sq positions (at P = 0 that
             is causal attention on the same shape)
  decode     Sq calls of ``ops.decode_attention``, one per new token
Reported per arm: us per call, and for the ext arms the max abs difference to
the last Sq rows of ``reprefill`` on the seeded inputs. K/V are cycled through
enough copies that a call never finds its cache in the 256 MiB Infinity Cache.
Shapes: verify-like (Sq 4, 8, 16), second turn (Sq 128) and chunked prefill
(Sq 512) at batch 1 for the heads of Llama-3-8B, Qwen2-7B and GPT-2-small.

Step ``e2e``: time and peak memory of prefilling a ``--prompt``-token prompt
on ``--llama-layers`` Llama-3-8B layers plus head, ``prefill_chunk`` 0
against ``--chunk``.

The parent starts one child process per step under its own time limit and
stops at the first step that fails; it never touches the GPU itself.

    python tools/extend_attn_ab.py --out profiles/extend_attention.json
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
CACHE_BYTES = 768 << 20
HEADS = [("llama3-8b", 32, 8, 128), ("qwen2-7b", 28, 4, 128),
         ("gpt2-small", 12, 12, 64)]
# (B, P, Sq)
BPS = [(1, P, Sq) for Sq in (4, 8, 16) for P in (2048, 8192)] \
    + [(1, P, 128) for P in (2048, 8192)] \
    + [(1, P, 512) for P in (0, 2048, 8192)]


def _time_arms(arms, repeats, window_s):
    """arms: {name: fn(i)}. Per arm (median, min, max) over ``repeats`` of the
    mean call time in us; arms alternate inside every repeat."""
    import torch
    iters = {}
    for name, fn in arms.items():          # warm-up, then size the window
        for i in range(2):
            fn(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        per = (time.perf_counter() - t0) / 3
        iters[name] = max(3, min(20000, int(window_s / per)))
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
    for (name, H, Hk, D), (B, P, Sq) in ((h, s) for h in HEADS for s in BPS):
        L = P + Sq
        g = torch.Generator(device=DEV).manual_seed(L + H)

        def randn(*shape):
            return torch.randn(*shape, generator=g, device=DEV,
                               dtype=torch.bfloat16)
        qa, kc, vc = randn(B, H, L, D), randn(B, Hk, L, D), randn(B, Hk, L, D)
        q = qa[:, :, P:]
        nbytes = 2 * B * Hk * L * D * 2
        ncopy = max(1, min(16, -(-CACHE_BYTES // nbytes)))
        ks = [kc] + [kc.clone() for _ in range(ncopy - 1)]
        vs = [vc] + [vc.clone() for _ in range(ncopy - 1)]
        plan = ops.extend_split_plan(B, H, Hk, Sq, P, D, cus)
        cap = max(1, L // 128)
        splits = sorted({1, max(1, plan // 2), plan, min(2 * plan, cap),
                         min(4 * plan, cap)})

        def ext(n):
            return lambda i: ops.extend_attention(
                q, ks[i % ncopy], vs[i % ncopy], P, split_kv=n)

        def reprefill(i):
            return ops.causal_attention(qa, ks[i % ncopy], vs[i % ncopy])

        def decode(i):
            for t in range(Sq):
                ops.decode_attention(q[:, :, t], ks[i % ncopy], vs[i % ncopy],
                                     P + t + 1)
        arms = {**{f"ext{n}": ext(n) for n in splits},
                "reprefill": reprefill, "decode": decode}
        with torch.no_grad():
            ref = reprefill(0)[:, :, P:].transpose(1, 2).float()
            diff = {k: float((fn(0).float() - ref).abs().max())
                    for k, fn in arms.items() if k.startswith("ext")}
            t = _time_arms(arms, args.repeats, args.window)
        for k, (med, lo, hi) in t.items():
            row = dict(shape=name, H=H, Hk=Hk, D=D, B=B, P=P, Sq=Sq, arm=k,
                       plan=plan, copies=ncopy, us=med, us_min=lo, us_max=hi,
                       max_abs_diff=diff.get(k))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del ks, vs, kc, vc, qa, q
        torch.cuda.empty_cache()
    return rows


def step_e2e(args):
    import torch
    from distributedtraining_amd.config import ModelConfig
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.models.generate import _prefill
    cfg = ModelConfig.llama3_8b()
    cfg.n_layer, cfg.n_positions = args.llama_layers, args.prompt + 8
    torch.manual_seed(0)
    with torch.device(DEV):
        model = build_model(cfg).to(torch.bfloat16).eval()
    ids = torch.randint(0, cfg.vocab_size, (1, args.prompt), device=DEV)
    rows, logits = [], {}
    for chunk in (0, args.chunk, 0, args.chunk):     # first pair is warm-up
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            cache = model.new_cache(1, args.prompt + 8, DEV)
            logits[chunk] = _prefill(model, ids, cache, chunk).float()
        torch.cuda.synchronize()
        row = dict(layers=cfg.n_layer, prompt=args.prompt, prefill_chunk=chunk,
                   ms=(time.perf_counter() - t0) * 1e3,
                   peak_mib_over_weights=(torch.cuda.max_memory_allocated()
                                          - base) / 2**20,
                   cache_mib=cache.nbytes() / 2**20)
        del cache
        rows.append(row)
    rows = rows[2:]
    rows.append(dict(logits_max_abs_diff=float(
        (logits[0] - logits[args.chunk]).abs().max()),
        logits_max_abs=float(logits[0].abs().max())))
    for row in rows:
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernels", "e2e"], default=None)
    ap.add_argument("--llama-layers", type=int, default=4)
    ap.add_argument("--prompt", type=int, default=7900)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
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
               "--repeats", str(args.repeats), "--window", str(args.window),
               "--prompt", str(args.prompt), "--chunk", str(args.chunk),
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
