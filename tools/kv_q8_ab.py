#!/usr/bin/env python3
"""A/B of the int8 KV cache against the bf16 one on the split-KV decode route
(attn_decode_split_q8_k against attn_decode_split_k, both finished by
attn_decode_combine_k).

Step ``kernels``: the serving shapes of tools/decode_attn_ab.py, both formats
in one process, alternating inside every repeat (its ``_time_arms``: warm-up,
device events around about ``--window`` s of calls, median of ``--repeats``).
The bf16 arm runs the split count of ``ops.decode_split_plan``; the int8 arm
runs 1, that count, and half, once and twice ``ops.decode_split_plan_q8``.
Reported per arm: us per call, the bytes the arm's format needs (K and V once per KV head: 2 B Hk L D
times 2 for bf16, times 1 plus 8 B of scales per key for int8) over that time,
the share of the 8 TB/s HBM peak, and for int8 the max abs difference to the
bf16 output (the quantisation error of seeded randn caches, not a kernel
error: tests/test_kv_q8_gpu.py bounds that). The caches are cycled through
enough copies that a call never finds them in the 256 MiB Infinity Cache.

Step ``e2e``: ms/token of a graph-replayed greedy decode on ``--llama-layers``
Llama-3-8B layers plus head after a ``--prompt``-token prefill, batch 1 and 16,
bf16 cache against int8 cache (each on its rule's split count), the two
decoders alternating window by window; and the bytes of both caches.

The parent starts one child process per step under its own time limit and
stops at the first step that fails; it never touches the GPU itself.

    python tools/kv_q8_ab.py --out profiles/kv_q8.json
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
sys.path.insert(0, os.path.join(_root, "tools"))

from decode_attn_ab import CACHE_BYTES, DEV, HBM_PEAK, SHAPES, _time_arms  # noqa: E402


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
        keys = 2 * B * Hk * L
        nbytes = {"bf16": keys * D * 2, "int8": keys * (D + 4)}
        ncopy = max(1, min(16, -(-CACHE_BYTES // nbytes["bf16"])))
        kc, vc = randn(B, Hk, L, D), randn(B, Hk, L, D)
        pad = ops.kv_scale_len(L) - L
        kq, ksc = ops.kv_quantize(kc)
        vq, vsc = ops.kv_quantize(vc)
        ksc, vsc = (torch.nn.functional.pad(t, (0, pad), value=1.0)
                    for t in (ksc, vsc))
        bf = [(kc, vc)] + [(kc.clone(), vc.clone()) for _ in range(ncopy - 1)]
        q8 = [(kq, vq, ksc, vsc)] + [tuple(t.clone() for t in
                                           (kq, vq, ksc, vsc))
                                     for _ in range(ncopy - 1)]
        rule = max(1, ops.decode_split_plan(B, H, Hk, L, D, cus))
        rule8 = ops.decode_split_plan_q8(B, H, Hk, L, D, cus)
        splits = sorted({1, rule, max(1, rule8 // 2), rule8,
                         min(2 * rule8, max(1, L // 128))})

        def arm_bf(i):
            k, v = bf[i % ncopy]
            return ops.decode_attention(q, k, v, L, split_kv=rule)

        def arm_q8(n):
            def fn(i):
                k, v, s, t = q8[i % ncopy]
                return ops.decode_attention(q, k, v, L, split_kv=n,
                                            k_scale=s, v_scale=t)
            return fn
        arms = {"bf16": arm_bf, **{f"int8/{n}": arm_q8(n) for n in splits}}
        with torch.no_grad():
            ref = arm_bf(0).float()
            diff = {k: float((fn(0).float() - ref).abs().max())
                    for k, fn in arms.items() if k != "bf16"}
            t = _time_arms(arms, args.repeats, args.window)
        for k, (med, lo, hi) in t.items():
            need = nbytes[k.split("/")[0]]
            row = dict(shape=name, H=H, Hk=Hk, D=D, B=B, L=L, arm=k,
                       rule=rule, rule_int8=rule8, copies=ncopy, us=med,
                       us_min=lo, us_max=hi,
                       bytes=need, tbs=need / med / 1e6,
                       hbm_share=need / (med * 1e-6) / HBM_PEAK,
                       speedup=t["bf16"][0] / med,
                       max_abs_diff=diff.get(k))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del bf, q8, kc, vc, kq, vq
        torch.cuda.empty_cache()
    return rows


def step_e2e(args):
    import torch
    from distributedtraining_amd.config import ModelConfig
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.models.generate import GraphedDecoder
    cfg = ModelConfig.llama3_8b()
    prompt, tokens = args.prompt, args.tokens
    Lmax = prompt + 4 * tokens + 8
    cfg.n_layer, cfg.n_positions = args.llama_layers, Lmax
    torch.manual_seed(0)
    with torch.device(DEV):
        model = build_model(cfg).to(torch.bfloat16).eval()
    rows = []
    for batch in (1, 16):
        ids = torch.randint(0, cfg.vocab_size, (batch, prompt), device=DEV)
        arms = {}
        with torch.no_grad():
            for fmt in ("bf16", "int8"):
                cache = model.new_cache(batch, Lmax, DEV, graphable=True,
                                        kv_dtype=fmt)
                tok = model.prefill(ids, cache).argmax(-1, keepdim=True)
                arms[fmt] = [GraphedDecoder(model, cache, batch, DEV), tok,
                             cache.nbytes(), []]
            for r in range(4):              # first window is warm-up
                for fmt, arm in arms.items():
                    dec, tok = arm[0], arm[1]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(tokens):
                        tok = dec.step(tok).argmax(-1, keepdim=True)
                    torch.cuda.synchronize()
                    arm[1] = tok
                    arm[3].append((time.perf_counter() - t0) / tokens * 1e3)
        for fmt, (_, _, nbytes, times) in arms.items():
            row = dict(layers=cfg.n_layer, batch=batch, prompt=prompt,
                       kv=fmt, cache_bytes=nbytes,
                       cache_bytes_32_layers=nbytes // cfg.n_layer * 32,
                       ms_per_token=statistics.median(times[1:]),
                       ms_min=min(times[1:]), ms_max=max(times[1:]))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del arms, cache
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
    ap.add_argument("--window", type=float, default=0.3,
                    help="seconds of calls per arm and repeat")
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
               "--window", str(args.window), "--prompt", str(args.prompt),
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
