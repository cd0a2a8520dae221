#!/usr/bin/env python3
"""A/B of the two fused backward kernels at the flagship shapes, each of the
four DTA_ATTN_BWD_FUSED x DTA_CE_FUSED settings in a fresh child process
(both flags are read once per process).

  attention: ops.qkv_attention backward, packed [1024, 64, 3*768] bf16,
             12 heads, dropout 0.1: attn_bwd_fused_k vs dq + dkv
  CE:        [64512, 50257] bf16 logits: ce_fwd_bwd (in place) vs
             ce_fwd + ce_bwd (second buffer); also the variant of
             ce_fwd_bwd that holds the row in LDS

Device-event times, median and min over --rounds rounds of --iters calls.
Compare only within one run of this script.

    python tools/fused_backward_ab.py [--rounds 7] [--iters 5] [--md out.md]
    python tools/fused_backward_ab.py --ce-rows 512 1024 1335 2048 4096
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)

ATTN = dict(B=1024, S=64, H=12, D=64, p=0.1)
CE = dict(T=1024 * 63, V=50257)


def _time(fn, rounds, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out)


def child(args):
    import torch
    from distributedtraining_amd import ops
    from distributedtraining_amd.ops.backend import require_ext
    m = require_ext()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    res = {"attn_fused": os.environ.get("DTA_ATTN_BWD_FUSED", "1") != "0",
           "ce_fused": ops._CE_FUSED}

    B, S, H, D, p = (ATTN[k] for k in "BSHDp")
    qkv = torch.randn(B, S, 3 * H * D, device=dev, generator=g).to(
        torch.bfloat16).requires_grad_(True)
    do = torch.randn(B, S, H * D, device=dev, generator=g).to(torch.bfloat16)
    o = ops.qkv_attention(qkv, H, p_drop=p, site=1)
    n0 = m.attn_bwd_fused_calls()

    def attn_bwd():
        qkv.grad = None
        o.backward(do, retain_graph=True)

    res["attn_bwd_ms"] = _time(attn_bwd, args.rounds, args.iters, args.warmup)
    res["attn_fused_ran"] = m.attn_bwd_fused_calls() > n0
    del qkv, do, o

    T, V = CE["T"], CE["V"]
    logits = torch.randn(T, V, device=dev, generator=g,
                         dtype=torch.bfloat16).mul_(3.0)
    tgt = torch.randint(0, V, (T,), device=dev, generator=g)
    inv = torch.full((1,), 1.0 / T, device=dev)

    def ce_two():
        _, lse, _ = m.ce_fwd(logits, tgt, -100)
        return m.ce_bwd(logits, tgt, lse, inv, 0.0, -100, 0, True)

    # in place: after the first call the buffer holds gradients, not
    # logits; the kernel's work does not depend on the values
    def ce_one(rows=0):
        m.ce_fwd_bwd(logits, tgt, -100, inv, rows)

    if args.ce_rows:
        res["ce_rows_ms"] = {
            r: _time(lambda r=r: ce_one(r), args.rounds, args.iters,
                     args.warmup) for r in args.ce_rows}
    if ops._CE_FUSED and res["attn_fused"]:
        # the LDS-resident-row variant (binding flag only)
        res["ce_lds_ms"] = _time(
            lambda: m.ce_fwd_bwd(logits, tgt, -100, inv, 0, True),
            args.rounds, args.iters, args.warmup)
    res["ce_ms"] = _time(ce_one if ops._CE_FUSED else ce_two, args.rounds,
                         args.iters, args.warmup)
    print("AB_RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ce-rows", type=int, nargs="*", default=[],
                    help="also time ce_fwd_bwd at these rows-in-flight caps")
    ap.add_argument("--md", default=None, help="also write the table here")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import torch
    if not torch.cuda.is_available():
        sys.exit("fused_backward_ab needs a GPU: nothing is measured "
                 "without one")
    rows = []
    for af in ("1", "0"):
        for cf in ("1", "0"):
            env = dict(os.environ, DTA_ATTN_BWD_FUSED=af, DTA_CE_FUSED=cf)
            cmd = [sys.executable, os.path.abspath(__file__), "--child",
                   "--rounds", str(args.rounds), "--iters", str(args.iters),
                   "--warmup", str(args.warmup)]
            if args.ce_rows and af == "1" and cf == "1":
                cmd += ["--ce-rows"] + [str(r) for r in args.ce_rows]
            out = subprocess.run(cmd, env=env, check=True, timeout=600,
                                 stdout=subprocess.PIPE, text=True).stdout
            line = [ln for ln in out.splitlines()
                    if ln.startswith("AB_RESULT ")][-1]
            rows.append(json.loads(line[len("AB_RESULT "):]))
    lines = ["| DTA_ATTN_BWD_FUSED | DTA_CE_FUSED | attention bwd ms "
             "(median / min) | CE fwd+bwd ms (median / min) |",
             "|---|---|---|---|"]
    for r in rows:
        assert r["attn_fused_ran"] == r["attn_fused"]
        lines.append(f"| {int(r['attn_fused'])} | {int(r['ce_fused'])} | "
                     f"{r['attn_bwd_ms'][0]:.3f} / {r['attn_bwd_ms'][1]:.3f}"
                     f" | {r['ce_ms'][0]:.3f} / {r['ce_ms'][1]:.3f} |")
    for r in rows:
        for cap, (med, mn) in r.get("ce_rows_ms", {}).items():
            lines.append(f"| ce_fwd_bwd, {cap} rows in flight | | | "
                         f"{med:.3f} / {mn:.3f} |")
        if "ce_lds_ms" in r:
            med, mn = r["ce_lds_ms"]
            lines.append(f"| ce_fwd_bwd, row held in LDS | | | "
                         f"{med:.3f} / {mn:.3f} |")
    table = "\n".join(lines)
    print(f"device: {torch.cuda.get_device_name(0)}; rounds={args.rounds} "
          f"iters={args.iters} warmup={args.warmup}")
    print(table)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
