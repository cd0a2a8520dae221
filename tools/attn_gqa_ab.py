#!/usr/bin/env python3
"""A/B of the GQA attention backward (dq + dk/dv, one ``attn_bwd`` call on
[B,S,heads,D] projection views, as models/llama.py makes it):

  atomic    two fp32 fills + attn_bwd_dkv_k<.,ATOMIC> (one block per query
            head, fp32 atomics) + two casts to bf16: the parent's path
  one-pass  attn_bwd_dkv_gqa_k: one block per KV head walks the group and
            stores bf16 dk/dv                            (hip/attention.hip)

The dq kernel is common to both arms and inside both times. Each shape runs
in a child process with its own time limit, with and without a document
mask of four documents per row. The rounds alternate between the arms in ONE
process; device-event times over --iters calls per round; median / min / max
over --rounds rounds; peak allocated memory of one backward per arm. A shape
belongs in dta_attn_bwd_gqa_wins (hip/dta_kernels.h) only if the atomic
arm's median minus the one-pass median exceeds the atomic arm's own spread
(max - min). Compare only within one run of this script.

    python tools/attn_gqa_ab.py [--rounds 9] [--iters 5] [--md out.md]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)

# B, H, Hk, S, D, note
SHAPES = ((8, 32, 8, 512, 128, "r02's shape"),
          (2, 32, 8, 2048, 128, "packed rows"),
          (256, 32, 8, 64, 128, "the Llama bench row"),
          (8, 14, 2, 512, 64, "grp 7"))
SHAPE_LIMIT_S = 240


def child(args):
    import torch
    from distributedtraining_amd import ops
    from distributedtraining_amd.ops.backend import require_ext
    m = require_ext()
    dev = "cuda:0"
    B, H, Hk, S, D, _note = SHAPES[args.child]
    g = torch.Generator(device=dev).manual_seed(0)

    def proj(heads):   # a projection output viewed as [B,heads,S,D]
        return torch.randn(B, S, heads, D, device=dev, generator=g) \
            .to(torch.bfloat16).transpose(1, 2)

    q, k, v, do = proj(H), proj(Hk), proj(Hk), proj(H)
    scale = 1.0 / math.sqrt(D)
    nokv = torch.empty(0, dtype=torch.int32, device=dev)
    rng = ops.droprng.counter(torch.device(dev))
    out = {}
    for docs in (1, 4):
        q_lo = k_hi = None
        if docs > 1:
            starts = torch.arange(S, device=dev) // (S // docs) * (S // docs)
            q_lo = starts.to(torch.int32).expand(B, S).contiguous()
            k_hi = ops.q_lo_inverse(q_lo)
        o_bshd, lse = m.attn_fwd(q, k, v, scale, nokv, rng, 0, 0.0, q_lo)

        def bwd():
            return m.attn_bwd(do, q, k, v, o_bshd, lse, scale, nokv, rng, 0,
                              0.0, q_lo, k_hi)

        def ev_time():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                bwd()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / args.iters

        arms = (("atomic", False), ("one-pass", True))
        res = {name: dict(ms=[]) for name, _on in arms}
        grads = {}
        for name, on in arms:
            m.attn_gqa.bwd_enable(on)
            for _ in range(args.warmup):
                bwd()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            grads[name] = bwd()
            torch.cuda.synchronize()
            res[name]["peak_mb"] = \
                (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        for _ in range(args.rounds):              # arms alternate per round
            for name, on in arms:
                m.attn_gqa.bwd_enable(on)
                res[name]["ms"].append(ev_time())
        # same inputs, both arms: the largest dk/dv difference, in units of
        # the largest gradient (the arms round at different places)
        for i, t in ((1, "dk"), (2, "dv")):
            a, b = grads["atomic"][i].float(), grads["one-pass"][i].float()
            res["one-pass"][t + "_maxdiff"] = \
                float((a - b).abs().max() / a.abs().max())
        out[f"{docs} doc"] = res
        del grads
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="*",
                    default=list(range(len(SHAPES))))
    ap.add_argument("--md", default=None, help="also write the table here")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        print("AB_RESULT " + json.dumps(child(args)), flush=True)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("attn_gqa_ab needs a GPU: nothing is measured without one")
    head = ["B H Hk S D", "mask", "arm", "median ms", "min", "max",
            "peak MiB", "dk/dv max diff", "verdict"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for i in args.shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(i),
               "--rounds", str(args.rounds), "--iters", str(args.iters),
               "--warmup", str(args.warmup)]
        # check=True and the timeout end the run at the first failing shape
        outp = subprocess.run(cmd, check=True, timeout=SHAPE_LIMIT_S,
                              stdout=subprocess.PIPE, text=True).stdout
        line = [ln for ln in outp.splitlines()
                if ln.startswith("AB_RESULT ")][-1]
        for mask, res in json.loads(line[len("AB_RESULT "):]).items():
            old = res["atomic"]["ms"]
            omed, ospread = statistics.median(old), max(old) - min(old)
            for arm, r in res.items():
                med = statistics.median(r["ms"])
                verdict = diff = ""
                if arm == "one-pass":
                    verdict = ("wins" if omed - med > ospread
                               else "atomic stays")
                    diff = f"{r['dk_maxdiff']:.1e} / {r['dv_maxdiff']:.1e}"
                lines.append(
                    f"| {' '.join(map(str, SHAPES[i][:5]))} | {mask} | {arm} "
                    f"| {med:.4f} | {min(r['ms']):.4f} | {max(r['ms']):.4f} "
                    f"| {r['peak_mb']:.1f} | {diff} | {verdict} |")
    table = "\n".join(lines)
    print(f"device: {torch.cuda.get_device_name(0)}; ms per backward call; "
          f"rounds={args.rounds} iters={args.iters} warmup={args.warmup}")
    print(table)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
