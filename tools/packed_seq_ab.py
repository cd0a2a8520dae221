#!/usr/bin/env python3
"""A/B of packed-sequence training against the plain causal path, the two
variants of every step alternating inside one child process. Each step is a
fresh child with a time limit; the run ends at the first step that fails.

  attn:  attention forward + backward at the validator shape (8,12,12,512,64)
         and the Llama shape (8,32,8,512,128), every row packed with
         --doc-len-token documents, against the plain causal call on the same
         tensors. The masked call walks about doc_len/S of the tiles.
  dwpe:  embedding backward at [1024, 64, 768], packed with about 3 documents
         per row (emb_dwpe_doc_k) against the column-sum path on unpacked
         input.
  mattn: the miner's attention alone, ops.qkv_attention at [1024, 64, 3*768],
         12 heads, dropout 0.1, forward and backward timed apart, packed
         (about 3 documents per row) against plain: where a difference of
         the whole step comes from.
  step:  the flagship miner step (GPT-2 small, batch 1024, seq 64) through
         GraphedMinerStep, packed batches against plain ones.

Device-event times; per variant the median, min and spread (max - min) over
--rounds rounds of --iters calls. Compare only within one run.

    python tools/packed_seq_ab.py [--steps attn dwpe step] [--md out.md]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)

ATTN_SHAPES = {"validator": (8, 12, 12, 512, 64), "llama": (8, 32, 8, 512, 128)}
DWPE = dict(B=1024, S=64, E=768, P=1024, V=50257)
STEP_LIMIT_S = {"attn": 300, "dwpe": 180, "mattn": 180, "step": 420}


def _ab(fns, rounds, iters, warmup):
    """{name: (median, min, spread)} with the variants alternating."""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
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
    return {k: (statistics.median(v), min(v), max(v) - min(v))
            for k, v in out.items()}


def _doc_layout(B, S, doc_len, dev):
    import torch
    s = torch.arange(S, dtype=torch.int32, device=dev)
    return ((s // doc_len) * doc_len).expand(B, S).contiguous()


def child_attn(args):
    import torch
    from distributedtraining_amd import ops
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    res = {}
    for name, (B, H, Hk, S, D) in ATTN_SHAPES.items():
        q = torch.randn(B, H, S, D, device=dev, generator=g).to(
            torch.bfloat16).requires_grad_(True)
        k = torch.randn(B, Hk, S, D, device=dev, generator=g).to(
            torch.bfloat16).requires_grad_(True)
        v = torch.randn(B, Hk, S, D, device=dev, generator=g).to(
            torch.bfloat16).requires_grad_(True)
        do = torch.randn(B, H, S, D, device=dev, generator=g).to(
            torch.bfloat16)
        q_lo = _doc_layout(B, S, args.doc_len, dev)
        k_hi = ops.q_lo_inverse(q_lo)     # once per batch, outside the timing

        def run(q_lo=None, k_hi=None):
            q.grad = k.grad = v.grad = None
            ops.causal_attention(q, k, v, q_lo=q_lo, k_hi=k_hi).backward(do)

        res[name] = _ab({"plain": run,
                         "masked": lambda: run(q_lo, k_hi)},
                        args.rounds, args.iters, args.warmup)
    return res


def child_dwpe(args):
    import torch
    from distributedtraining_amd.ops.backend import require_ext
    m = require_ext()
    dev = "cuda:0"
    B, S, E, P, V = (DWPE[k] for k in "BSEPV")
    g = torch.Generator(device=dev).manual_seed(0)
    dy = torch.randn(B, S, E, device=dev, generator=g).to(torch.bfloat16)
    ids = torch.randint(0, V, (B, S), device=dev, generator=g)
    ds = _random_layout(B, S, torch.Generator().manual_seed(1), dev)
    res = _ab({"colsum": lambda: m.embedding_bwd(dy, ids, V, P),
               "doc": lambda: m.embedding_bwd(dy, ids, V, P, ds)},
              args.rounds, args.iters, args.warmup)
    col = torch.arange(S, dtype=torch.int32, device=dev)
    res["docs_per_row"] = float((ds == col).sum()) / B
    return res


def _random_layout(B, S, g, dev):
    """About 3 documents per row: a start with probability 2/S per column."""
    import torch
    st = torch.rand(B, S, generator=g) < 2.0 / S
    st[:, 0] = True
    col = torch.arange(S, dtype=torch.int32).expand(B, S)
    return torch.cummax(torch.where(st, col, torch.zeros_like(col)),
                        dim=1).values.contiguous().to(dev)


def child_mattn(args):
    import torch
    from distributedtraining_amd import ops
    dev = "cuda:0"
    B, S, H, D, p = args.batch_size, 64, 12, 64, 0.1
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B, S, 3 * H * D, device=dev, generator=g).to(
        torch.bfloat16).requires_grad_(True)
    do = torch.randn(B, S, H * D, device=dev, generator=g).to(torch.bfloat16)
    q_lo = _random_layout(B, S, torch.Generator().manual_seed(1), dev)
    k_hi = ops.q_lo_inverse(q_lo)
    kw = {"plain": {}, "packed": dict(q_lo=q_lo, k_hi=k_hi)}
    outs = {n: ops.qkv_attention(qkv, H, p_drop=p, site=1, **k)
            for n, k in kw.items()}

    def bwd(o):
        qkv.grad = None
        o.backward(do, retain_graph=True)

    def fwd(k):
        with torch.no_grad():
            ops.qkv_attention(qkv, H, p_drop=p, site=1, **k)

    res = {"forward": _ab({n: (lambda k=k: fwd(k)) for n, k in kw.items()},
                          args.rounds, args.iters, args.warmup),
           "backward": _ab({n: (lambda o=o: bwd(o)) for n, o in outs.items()},
                           args.rounds, args.iters, args.warmup)}
    return res


def child_step(args):
    import torch
    from distributedtraining_amd.config import Config, ModelConfig
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.parallel.flat import FlatParams
    from distributedtraining_amd.parallel.graphstep import GraphedMinerStep
    from distributedtraining_amd.roles.miner import DeltaLoop
    from distributedtraining_amd.utils.data import synthetic_batches
    dev = "cuda:0"
    cfg = Config()
    cfg.model = ModelConfig.gpt2_small()
    B, S = args.batch_size, 64
    g = torch.Generator().manual_seed(1)
    pool = []
    src = synthetic_batches(cfg.model.vocab_size, B, S, seed=2)
    for _ in range(4):
        b = {k: t.to(dev) for k, t in next(src).items()}
        b["doc_start"] = _random_layout(B, S, g, dev)
        pool.append(b)
    plain_pool = [{k: t for k, t in b.items() if k != "doc_start"}
                  for b in pool]

    def mk(batches):
        torch.manual_seed(0)
        model = build_model(cfg.model).to(dev)
        miner = DeltaLoop(model, FlatParams(model), iter(()), cfg.train)
        return GraphedMinerStep(miner, batches, warmup=3)

    gp, gd = mk(plain_pool), mk(pool)
    i = [0]

    def step(gs, batches):
        i[0] += 1
        gs.step(batches[i[0] % len(batches)])

    return _ab({"plain": lambda: step(gp, plain_pool),
                "packed": lambda: step(gd, pool)},
               args.rounds, args.iters, args.warmup)


CHILDREN = {"attn": child_attn, "dwpe": child_dwpe, "mattn": child_mattn,
            "step": child_step}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="*", default=list(CHILDREN),
                    choices=list(CHILDREN))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--doc-len", type=int, default=64,
                    help="document length of the attention step")
    ap.add_argument("--batch-size", type=int, default=1024,
                    help="batch of the miner step")
    ap.add_argument("--md", default=None, help="also write the table here")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("AB_RESULT " + json.dumps(CHILDREN[args.child](args)),
              flush=True)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("packed_seq_ab needs a GPU: nothing is measured without one")
    lines = ["| step | case | variant | ms median | ms min | spread |",
             "|---|---|---|---|---|---|"]
    for name in args.steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name,
               "--rounds", str(args.rounds), "--iters", str(args.iters),
               "--warmup", str(args.warmup), "--doc-len", str(args.doc_len),
               "--batch-size", str(args.batch_size)]
        # check=True and the timeout end the run at the first failing step
        out = subprocess.run(cmd, check=True, timeout=STEP_LIMIT_S[name],
                             stdout=subprocess.PIPE, text=True).stdout
        line = [ln for ln in out.splitlines()
                if ln.startswith("AB_RESULT ")][-1]
        res = json.loads(line[len("AB_RESULT "):])
        groups = res if name in ("attn", "mattn") else {"": res}
        for case, r in groups.items():
            for variant, val in r.items():
                if not isinstance(val, list):
                    case = f"{case} {variant}={val:.2f}".strip()
                    continue
            for variant, val in r.items():
                if isinstance(val, list):
                    lines.append(f"| {name} | {case} | {variant} | "
                                 f"{val[0]:.3f} | {val[1]:.3f} | "
                                 f"{val[2]:.3f} |")
    table = "\n".join(lines)
    print(f"device: {torch.cuda.get_device_name(0)}; rounds={args.rounds} "
          f"iters={args.iters} warmup={args.warmup} doc_len={args.doc_len}")
    print(table)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
