#!/usr/bin/env python3
"""Compare two `bench.py --dump-outputs` directories per parameter class.

The dump holds a seeded sample of the flat planes (bench.dump_outputs); this
maps every sampled element back to its parameter through FlatParams.spec
and counts, per class (Linear weights, wte/wpe, Linear biases, norm γ/β),
the elements of params.npy and adam_m.npy that differ, the largest
difference, and how many adam_m differences exceed 0.1 x one bf16 ulp of the
gradient (adam_m is 0.1 x the bf16 gradient after the dump's single fresh
step). --offenders also says, per class, how large the gradients of the
elements beyond one ulp are against the class's rms gradient.

    python tools/dump_diff_by_param.py REF_DIR DIR [DIR ...] [--model gpt2-small]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLASSES = ("Linear weights", "wte, wpe", "Linear biases", "norm γ/β")


def classes_of_sample(model_name):
    """int8 class id of every dumped element."""
    import bench
    from distributedtraining_amd.config import ModelConfig
    from distributedtraining_amd.models import build_model
    cfg = getattr(ModelConfig, model_name.replace("-", "_"))()
    with torch.device("meta"):
        model = build_model(cfg)
    seen, cls = set(), []
    for name, p in model.named_parameters():
        if id(p) in seen:          # tied parameters: FlatParams keeps one
            continue
        seen.add(id(p))
        leaf = name.rsplit(".", 1)[-1]
        if p.dim() >= 2:
            c = 1 if leaf in ("wte", "wpe", "embed_tokens") else 0
        else:
            c = 3 if "ln" in leaf or "norm" in leaf else 2
        cls.append(torch.full((p.numel(),), c, dtype=torch.int8))
    cls = torch.cat(cls)
    if cls.numel() > bench.DUMP_MAX_ELEMS:
        g = torch.Generator().manual_seed(20240521)
        idx = torch.randint(0, cls.numel(), (bench.DUMP_MAX_ELEMS,),
                            generator=g).sort().values
        cls = cls[idx]
    return cls.numpy()


def bf16_ulp(v):
    a = np.abs(v).astype(np.float32)
    e = np.floor(np.log2(np.maximum(a, np.float32(2.0 ** -126))))
    return np.exp2(e - 7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ref")
    ap.add_argument("dirs", nargs="+")
    ap.add_argument("--model", default="gpt2-small")
    ap.add_argument("--offenders", action="store_true",
                    help="size of the gradients beyond one bf16 ulp")
    a = ap.parse_args()
    cls = classes_of_sample(a.model)
    ref = {n: np.load(os.path.join(a.ref, n + ".npy"))
           for n in ("params", "adam_m", "loss")}
    assert ref["params"].shape == cls.shape, (ref["params"].shape, cls.shape)
    print("| run | class (sampled elements) | params differ / max | "
          "adam_m differ / max | adam_m beyond 0.1 bf16 ulp of the gradient |")
    print("|---|---|---|---|---|")
    for d in a.dirs:
        cur = {n: np.load(os.path.join(d, n + ".npy"))
               for n in ("params", "adam_m", "loss")}
        for c, cname in enumerate(CLASSES):
            sel = cls == c
            dp = np.abs(cur["params"][sel] - ref["params"][sel])
            dm = np.abs(cur["adam_m"][sel] - ref["adam_m"][sel])
            grad = ref["adam_m"][sel] / np.float32(0.1)
            # 1.01: adam_m = fp32(0.1) * g is itself rounded
            beyond = dm > 0.1 * 1.01 * bf16_ulp(grad)
            over = int(beyond.sum())
            print(f"| {d} | {cname} ({int(sel.sum())}) | "
                  f"{int((dp != 0).sum())} / {dp.max(initial=0):.3g} | "
                  f"{int((dm != 0).sum())} / {dm.max(initial=0):.3g} | {over} |")
            if a.offenders and over:
                rms = float(np.sqrt(np.mean(grad.astype(np.float64) ** 2)))
                rel = np.abs(grad[beyond]) / rms
                ulps = dm[beyond] / (0.1 * bf16_ulp(grad[beyond]))
                print(f"| {d} | {cname}: |g| / rms |g| of the {over} beyond "
                      f"one ulp | median {np.median(rel):.3g} | max "
                      f"{rel.max():.3g} | ulps: median {np.median(ulps):.3g} "
                      f"max {ulps.max():.3g} |")
        print(f"| {d} | loss abs diff | "
              f"{abs(float(cur['loss'][0] - ref['loss'][0])):.3g} | | |")


if __name__ == "__main__":
    main()
