#!/usr/bin/env python3
"""Where the weight-gradient kernel (hip/wgrad.hip) and the library GEMM give
different bf16 results, which of the two is closer to an fp64 product?

T = 65536, dy 0.05 randn, x 0.5 randn, zero destination, one shape per call.
Counts the elements that differ, those that differ by more than one bf16 ulp
of the library's value, how small those sums are against the root-sum-square
of their 65536 terms, and the error of either result against fp64 - source of
the second table of section 4 in profiles/r10_wgrad.md.

    python tools/wgrad_vs_fp64.py OUT IN        # e.g. 3072 768
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributedtraining_amd.ops.backend import require_ext
m = require_ext()
dev = "cuda:0"
g = torch.Generator(device=dev).manual_seed(1)
T, out, inp = 65536, int(sys.argv[1]), int(sys.argv[2])
print(f"== shape T={T} out={out} in={inp}, splits {m.wgrad.nsplit(T, out, inp)}")
dy = (torch.randn(T, out, device=dev, generator=g) * 0.05).to(torch.bfloat16)
x = (torch.randn(T, inp, device=dev, generator=g) * 0.5).to(torch.bfloat16)
k = torch.zeros(out, inp, dtype=torch.bfloat16, device=dev)
l = torch.zeros_like(k)
m.wgrad.bias(dy, x, k)
l.addmm_(dy.t(), x)
ex = torch.zeros(out, inp, dtype=torch.float64, device=dev)
sq = torch.zeros(out, inp, dtype=torch.float64, device=dev)
for t0 in range(0, T, 8192):
    a, b = dy[t0:t0 + 8192].double(), x[t0:t0 + 8192].double()
    ex += a.t() @ b
    sq += (a * a).t() @ (b * b)
size = sq.sqrt()   # root-sum-square of the 65536 terms of each element
kd, ld = k.double(), l.double()
ulp = torch.exp2(torch.floor(torch.log2(ld.abs().clamp(min=2.0 ** -126))) - 7)
diff = (kd - ld).abs()
n = k.numel()
differ = diff > 0
beyond = diff > 1.01 * ulp
rms = ex.pow(2).mean().sqrt()
print(f"elements {n}; differ {int(differ.sum())}; beyond one bf16 ulp of the library value {int(beyond.sum())}")
print(f"rms |dW| {rms:.4e}; median |exact| among 'beyond' {ex[beyond].abs().median():.4e}; max {ex[beyond].abs().max():.4e}")
ke, le = (kd - ex).abs(), (ld - ex).abs()
print(f"among 'beyond': kernel closer to fp64 in {int((ke[beyond] < le[beyond]).sum())}, library closer in {int((le[beyond] < ke[beyond]).sum())}, tie {int((le[beyond] == ke[beyond]).sum())}")
print(f"among 'differ': kernel closer {int((ke[differ] < le[differ]).sum())}, library closer {int((le[differ] < ke[differ]).sum())}")
print(f"rel_l2 vs fp64: kernel {(kd-ex).norm()/ex.norm():.4e} library {(ld-ex).norm()/ex.norm():.4e} bf16(exact) {(ex.float().bfloat16().double()-ex).norm()/ex.norm():.4e}")
rb = ex.float().bfloat16().double()
print(f"kernel == bf16(fp64) in {int((kd == rb).sum())} of {n}; library in {int((ld == rb).sum())}")
rel = ex.abs() / size
print(f"|exact| / rss(terms): all elements median {rel.median():.3e}; 'differ' median {rel[differ].median():.3e}; 'beyond' median {rel[beyond].median():.3e} max {rel[beyond].max():.3e}")
print(f"|kernel - library| / rss(terms) among 'beyond': median {(diff[beyond]/size[beyond]).median():.3e} max {(diff[beyond]/size[beyond]).max():.3e}")
print(f"error / rss(terms) among 'beyond': kernel median {(ke[beyond]/size[beyond]).median():.3e} max {(ke[beyond]/size[beyond]).max():.3e}; library median {(le[beyond]/size[beyond]).median():.3e} max {(le[beyond]/size[beyond]).max():.3e}")
kb = ke > 1.01 * torch.exp2(torch.floor(torch.log2(ex.abs().clamp(min=2.0 ** -126))) - 7)
lb = le > 1.01 * torch.exp2(torch.floor(torch.log2(ex.abs().clamp(min=2.0 ** -126))) - 7)
print(f"elements more than one bf16 ulp from fp64: kernel {int(kb.sum())}, library {int(lb.sum())}")
