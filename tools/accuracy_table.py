#!/usr/bin/env python
"""Markdown table for docs/test_accuracy.md from the rows that
tests/test_kernel_accuracy_gpu.py writes when DTA_ACCURACY_REPORT is set:

    DTA_ACCURACY_REPORT=acc.json python -m pytest \\
        tests/test_kernel_accuracy_gpu.py -m gpu
    python tools/accuracy_table.py acc.json

One line per (op, tensor): the number of checks and the case with the
largest kernel / baseline ratio (the larger of the rel_l2 and worst_row
ratios; a baseline of zero means the kernel had to be exact, and was).
"""

import json
import sys


def ratio(r):
    out = 0.0
    for k, b in ((r["kern_l2"], r["base_l2"]), (r["kern_worst"], r["base_worst"])):
        if b > 0:
            out = max(out, k / b)
        elif k > 0:
            out = float("inf")
    return out


def main(path):
    rows = json.load(open(path))
    groups = {}
    for r in rows:
        groups.setdefault((r["op"], r["tensor"], r["fp32"]), []).append(r)
    print("| op | tensor | rule | checks | worst case | baseline rel_l2 / "
          "worst_row | kernel rel_l2 / worst_row | ratio | bound used |")
    print("|---|---|---|---|---|---|---|---|---|")
    for (op, tensor, fp32), rs in groups.items():
        # how much of its bound the worst check used (fp32: the bound is
        # max(16 x baseline, 4 ulp), so the ratio alone does not tell)
        def used(r):
            return max(r["kern_l2"] / r["bound_l2"] if r["bound_l2"] else 0.0,
                       r["kern_worst"] / r["bound_worst"]
                       if r["bound_worst"] else 0.0)
        w = max(rs, key=used)
        rt = ratio(w)
        print(f"| {op} | {tensor} | {'fp32 16x' if fp32 else 'bf16 3x'} | "
              f"{len(rs)} | {w['case']} | {w['base_l2']:.2e} / "
              f"{w['base_worst']:.2e} | {w['kern_l2']:.2e} / "
              f"{w['kern_worst']:.2e} | {rt:.2f} | {used(w):.0%} |")


if __name__ == "__main__":
    main(sys.argv[1])
