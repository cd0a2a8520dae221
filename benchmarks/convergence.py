#!/usr/bin/env python3
"""Protocol convergence: held-out eval loss across averaging rounds.

The BASELINE metric is tokens/s PLUS "eval loss after K averaging rounds"
— this produces the latter: N miners do local SGD on disjoint shards of a
byte-level corpus, the averager merges their deltas each round
(configurable strategy), and the validator's held-out eval loss is
recorded after every merge. The merged model must improve on held-out
data round over round (the whole point of the reference's protocol).

Usage: python benchmarks/convergence.py [--rounds 6] [--miners 4]
       [--steps-per-round 30] [--strategy mean|nesterov|parameterized]
       [--exchange-dtype fp32|bf16|int8|topk] [--topk-k 128]
       [--topk-block 4096] [--topk-error-feedback true|false]
       [--strategy trimmed_mean|median] [--trim-count 1]
       [--poison K --poison-kind scale|signflip|nan]
--exchange-dtype (default fp32: the deltas reach the averager as they are)
sends every miner's delta through that wire form first; topk keeps one
error-feedback residual per miner across the rounds.
--strategy trimmed_mean / median is the coordinate-wise robust merge
(--trim-count miners dropped per side for trimmed_mean); the JSON then holds
every round's per-miner outside share. --poison K replaces the deltas of the
last K miners before the merge: by -20 x delta (scale), -delta (signflip) or
NaN (nan).
Prints one JSON line; add --table for a human round-by-round table.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--miners", type=int, default=4)
    ap.add_argument("--steps-per-round", type=int, default=30)
    ap.add_argument("--strategy", default="mean",
                    choices=["mean", "nesterov", "parameterized",
                             "score_weighted", "trimmed_mean", "median"])
    ap.add_argument("--trim-count", type=int, default=1)
    ap.add_argument("--poison", type=int, default=0,
                    help="the last K miners send a hostile delta")
    ap.add_argument("--poison-kind", default="scale",
                    choices=["scale", "signflip", "nan"])
    ap.add_argument("--tokenizer", default="byte", choices=["byte", "bpe"],
                    help="byte: 258-vocab byte tokenizer; bpe: GPT-2-style "
                         "byte-level BPE trained offline on the corpus "
                         "(ragged lengths -> the padding/attention-mask "
                         "path is exercised end to end)")
    ap.add_argument("--exchange-dtype", default="fp32",
                    choices=["fp32", "bf16", "int8", "topk"])
    ap.add_argument("--topk-k", type=int, default=128)
    ap.add_argument("--topk-block", type=int, default=4096)
    ap.add_argument("--topk-error-feedback", default="true",
                    choices=["true", "false"])
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    robust = args.strategy in ("trimmed_mean", "median")
    if robust and args.exchange_dtype == "topk":
        ap.error("the robust merges do not take top-k deltas")
    if not 0 <= args.poison <= args.miners:
        ap.error("--poison must be between 0 and --miners")

    from distributedtraining_amd.config import (AverageConfig, Config,
                                                ModelConfig)
    from distributedtraining_amd import ops
    from distributedtraining_amd.models import build_model
    from distributedtraining_amd.parallel.comm import PackedDeltas
    from distributedtraining_amd.parallel.flat import FlatParams
    from distributedtraining_amd.roles.averager import ParameterizedAverager
    from distributedtraining_amd.roles.miner import DeltaLoop
    from distributedtraining_amd.roles.validator import DeltaValidator
    from distributedtraining_amd.utils.textdata import (ByteTokenizer,
                                                        TextDataset,
                                                        text_batches)

    use_gpu = torch.cuda.is_available()
    dev = torch.device("cuda:0" if use_gpu else "cpu")

    # synthetic byte corpus with real sequential structure, sharded
    # disjointly across miners (each miner sees a different slice — the
    # merge must combine them)
    def corpus(shard: int, n: int = 200):
        return [f"shard {shard} line {i}: the quick brown fox jumps over "
                f"the lazy dog while counting {i * shard + i} apples"
                for i in range(n)]

    if args.tokenizer == "bpe":
        # offline-trained GPT-2-style BPE (utils/bpe.py): variable-length
        # rows => padding + attention_mask flow through the kernels
        from distributedtraining_amd.utils.bpe import train_bpe
        train_corpus = [t for s in range(1, args.miners + 1)
                        for t in corpus(s)]
        tok = train_bpe(train_corpus, vocab_size=512)
    else:
        tok = ByteTokenizer()

    cfg = Config()
    # vocab rounded up to a multiple of 8 (norm/CE kernel width contract)
    vs = (tok.vocab_size + 7) // 8 * 8
    cfg.model = ModelConfig(family="gpt2", vocab_size=vs,
                            n_layer=2, n_head=4, n_embd=128, n_positions=64)
    cfg.train.lr = 5e-4
    seq = 48

    torch.manual_seed(0)
    base_model = build_model(cfg.model).to(dev)
    fp = FlatParams(base_model)
    base = fp.snapshot()

    held_out = TextDataset(corpus(999), tokenizer=tok, seq_len=seq)
    ev = [next(text_batches(held_out, 16, seed=7)) for _ in range(4)]

    validator = DeltaValidator(base_model, fp, ev, cfg.validate)
    av = ParameterizedAverager(base_model, fp,
                               AverageConfig(strategy=args.strategy,
                                             meta_epochs=2, meta_lr=0.01,
                                             trim_count=args.trim_count))
    outside_shares = []
    losses = [validator.base_loss]
    feedback = args.topk_error_feedback == "true"
    residuals = [None] * args.miners     # topk: what a miner has not sent

    for rnd in range(args.rounds):
        deltas = []
        for m in range(args.miners):
            fp.load_flat_master(base)
            ds = TextDataset(corpus(m + 1), tokenizer=tok, seq_len=seq)
            loop = DeltaLoop(base_model, fp,
                             text_batches(ds, 16, seed=100 * rnd + m),
                             cfg.train)
            loop.train(args.steps_per_round)
            delta = loop.make_delta().flat.clone()
            if m >= args.miners - args.poison:
                if args.poison_kind == "scale":
                    delta.mul_(-20.0)
                elif args.poison_kind == "signflip":
                    delta.neg_()
                else:
                    delta.fill_(float("nan"))
            if args.exchange_dtype == "topk":
                if feedback and residuals[m] is None:
                    residuals[m] = torch.zeros_like(delta)
                delta, _ = ops.topk_compress_blockwise(
                    delta, args.topk_k, args.topk_block,
                    residual=residuals[m], update_residual=feedback)
            deltas.append(delta)
        stack = torch.stack(deltas)
        if args.exchange_dtype == "topk":
            stack = PackedDeltas("topk", stack, fp.numel, None,
                                 args.topk_block, args.topk_k)
        elif args.exchange_dtype != "fp32":
            stack = PackedDeltas.pack(stack, args.exchange_dtype)
        if args.exchange_dtype != "fp32" and args.strategy == "nesterov":
            stack = stack.dequantize()
        fp.load_flat_master(base)
        if args.strategy == "parameterized":
            merged = av.meta_learning(base, stack, ev)
        elif args.strategy == "nesterov":
            merged = av.nesterov_merge(base, stack)
        elif robust:
            merged = av.robust_merge(base, stack)
            outside_shares.append([round(x, 4)
                                   for x in av.last_outside_share])
        elif args.strategy == "score_weighted":
            merged = av.score_weighted_merge(base, stack,
                                             [1.0] * args.miners)
        else:
            merged = av.merged_from(base, stack,
                                    av._uniform_weights(args.miners))
        fp.load_flat_master(merged)
        base = fp.snapshot()
        loss, _ = validator.evaluate_model()
        losses.append(loss)
        if args.table:
            print(f"round {rnd + 1}: held-out loss {loss:.4f}")

    out = {"metric": "held-out eval loss after K averaging rounds",
           "device": "MI355X" if use_gpu else "cpu",
           "tokenizer": args.tokenizer, "vocab_size": vs,
           "strategy": args.strategy, "miners": args.miners,
           "exchange_dtype": args.exchange_dtype,
           "steps_per_round": args.steps_per_round,
           "rounds": args.rounds, "initial_loss": round(losses[0], 4),
           "final_loss": round(losses[-1], 4),
           "losses": [round(x, 4) for x in losses],
           "improved": losses[-1] < losses[0]}
    if args.exchange_dtype == "topk":
        out.update(topk_k=args.topk_k, topk_block=args.topk_block,
                   topk_error_feedback=feedback)
    if robust:
        out.update(trim_count=args.trim_count,
                   outside_share=outside_shares)
    if args.poison:
        out.update(poison=args.poison, poison_kind=args.poison_kind)
    print(json.dumps(out))
    return 0 if out["improved"] else 1


if __name__ == "__main__":
    sys.exit(main())
