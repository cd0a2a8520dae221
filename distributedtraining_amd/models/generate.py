"""Autoregressive generation over the native models (serving path).

The reference is training-only; this provides the serving-side surface a
deployed base model needs: batched greedy / temperature / top-k sampling
driven through the same CDNA4 kernel stack. Two execution modes:

* ``use_cache=True`` (models exposing new_cache/prefill/decode_step, i.e.
  GPT-2): prompt prefill through the causal-attention kernel, then one
  token per step through the flash-decoding KV-cache kernel
  (ops.decode_attention) — O(S) per token;
* ``use_cache=False``: full-context re-forward per token (any model).
"""

from __future__ import annotations

from typing import Optional

import torch


class GraphedDecoder:
    """hipGraph-captured decode step: ~100 eager kernel launches per token
    collapse into ONE graph replay (the round-1 serving path was
    launch-bound at batch 1). Requires a graphable KVCache (device
    position counter) — the captured i32_inc advances it every replay.

    ``sampler(logits, tok)``, when given, is captured behind the decode step:
    it turns the step's logits into the next step's ``self.tok`` on the device
    (ops.sample_tokens and its rng_tick), and a token is ``replay()`` with no
    host work at all."""

    def __init__(self, model, cache, batch: int, device, sampler=None):
        assert cache.pos_dev is not None
        self.model = model
        self.cache = cache
        self.tok = torch.zeros(batch, 1, dtype=torch.long, device=device)
        len0 = cache.len
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):     # allocator warmup (mutates, rewound)
                model.decode_step(self.tok, cache)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        cache.len = len0
        cache.pos_dev.fill_(len0)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.logits = model.decode_step(self.tok, cache)
            if sampler is not None:
                sampler(self.logits, self.tok)
        cache.len = len0           # capture records, does not execute
        cache.pos_dev.fill_(len0)

    def step(self, tok: torch.Tensor) -> torch.Tensor:
        self.tok.copy_(tok, non_blocking=True)
        self.graph.replay()        # device pos advances inside the graph
        self.cache.len += 1
        return self.logits

    def replay(self) -> None:
        """One token of a decoder built with a sampler."""
        self.graph.replay()
        self.cache.len += 1


def _sample(logits, temperature, top_k, generator, top_p=0.0):
    if temperature <= 0:
        return logits.argmax(dim=-1)
    logits = logits / temperature
    if top_k > 0 and top_k < logits.shape[-1]:
        kth = torch.topk(logits, top_k, dim=-1).values[:, -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    if 0.0 < top_p < 1.0:
        # nucleus: keep the smallest prefix of sorted probs summing > p
        sorted_logits, idx = torch.sort(logits, descending=True, dim=-1)
        cum = torch.softmax(sorted_logits, dim=-1).cumsum(dim=-1)
        cut = cum - torch.softmax(sorted_logits, dim=-1) >= top_p
        sorted_logits = sorted_logits.masked_fill(cut, float("-inf"))
        logits = torch.full_like(logits, float("-inf")) \
            .scatter_(-1, idx, sorted_logits)
    probs = torch.softmax(logits, dim=-1)
    return torch.multinomial(probs, 1, generator=generator).squeeze(-1)


@torch.no_grad()
def generate(model, input_ids: torch.Tensor, max_new_tokens: int,
             temperature: float = 0.0, top_k: int = 0,
             top_p: float = 0.0,
             eos_token_id: Optional[int] = None,
             generator: Optional[torch.Generator] = None,
             use_cache: bool = False,
             seed: Optional[int] = None,
             kv_cache: str = "bf16",
             prefill_chunk: int = 0) -> torch.Tensor:
    """Extend ``input_ids`` [B, S] by up to ``max_new_tokens``.

    temperature 0 = greedy; top_k > 0 restricts sampling to the k highest
    logits; 0 < top_p < 1 restricts to the smallest nucleus of tokens
    whose probability mass exceeds top_p (applied after top_k).
    Stops early when every sequence has produced eos_token_id.

    ``seed`` selects the fused sampler (ops.sample_tokens, which documents
    where its tokens differ from the default path's): the draws come from a
    per-generation counter that starts at ``seed``, ``generator`` is unused,
    and on the GPU cached decode replays decode step, sampler and counter
    tick as one graph with the host looking at ``done`` every 16 tokens.
    Output shape and early stop are those of the default path.

    ``kv_cache`` ("bf16" or "int8", with ``use_cache``): the format of the KV
    cache (``KVCache(kv_dtype=)``). int8 halves the cache and the decode
    attention traffic and changes the numbers from the second new token on;
    prefill attends the freshly computed bf16 K and V either way.

    ``prefill_chunk`` (with ``use_cache``): 0 < prefill_chunk < S feeds the
    prompt to ``model.prefill`` in pieces of that many tokens, each attending
    the cache filled so far (ops.extend_attention), so prompt activations are
    bounded by the piece and not by S. 0: one pass. The GPU kernel has no
    int8-cache form, so chunking an int8 cache there raises.
    """
    if kv_cache not in ("bf16", "int8"):
        raise ValueError(f"generate: kv_cache {kv_cache!r} (bf16 or int8)")
    if prefill_chunk < 0:
        raise ValueError(f"generate: prefill_chunk {prefill_chunk}")
    if (0 < prefill_chunk < input_ids.shape[1] and kv_cache == "int8"
            and use_cache and input_ids.is_cuda):
        raise ValueError("generate: chunked prefill has no int8-cache kernel "
                         "on the GPU (kv_cache='bf16', or prefill_chunk=0)")
    if seed is not None:
        return _generate_seeded(model, input_ids, max_new_tokens, temperature,
                                top_k, top_p, eos_token_id, use_cache,
                                int(seed), kv_cache, prefill_chunk)
    model_was_training = model.training
    model.eval()
    n_pos = getattr(model, "cfg").n_positions
    ids = input_ids
    done = torch.zeros(ids.shape[0], dtype=torch.bool, device=ids.device)
    try:
        if use_cache and hasattr(model, "prefill"):
            total = min(ids.shape[1] + max_new_tokens, n_pos)
            cache = model.new_cache(ids.shape[0], total, ids.device,
                                    graphable=ids.is_cuda, kv_dtype=kv_cache)
            logits = _prefill(model, ids, cache, prefill_chunk).float()
            dec = None
            for _ in range(max_new_tokens):
                nxt = _sample(logits, temperature, top_k, generator,
                              top_p=top_p)
                if eos_token_id is not None:
                    nxt = torch.where(done,
                                      torch.full_like(nxt, eos_token_id),
                                      nxt)
                    done |= nxt == eos_token_id
                ids = torch.cat([ids, nxt.unsqueeze(1)], dim=1)
                if ((eos_token_id is not None and bool(done.all()))
                        or cache.len >= cache.max_len):
                    break
                # capture costs ~2 warmup decodes + the graph build —
                # only worth amortizing over a long enough generation
                if (dec is None and cache.pos_dev is not None
                        and max_new_tokens >= 16):
                    dec = GraphedDecoder(model, cache, ids.shape[0],
                                         ids.device)
                step = dec.step if dec is not None else (
                    lambda t: model.decode_step(t, cache))
                logits = step(ids[:, -1:]).float()
            return ids
        for _ in range(max_new_tokens):
            ctx = ids[:, -n_pos:]
            logits = model(input_ids=ctx).logits[:, -1].float()
            nxt = _sample(logits, temperature, top_k, generator,
                          top_p=top_p)
            if eos_token_id is not None:
                nxt = torch.where(done, torch.full_like(nxt, eos_token_id),
                                  nxt)
                done |= nxt == eos_token_id
            ids = torch.cat([ids, nxt.unsqueeze(1)], dim=1)
            if eos_token_id is not None and bool(done.all()):
                break
    finally:
        if model_was_training:
            model.train()
    return ids


def _prefill(model, ids, cache, chunk):
    """``model.prefill`` of the prompt, in pieces of ``chunk`` tokens when
    0 < chunk < S; the logits are those of the last piece."""
    if not 0 < chunk < ids.shape[1]:
        return model.prefill(ids, cache)
    for s0 in range(0, ids.shape[1], chunk):
        logits = model.prefill(ids[:, s0:s0 + chunk], cache)
    return logits


_POLL = 16     # tokens between two host looks at ``done`` (seeded path)


def _generate_seeded(model, input_ids, max_new_tokens, temperature, top_k,
                     top_p, eos, use_cache, seed, kv_cache="bf16",
                     prefill_chunk=0):
    from .. import ops
    from ..ops.backend import require_ext
    model_was_training = model.training
    model.eval()
    n_pos = getattr(model, "cfg").n_positions
    B, S = input_ids.shape
    dev = input_ids.device
    ctr = torch.full((1,), seed, dtype=torch.int64, device=dev)
    done = (torch.zeros(B, dtype=torch.bool, device=dev)
            if eos is not None else None)

    def sample(logits, **kw):
        ops.sample_tokens(logits, temperature, top_k, top_p, ctr, done=done,
                          eos=eos, **kw)
        if ctr.is_cuda:
            require_ext().rng_tick(ctr)    # capturable
        else:
            ctr.add_(1)

    try:
        if not (use_cache and hasattr(model, "prefill")):
            ids = input_ids
            for _ in range(max_new_tokens):
                tok = torch.empty(B, 1, dtype=torch.long, device=dev)
                sample(model(input_ids=ids[:, -n_pos:]).logits[:, -1],
                       tok=tok)
                ids = torch.cat([ids, tok], dim=1)
                if eos is not None and bool(done.all()):
                    break
            return ids
        # the default path samples once per cache position S .. total
        total = min(S + max_new_tokens, n_pos)
        n_new = min(max_new_tokens, total - S + 1)
        if n_new <= 0:
            return input_ids
        cache = model.new_cache(B, total, dev, graphable=input_ids.is_cuda,
                                kv_dtype=kv_cache)
        ids = torch.zeros(B, S + n_new, dtype=torch.long, device=dev)
        ids[:, :S] = input_ids
        tok = torch.zeros(B, 1, dtype=torch.long, device=dev)

        def sample_at_cache_pos(logits, tok):
            sample(logits, tok=tok, ids=ids,
                   pos=cache.pos_dev if cache.pos_dev is not None
                   else cache.len)

        sample_at_cache_pos(_prefill(model, input_ids, cache, prefill_chunk),
                            tok)
        dec = None
        for i in range(1, n_new):
            if (i - 1) % _POLL == 0 and eos is not None and bool(done.all()):
                break
            if (dec is None and cache.pos_dev is not None
                    and max_new_tokens >= 16):
                dec = GraphedDecoder(model, cache, B, dev,
                                     sampler=sample_at_cache_pos)
                dec.tok.copy_(tok)
            if dec is not None:
                dec.replay()
            else:
                sample_at_cache_pos(model.decode_step(tok, cache), tok)
        if eos is not None:
            # cut where the default path stops: the first column at which
            # every row has produced eos
            all_done = (ids[:, S:] == eos).cummax(dim=1).values.all(dim=0)
            if bool(all_done.any()):
                ids = ids[:, :S + int(all_done.int().argmax()) + 1]
        return ids
    finally:
        if model_was_training:
            model.train()
