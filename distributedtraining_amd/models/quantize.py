"""Weight-only serving: swap a loaded model's projection weights for packed
``ops.QuantWeight``s (ops/w8.py). The decode step is a weight stream; int8
codes halve the bytes per token and the memory of a served model, int4 codes
halve them again."""

from __future__ import annotations

import torch

from .. import ops

# projection weights of a block, by family
_GPT2_W = ("attn_qkv_w", "attn_proj_w", "mlp_fc_w", "mlp_proj_w")
_LLAMA_W = ("q_w", "k_w", "v_w", "o_w", "gate_w", "up_w", "down_w")


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


@torch.no_grad()
def quantize_for_serving(model, weights: str = "int8") -> dict:
    """Replace the projection weights of every GPT-2 / Llama / Qwen2 block by
    ``QuantWeight``s, in place, and give the model a quantised head: a
    quantised copy of the tied embedding used only by the logits projection
    (the embedding table itself stays as it is), or the quantised
    ``lm_head_w``. A layer whose K is no multiple of 128 keeps its weight.
    ``weights``: ``"int8"`` or ``"int4"``, the code width of every converted
    layer.

    Call it on the loaded model, on the device it serves from. The model is
    inference-only afterwards (forward without labels, prefill, decode_step,
    generate). Returns ``{"converted", "kept", "bytes_before",
    "bytes_after"}``, the byte counts over the projection and head weights.
    """
    quantize = {"int8": ops.quantize_weight_int8,
                "int4": ops.quantize_weight_int4}.get(weights)
    if quantize is None:
        raise ValueError(f"weights must be 'int8' or 'int4', got {weights!r}")
    names = _GPT2_W if hasattr(model, "wte") else _LLAMA_W
    stats = dict(converted=0, kept=0, bytes_before=0, bytes_after=0)

    def convert(w):
        stats["bytes_before"] += _nbytes(w)
        if w.shape[1] % 128 != 0:
            stats["kept"] += 1
            stats["bytes_after"] += _nbytes(w)
            return None
        qw = quantize(w.detach())
        stats["converted"] += 1
        stats["bytes_after"] += qw.nbytes()
        return qw

    for blk in model.blocks:
        for name in names:
            qw = convert(getattr(blk, name))
            if qw is not None:
                delattr(blk, name)       # the Parameter and its storage go
                setattr(blk, name, qw)
    own_head = getattr(model, "lm_head_w", None)
    if own_head is not None:
        qw = convert(own_head)
        if qw is not None:
            model.head_q = qw
            model.lm_head_w = None
    else:
        tied = model.wte if hasattr(model, "wte") else model.tok_emb
        qw = convert(tied)
        if qw is not None:               # the table stays for the lookup
            stats["bytes_after"] += _nbytes(tied)
            model.head_q = qw
    model.eval()
    return stats
