"""Real-text training data (offline twin of the reference's pipeline).

The reference streams WikiText-103 through the GPT-2 tokenizer
(/root/reference/neurons/miner.py:54,69-92: per-text tokenization with
max_length truncation to seq 64, labels = input_ids). This environment
has no hub access, so the same pipeline is provided over local sources:

* ``ByteTokenizer`` — dependency-free byte-level tokenizer (vocab 256 +
  pad/eos), so "train on real text" works with zero artifacts;
* any HF tokenizer loaded from LOCAL files plugs in unchanged
  (``transformers.AutoTokenizer.from_pretrained(local_dir)``);
* ``TextDataset`` — line/paragraph records from a text file, tokenized
  with truncation+padding to seq_len (the reference's WikitextDataset
  contract, incl. labels = input_ids);
* ``text_batches`` — endless shuffled batch iterator (the DataLoader +
  custom_collate_fn role, neurons/miner.py:95-106);
* ``PackedTextDataset`` / ``packed_text_batches`` — sequence packing: the
  records are concatenated with EOS separators and the stream is cut into
  full rows, with the ``doc_start`` layout the models need to keep every
  document on its own (no truncation, no padding).
"""

from __future__ import annotations

import os
from typing import Iterator, List, Optional

import torch


class ByteTokenizer:
    """Byte-level tokenizer: token = byte value; 256 = PAD, 257 = EOS."""

    vocab_size = 258
    pad_token_id = 256
    eos_token_id = 257

    def encode(self, text: str, max_length: Optional[int] = None) -> List[int]:
        ids = list(text.encode("utf-8"))
        if max_length is not None:
            ids = ids[:max_length]
        return ids

    def decode(self, ids) -> str:
        return bytes(i for i in ids if i < 256).decode("utf-8",
                                                       errors="replace")

    def __call__(self, text: str, max_length: int, truncation: bool = True,
                 padding: str = "max_length"):
        ids = self.encode(text, max_length if truncation else None)
        attn = [1] * len(ids)
        if padding == "max_length" and len(ids) < max_length:
            pad = max_length - len(ids)
            ids = ids + [self.pad_token_id] * pad
            attn = attn + [0] * pad
        return {"input_ids": ids, "attention_mask": attn}


class TextDataset:
    """Per-record tokenized dataset (reference: WikitextDataset,
    neurons/miner.py:69-92 — each text truncated/padded to seq_len,
    labels = input_ids)."""

    def __init__(self, source, tokenizer=None, seq_len: int = 64,
                 min_chars: int = 8):
        self.texts = _load_texts(source, min_chars)
        self.tokenizer = tokenizer or ByteTokenizer()
        self.seq_len = seq_len

    def __len__(self) -> int:
        return len(self.texts)

    def __getitem__(self, idx: int) -> dict:
        enc = self.tokenizer(self.texts[idx], max_length=self.seq_len,
                             truncation=True, padding="max_length")
        ids = torch.tensor(enc["input_ids"], dtype=torch.long)
        return {"input_ids": ids, "labels": ids.clone(),
                "attention_mask": torch.tensor(enc["attention_mask"],
                                               dtype=torch.long)}


def text_batches(dataset: TextDataset, batch_size: int, seed: int = 0,
                 shuffle: bool = True) -> Iterator[dict]:
    """Endless batch iterator (the reference's DataLoader + collate,
    neurons/miner.py:95-106); re-shuffles each epoch."""
    g = torch.Generator().manual_seed(seed)
    n = len(dataset)
    assert n > 0, "empty dataset"
    while True:
        order = torch.randperm(n, generator=g) if shuffle else torch.arange(n)
        for i in range(0, n - batch_size + 1, batch_size):
            items = [dataset[int(j)] for j in order[i:i + batch_size]]
            yield {k: torch.stack([it[k] for it in items])
                   for k in items[0]}
        if n < batch_size:   # tiny datasets: single undersized batch
            items = [dataset[int(j)] for j in order]
            yield {k: torch.stack([it[k] for it in items])
                   for k in items[0]}


def _load_texts(source, min_chars: int) -> List[str]:
    """Records of a text file (one per line) or of an iterable of strings,
    without the ones shorter than ``min_chars``."""
    if isinstance(source, str) and os.path.exists(source):
        with open(source, encoding="utf-8", errors="replace") as f:
            texts = f.read().split("\n")
    elif isinstance(source, str):
        raise FileNotFoundError(source)
    else:
        texts = list(source)
    return [t for t in texts if len(t.strip()) >= min_chars]


class PackedTextDataset:
    """Records tokenized WITHOUT truncation, each followed by the
    tokenizer's EOS, for :func:`packed_text_batches` to concatenate and cut
    into rows of ``seq_len``. Nothing past the first ``seq_len`` tokens of a
    record is thrown away and no row carries padding."""

    def __init__(self, source, tokenizer=None, seq_len: int = 64,
                 min_chars: int = 8):
        self.tokenizer = tokenizer or ByteTokenizer()
        self.seq_len = seq_len
        eos = self.tokenizer.eos_token_id
        if eos is None:
            raise ValueError("packing needs a tokenizer with an EOS token")
        self.eos_token_id = int(eos)
        # one int64 tensor per document, tokenized once
        self.docs = [torch.tensor(self._encode(t) + [self.eos_token_id],
                                  dtype=torch.long)
                     for t in _load_texts(source, min_chars)]

    def _encode(self, text: str) -> List[int]:
        tok = self.tokenizer
        if isinstance(tok, ByteTokenizer):
            return tok.encode(text)
        return list(tok.encode(text, add_special_tokens=False))

    def __len__(self) -> int:
        return len(self.docs)

    def stream(self, order) -> torch.Tensor:
        """The documents in ``order``, concatenated (int64 [n_tokens])."""
        return torch.cat([self.docs[int(j)] for j in order])

    def rows(self, st: torch.Tensor, multiple: int = 1):
        """(ids [R, seq_len] int64, doc_start [R, seq_len] int32, tail):
        the token stream ``st`` cut into whole rows, R a multiple of
        ``multiple``, and the tokens left over. doc_start is 0 at column 0
        and s + 1 carried forward after every EOS at column s, so a document
        cut by a row end goes on in the next row as a document that starts
        at column 0."""
        S = self.seq_len
        R = st.numel() // (S * multiple) * multiple
        ids = st[:R * S].view(R, S)
        col = torch.arange(S, dtype=torch.int32)
        # start candidates: column 0, and the column after each EOS
        after_eos = torch.zeros(R, S, dtype=torch.bool)
        after_eos[:, 1:] = ids[:, :-1] == self.eos_token_id
        cand = torch.where(after_eos, col.expand(R, S),
                           torch.zeros(R, S, dtype=torch.int32))
        return ids, torch.cummax(cand, dim=1).values.contiguous(), st[R * S:]


def packed_text_batches(dataset: PackedTextDataset, batch_size: int,
                        seed: int = 0, shuffle: bool = True) -> Iterator[dict]:
    """Endless iterator of packed batches: ``input_ids``, ``labels`` (equal
    to the ids; the model ignores each document's first token as a target)
    and ``doc_start`` (int32, passes ``ops.check_q_lo``). Documents are
    ordered by a seeded shuffle, redrawn every epoch. Every batch is full;
    the tokens of an epoch that do not fill a whole batch of rows open the
    next epoch's stream, so no token is dropped, whatever ``batch_size``."""
    from ..ops import check_doc_start
    g = torch.Generator().manual_seed(seed)
    n = len(dataset)
    assert n > 0, "empty dataset"
    tail = torch.empty(0, dtype=torch.long)
    while True:
        order = torch.randperm(n, generator=g) if shuffle else torch.arange(n)
        ids, doc_start, tail = dataset.rows(
            torch.cat([tail, dataset.stream(order)]), batch_size)
        if ids.shape[0] == 0:   # less than one batch per epoch: keep collecting
            continue
        check_doc_start(doc_start)
        for i in range(0, ids.shape[0], batch_size):
            rows = ids[i:i + batch_size]
            yield {"input_ids": rows.clone(), "labels": rows.clone(),
                   "doc_start": doc_start[i:i + batch_size].clone()}


def doc_start_kw(batch: dict, device) -> dict:
    """``{"doc_start": tensor on device}`` for a packed batch, else ``{}``:
    what the training and scoring loops add to the model call."""
    ds = batch.get("doc_start")
    if ds is None:
        return {}
    return {"doc_start": ds.to(device, non_blocking=True)}
