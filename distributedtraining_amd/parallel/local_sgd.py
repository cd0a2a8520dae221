"""Local-SGD node orchestrator: N miner ranks on one MI355X box.

This is the framework's first-class parallelism: each of
the node's GPUs runs one miner doing communication-sparse local SGD on a
shared base; every merge interval the per-rank weight deltas are exchanged
with ONE RCCL collective over the xGMI clique, merged, and the merged base
installed on every rank — replacing the reference's
miner→HF-hub→averager→HF-hub→miner round trip.

Collective choice per strategy (see merge_round): mean/nesterov use an
all-reduce (O(P) resident — mandatory at Llama scale); score-weighted,
meta-learned and genetic use an all-gather (every delta HBM-resident,
optionally bf16/int8/top-k on the wire, and with comm.resident_dtype =
"wire" also in that form in HBM); so do the robust trimmed_mean / median
merges, which need every delta (top-k excluded). Deterministic merges are computed
redundantly by every rank (identical bases, no broadcast); the
meta-learned and genetic merges run on rank 0 (they need val-loss
evaluations) and are broadcast (C2/C5).
"""

from __future__ import annotations

import logging
from typing import Dict, List, Optional

import torch

from ..config import Config
from ..parallel.comm import CommPlane, PackedDeltas, check_topk_format
from ..parallel.flat import FlatParams
from ..roles.averager import ParameterizedAverager
from ..roles.miner import DeltaLoop
from ..roles.validator import DeltaValidator
from ..store import DeltaCheckpoint

log = logging.getLogger(__name__)


class LocalSGDNode:
    def __init__(self, model, fp: FlatParams, data_iter, cfg: Config,
                 comm: CommPlane, val_batches: Optional[List[dict]] = None,
                 merge_strategy: Optional[str] = None):
        self.comm = comm
        self.cfg = cfg
        self.fp = fp
        self.model = model
        self.val_batches = val_batches or []
        self.merge_strategy = merge_strategy or cfg.average.strategy
        # decorrelate the dropout streams across miner ranks (counters
        # start at 0 everywhere; without an offset all miners would draw
        # IDENTICAL mask sequences)
        from ..ops import droprng
        droprng.counter(fp.device).fill_(comm.rank << 32)
        self.miner = DeltaLoop(model, fp, data_iter, cfg.train,
                               hotkey=f"rank{comm.rank}")
        self.averager = ParameterizedAverager(model, fp, cfg.average)
        self.merge_rounds = 0
        self._validator: Optional[DeltaValidator] = None
        self._validator_base = None   # base tensor identity at last refresh
        # top-k error feedback: what this miner has not sent yet, fp32 [P],
        # made on first use and zeroed with every fresh initial base
        self.residual: Optional[torch.Tensor] = None
        if self._topk():
            check_topk_format(cfg.comm.topk_k, cfg.comm.topk_block)
            if self.merge_strategy in ("trimmed_mean", "median"):
                raise ValueError(
                    f"merge strategy {self.merge_strategy!r} cannot run on "
                    "comm.exchange_dtype = 'topk': most coordinates are sent "
                    "by fewer than half of the miners, so a coordinate-wise "
                    "median would zero almost everything")

    def _topk(self) -> bool:
        return self.cfg.comm.exchange_dtype == "topk"

    def _topk_residual(self) -> Optional[torch.Tensor]:
        if not self.cfg.comm.topk_error_feedback:
            return None
        if self.residual is None:
            self.residual = torch.zeros_like(self.fp.master,
                                             dtype=torch.float32)
        return self.residual

    def _wire_dtype(self):
        return (torch.bfloat16 if self.cfg.comm.exchange_dtype == "bf16"
                else None)

    def _resident_wire(self) -> bool:
        rd = self.cfg.comm.resident_dtype
        if rd not in ("fp32", "wire"):
            raise ValueError(f"unknown comm.resident_dtype {rd!r}")
        return rd == "wire"

    def _local_delta(self, base: torch.Tensor) -> Optional[torch.Tensor]:
        """This rank's fp32 delta for the gather — None where the gather
        quantises straight from fp.master and base instead (int8 kept in
        wire form: make_delta's fp32 plane is never written)."""
        if self._resident_wire() and self.cfg.comm.exchange_dtype == "int8":
            return None
        if self._topk():
            return None
        return self.fp.make_delta(base).flat    # fused θ−θ_base

    def _gather_deltas(self, flat: Optional[torch.Tensor],
                       base: Optional[torch.Tensor] = None,
                       update_residual: bool = True):
        """All-gather the flat delta at the configured wire dtype. Returns
        [world, P] fp32 for the merge math, or under comm.resident_dtype =
        "wire" a PackedDeltas still in wire form. ``flat`` None (see
        _local_delta): the delta is fp.master − ``base``. top-k compresses
        fp.master − ``base`` plus the residual, which takes what was not sent
        unless ``update_residual`` is False (a round that only scores)."""
        if self._topk():
            c = self.cfg.comm
            packed = self.comm.all_gather_packed(
                self.fp.master, "topk", block=c.topk_block, base=base,
                residual=self._topk_residual(),
                update_residual=update_residual and c.topk_error_feedback,
                k=c.topk_k)
            return packed if self._resident_wire() else packed.dequantize()
        if self._resident_wire():
            if flat is None:
                return self.comm.all_gather_packed(
                    self.fp.master, "int8", base=base)
            return self.comm.all_gather_packed(
                flat, self.cfg.comm.exchange_dtype)
        if self.cfg.comm.exchange_dtype == "int8":
            return self.comm.all_gather_flat_int8(flat)
        return self.comm.all_gather_flat(flat, self._wire_dtype()) \
            .to(torch.float32)

    def sync_initial_base(self) -> None:
        """Rank 0's random init becomes the shared base on all ranks."""
        self.comm.broadcast_flat(self.fp.master, src=0)
        self.fp.sync_work_from_master()
        self.miner.install_base(self.fp.master)
        if self.residual is not None:
            self.residual.zero_()

    def train_steps(self, n: int) -> float:
        last = None
        for _ in range(n):
            last = self.miner.train_step()
        return float(last) if last is not None else float("nan")

    # -- the delta exchange + merge (C1..C5) ---------------------------------
    def merge_round(self, scores: Optional[List[float]] = None) -> None:
        """Exchange + merge. Memory shapes:
        * mean/nesterov: ONE all-reduce of the flat delta — O(P) resident
          (required for Llama-3-8B x 8 ranks: a gather would need 256 GB);
        * score_weighted/parameterized/genetic: all-gather, all deltas
          HBM-resident (8 fp32 GPT-2 deltas ≈ 4 GB — the scoring/meta/
          evolutionary paths need every delta individually); with
          comm.resident_dtype = "wire" they stay bf16/int8 in HBM;
        * trimmed_mean/median: the same gather, then the coordinate-wise
          robust merge on every rank."""
        base = self.miner.base
        strat = self.merge_strategy
        if strat in ("mean", "uniform", "nesterov"):
            delta = self.fp.make_delta(base)     # fused θ−θ_base
            d = self.comm.all_reduce_mean(delta.flat)
            if strat == "nesterov":
                merged = self.averager.nesterov_merge(base, d.unsqueeze(0))
            else:
                merged = d.add_(base)        # in place: d becomes merged
        elif strat == "score_weighted":
            assert scores is not None
            merged = self.averager.score_weighted_merge(
                base, self._gather_deltas(self._local_delta(base), base),
                scores)
        elif strat in ("trimmed_mean", "median"):
            # needs every delta, so the gather path (wire dtype and resident
            # form apply). Bit-identical on every rank whatever the gather
            # order: computed redundantly, no broadcast
            deltas = self._gather_deltas(self._local_delta(base), base)
            merged = self.averager.robust_merge(
                base, deltas,
                self.averager.robust_trim(deltas.shape[0], strat))
        elif strat in ("parameterized", "genetic"):
            # both need val-loss evaluations: run on rank 0, broadcast
            deltas = self._gather_deltas(self._local_delta(base), base)
            if self.comm.rank == 0:
                merged = (self.averager.meta_learning(base, deltas,
                                                      self.val_batches)
                          if strat == "parameterized" else
                          self.averager.genetic_merge(base, deltas,
                                                      self.val_batches))
            else:
                merged = torch.empty_like(base)
            self.comm.broadcast_flat(merged, src=0)
        else:
            raise ValueError(f"unknown merge strategy {strat!r}")
        self.miner.install_base(merged)
        self.merge_rounds += 1

    # -- optional distributed validation (BASELINE config #3) ----------------
    def _refresh_validator(self) -> DeltaValidator:
        """Build the validator once and re-evaluate its cached base loss
        only when the base actually changed (round-1 verdict: a fresh
        validator per round recomputed the base loss every time).
        Caller must have the BASE loaded into fp.master."""
        if self._validator is None:
            self._validator = DeltaValidator(self.model, self.fp,
                                             self.val_batches,
                                             self.cfg.validate)
            self._validator_base = self.miner.base_version
        elif self._validator_base != self.miner.base_version:
            v = self._validator
            v.base_loss, v.base_perplexity = v.evaluate_model()
            self._validator_base = self.miner.base_version
        return self._validator

    def validation_round(self) -> Dict[str, float]:
        """Distributed scoring (round-1 verdict #9): the deltas are
        all-gathered once; each rank scores only its shard
        (i ≡ rank mod world) against the shared BASE model, and the raw
        per-delta scores are all-gathered — per-rank eval cost is
        ~1/world of the reference's every-validator-scores-everything
        loop (validation_logic.py:126-139). Normalization happens
        identically on every rank from the gathered totals."""
        base = self.miner.base
        if self._resident_wire() or self._topk():
            # the configured wire dtype applies to validation too, and the
            # gather stays in that form (rows are applied by ops.axpy_).
            # top-k reads the residual and leaves it alone: the merge round
            # that follows sends this delta again and must count it once
            deltas = self._gather_deltas(self._local_delta(base), base,
                                         update_residual=False)
        else:
            delta = self.fp.make_delta(base)
            deltas = self.comm.all_gather_flat(delta.flat)
        saved = self.fp.master.clone()
        self.fp.load_flat_master(base)   # score against the base, not the
        validator = self._refresh_validator()   # locally-drifted weights
        my: Dict[str, float] = {}
        N = deltas.shape[0]
        for i in range(self.comm.rank, N, self.comm.world_size):
            try:
                if isinstance(deltas, PackedDeltas):
                    _, _, _, ppl_score = validator.score_packed(deltas, i)
                else:
                    ck = DeltaCheckpoint(deltas[i].to(torch.float32),
                                         self.fp.spec, "")
                    _, _, _, ppl_score = validator.score_delta(ck)
            except Exception as e:   # reference: per-miner failure → 0
                log.warning("rank%d scoring failed (%s), score 0", i, e)
                ppl_score = 0.0
            my[f"rank{i}"] = ppl_score
        self.fp.master.copy_(saved)
        self.fp.sync_work_from_master()
        raw: Dict[str, float] = {}
        for d in self.comm.all_gather_object(my):
            raw.update(d)
        total = sum(raw.values())
        return {h: (max(0.0, s / total) if total > 0 else 0.0)
                for h, s in sorted(raw.items())}

    def run(self, total_steps: int, merge_every: int) -> None:
        self.sync_initial_base()
        done = 0
        while done < total_steps:
            n = min(merge_every, total_steps - done)
            self.train_steps(n)
            done += n
            if done < total_steps or total_steps % merge_every == 0:
                self.merge_round()
