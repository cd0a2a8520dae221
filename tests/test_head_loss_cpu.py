"""ops.lm_head_loss (forward-only fused LM-head loss) on the CPU gold path,
and its wiring through the models (``loss_only=``) and the validator
(``ValidateConfig.fused_head_loss``)."""

import pytest
import torch
import torch.nn.functional as F

from distributedtraining_amd import ops
from distributedtraining_amd.config import (Config, ModelConfig,
                                            ValidateConfig, from_args)
from distributedtraining_amd.models import build_model
from distributedtraining_amd.parallel.flat import FlatParams
from distributedtraining_amd.roles.validator import DeltaValidator
from distributedtraining_amd.utils.data import synthetic_eval_set


def _inputs(T=37, K=48, V=131, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, K, generator=g).to(torch.bfloat16)
    w = torch.randn(V, K, generator=g).to(torch.bfloat16)
    t = torch.randint(0, V, (T,), generator=g)
    t[::7] = -100   # striped ignored targets
    return x, w, t


def test_cpu_matches_cross_entropy_and_lse():
    x, w, t = _inputs()
    logits = F.linear(x.float(), w.float())
    ref = F.cross_entropy(logits, t, ignore_index=-100)
    loss = ops.lm_head_loss(x, w, t)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert not loss.requires_grad
    torch.testing.assert_close(loss, ref, rtol=1e-6, atol=1e-6)
    loss2, lse = ops.lm_head_loss(x, w, t, return_lse=True)
    torch.testing.assert_close(loss2, ref, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(lse, torch.logsumexp(logits, dim=-1),
                               rtol=1e-6, atol=1e-6)


def test_cpu_flattens_leading_dims():
    x, w, t = _inputs(T=36)
    ref = ops.lm_head_loss(x, w, t)
    got = ops.lm_head_loss(x.view(4, 9, -1), w, t.view(4, 9))
    torch.testing.assert_close(got, ref, rtol=0, atol=0)


def test_cpu_all_ignored_is_zero():
    x, w, t = _inputs()
    t[:] = -100
    loss = ops.lm_head_loss(x, w, t)
    assert float(loss) == 0.0


def test_requires_grad_raises():
    x, w, t = _inputs()
    w = w.float().requires_grad_(True)
    with pytest.raises(RuntimeError, match="lm_head_ce"):
        ops.lm_head_loss(x.float(), w, t)
    with torch.no_grad():   # fine without grad mode
        ops.lm_head_loss(x.float(), w, t)


@pytest.mark.parametrize("mk", [ModelConfig.gpt2_tiny,
                                ModelConfig.llama_tiny])
def test_models_loss_only(mk):
    cfg = mk()
    torch.manual_seed(0)
    model = build_model(cfg).eval()
    ids = torch.randint(0, cfg.vocab_size, (2, 16))
    am = torch.ones(2, 16, dtype=torch.long)
    am[1, 11:] = 0
    with torch.no_grad():
        full = model(input_ids=ids, attention_mask=am, labels=ids)
        lo = model(input_ids=ids, attention_mask=am, labels=ids,
                   loss_only=True)
    assert full.logits is not None      # default path still returns logits
    assert tuple(full.logits.shape) == (2, 15, cfg.vocab_size)
    assert lo.logits is None
    torch.testing.assert_close(lo.loss, full.loss, rtol=1e-5, atol=1e-5)


def test_models_loss_only_rejects_training_with_grad():
    cfg = ModelConfig.gpt2_tiny()
    model = build_model(cfg).train()
    ids = torch.randint(0, cfg.vocab_size, (2, 8))
    with pytest.raises(RuntimeError, match="loss_only"):
        model(input_ids=ids, labels=ids, loss_only=True)


def test_validate_config_flag_and_cli():
    assert ValidateConfig().fused_head_loss is False
    assert from_args([]).validate.fused_head_loss is False
    cfg = from_args(["--validate.fused-head-loss", "true"])
    assert cfg.validate.fused_head_loss is True


def test_validator_flag_same_base_loss():
    cfg = Config()
    cfg.model = ModelConfig.gpt2_tiny()
    ev = synthetic_eval_set(cfg.model.vocab_size, 2, 2, 16)
    losses = {}
    for flag in (False, True):
        torch.manual_seed(0)
        model = build_model(cfg.model)
        fp = FlatParams(model)
        v = DeltaValidator(model, fp, ev,
                           ValidateConfig(fused_head_loss=flag))
        losses[flag] = v.base_loss
    assert losses[True] == pytest.approx(losses[False], rel=1e-5, abs=1e-5)
