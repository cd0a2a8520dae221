"""The token sampler's CPU definition (ops/sampling.py), its draw in the
counter chain, and seeded generation and serving on the CPU."""

import numpy as np
import torch

from distributedtraining_amd import ops
from distributedtraining_amd.config import ModelConfig
from distributedtraining_amd.models import build_model, generate
from distributedtraining_amd.ops import droprng
from distributedtraining_amd.utils.serve import InferenceServer, post_generate

PROBS = [0.5, 0.3, 0.15, 0.05]
N = 400


def test_definition_on_four_tokens():
    logits = torch.tensor([PROBS]).log()
    nucleus = [int(ops.sample_tokens(logits, 1.0, 0, 0.75, c)) for c in range(N)]
    assert set(nucleus) == {0, 1}
    full = np.bincount([int(ops.sample_tokens(logits, 1.0, 0, 0.0, c))
                        for c in range(N)], minlength=4)
    for n, p in zip(full, PROBS):
        assert abs(n - N * p) <= 4 * (N * p * (1 - p)) ** 0.5
    assert int(ops.sample_tokens(logits, 0.0, 0, 0.0, 0)) == 0
    assert int(ops.sample_tokens(logits, 5.0, 1, 0.0, 0)) == 0


def test_sample_hash_by_hand():
    M = (1 << 64) - 1

    def sm64(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    s1 = sm64((5 + 0x53414D50 * 0xA24BAED4963EE407) & M)
    want = sm64((s1 + 2 * 0xD1B54A32D192ED03) & M)
    assert want == 0x43CFC22FDA854788
    assert int(droprng.sample_hash(5, 3)[2]) == want


def _tiny():
    torch.manual_seed(0)
    return build_model(ModelConfig(family="gpt2", vocab_size=64, n_layer=1,
                                   n_head=2, n_embd=32, n_positions=32)).eval()


def test_seeded_generate_on_cpu():
    model = _tiny()
    ids = torch.randint(0, 64, (2, 5))
    kw = dict(max_new_tokens=20, temperature=0.9, top_k=10, top_p=0.9)
    for cached in (True, False):
        a = generate(model, ids, seed=1, use_cache=cached, **kw)
        assert a.shape == (2, 25) and torch.equal(a[:, :5], ids)
        assert torch.equal(a, generate(model, ids, seed=1, use_cache=cached,
                                       **kw))
        assert not torch.equal(a, generate(model, ids, seed=2,
                                           use_cache=cached, **kw))
        eos = int(generate(model, ids[:1], 20, use_cache=cached)[0, 12])
        want = generate(model, ids[:1], 20, eos_token_id=eos, use_cache=cached)
        assert torch.equal(generate(model, ids[:1], 20, eos_token_id=eos,
                                    use_cache=cached, seed=0), want)


def test_server_passes_the_seed():
    srv = InferenceServer(_tiny(), "cpu")
    srv.start()
    try:
        url = f"http://127.0.0.1:{srv.port}"
        kw = dict(max_new_tokens=8, temperature=1.0, top_k=20)
        a = post_generate(url, [[1, 2, 3]], seed=11, **kw)
        assert len(a[0]) == 11 and a == post_generate(url, [[1, 2, 3]],
                                                      seed=11, **kw)
        assert a != post_generate(url, [[1, 2, 3]], seed=12, **kw)
    finally:
        srv.stop()
