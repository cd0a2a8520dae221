"""split_kv on the CPU: decode_attention ignores it, KVCache carries it."""

import torch

import _numerics as N
from distributedtraining_amd import ops
from distributedtraining_amd.models.gpt2 import KVCache


def test_cpu_path_ignores_split_kv():
    c = N.decode_case((2, 8, 2, 33, 64, "diffuse"))
    args = (c["q"], c["kc"], c["vc"], 33, c["scale"])
    assert torch.equal(ops.decode_attention(*args, split_kv=3),
                       ops.decode_attention(*args, split_kv=None))


def test_cache_carries_split_kv():
    assert KVCache(1, 2, 2, 16, 64, "cpu", split_kv=3).split_kv == 3
    assert KVCache(1, 2, 2, 16, 64, "cpu").split_kv is None
