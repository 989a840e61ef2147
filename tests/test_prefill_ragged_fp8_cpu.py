"""Chunked prefill over an fp8 cache has no host path: generate_batch on a CPU
model keeps its ValueError (the GPU path: test_prefill_ragged_fp8_gpu.py)."""
import pytest
import torch


def test_generate_batch_chunked_fp8_needs_gpu():
    from prime_amd.models import Llama
    from prime_amd.models.configs import get_config
    from prime_amd.models.generate import generate_batch

    torch.manual_seed(0)
    model = Llama(get_config("llama_150m", n_layers=1, n_heads=4, n_kv_heads=2))
    with pytest.raises(ValueError, match="GPU"):
        generate_batch(model, [[1, 2, 3]], 2, prefill_chunk=16, kv_dtype="fp8")
