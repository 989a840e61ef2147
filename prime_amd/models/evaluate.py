"""Evaluation: held-out loss / perplexity over a token stream (the
training-engine counterpart of the reference's `prime eval` surface)."""
from __future__ import annotations

import torch

from ..data import DataConfig, build_dataloader
from .llama import Llama


@torch.no_grad()
def evaluate_perplexity(
    model: Llama,
    data_cfg: DataConfig,
    n_batches: int = 10,
    device: torch.device | str = "cpu",
    doc_mask_eos_id: int | None = None,
) -> dict:
    """doc_mask_eos_id: evaluate with the document mask (attention within
    documents only), as trained with `data.doc_mask_eos_id`."""
    from ..ops import doc_starts

    model.eval()
    loader = build_dataloader(data_cfg, model.cfg.vocab_size, shard=0, n_shards=1)
    total_loss, total_tokens = 0.0, 0
    for _ in range(n_batches):
        x, y = loader.next_batch(torch.device(device))
        if doc_mask_eos_id is None:
            loss = model.loss(x, y)
        else:
            loss = model.loss(x, y, doc_start=doc_starts(x, doc_mask_eos_id))
        ntok = y.numel()
        total_loss += float(loss) * ntok
        total_tokens += ntok
    mean = total_loss / max(1, total_tokens)
    return {
        "loss": mean,
        "perplexity": float(torch.exp(torch.tensor(mean))),
        "tokens": total_tokens,
        "batches": n_batches,
    }
