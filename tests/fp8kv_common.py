"""Shared by tests/test_decode_fp8kv_cpu.py and tests/test_decode_fp8kv_gpu.py:
the model-step setup of the existing ragged model test (llama_150m, 2 layers,
12/6 heads, prompts of 5/33/64 tokens) and the measured effect of quantising
the KV cache on it."""
import torch

from prime_amd import ops

MODEL_KW = dict(n_layers=2, n_heads=12, n_kv_heads=6)
L0 = (5, 33, 64)
SMAX = 128

# Pure quantisation effect, per prompt of L0: max abs difference of the new
# token's final hidden state between the fp32 CPU model decoding over the
# plain-torch fp8 cache (prefill through kv_store_fp8, one seq_pos step) and
# the same fp32 model with no cache at all. No kernel and no bf16 arithmetic
# is involved: the weights are the bf16-rounded values the GPU model holds,
# the arithmetic is fp32. Measured on the CPU by quantisation_effect() below;
# test_decode_fp8kv_cpu.py recomputes it and holds this constant to it.
E_Q_MEASURED = (9.0132e-02, 6.2788e-02, 7.3915e-02)


def step_tokens(cfg):
    """n + 1 tokens per prompt: the prompt and the token decoded next."""
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, cfg.vocab_size, (n + 1,), generator=g) for n in L0]


def build_cpu_model():
    """The model of the GPU tests' fixture (seed 0), weights rounded to bf16
    and held in fp32 on the CPU."""
    from prime_amd.models import Llama
    from prime_amd.models.configs import get_config

    torch.manual_seed(0)
    cfg = get_config("llama_150m", **MODEL_KW)
    m = Llama(cfg)
    m.load_state_dict({k: v.to(torch.bfloat16).float()
                       for k, v in m.state_dict().items()})
    m.eval()
    return m


@torch.no_grad()
def fp8_step(model, toks, dev):
    """Prefill the three prompts (padded to 64) into fp8 caches, then one
    ragged step: hidden state [3, dim] of each prompt's next token."""
    cfg = model.cfg
    caches = [ops.kv_cache_fp8(len(L0), SMAX, cfg.n_kv_heads, cfg.head_dim, dev)
              for _ in range(cfg.n_layers)]
    pad = torch.zeros(len(L0), 64, dtype=torch.int64, device=dev)
    for b, (t, n) in enumerate(zip(toks, L0)):
        pad[b, :n] = t[:n].to(dev)
    model(pad, caches=caches, pos=0)
    cur = torch.stack([t[-1:] for t in toks]).to(dev)
    sp = {"pos": torch.tensor(L0, dtype=torch.int32, device=dev),
          "lens": torch.tensor([n + 1 for n in L0], dtype=torch.int32, device=dev)}
    return model(cur, caches=caches, seq_pos=sp)[:, 0]


@torch.no_grad()
def quantisation_effect(m32=None):
    """(e_q per prompt, fp32 reference hidden states)."""
    m32 = m32 or build_cpu_model()
    toks = step_tokens(m32.cfg)
    ref = [m32(t[None])[0, -1] for t in toks]
    new = fp8_step(m32, toks, "cpu")
    return [(new[b] - ref[b]).abs().max().item() for b in range(len(L0))], ref
