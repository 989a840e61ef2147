"""fp8 weight-only linear on the GPU: ops.linear_w8 against an fp64 CPU
reference over exactly the stored bytes, its guards, and the model path."""
import pytest
import torch

from tests.test_linear_w8_cpu import lossless

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _captured(fn):
    """fn() captured as a hipGraph after the usual side-stream warm-up."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


@pytest.mark.parametrize("ksplit", [1, 2, None])
@pytest.mark.parametrize("N,K", [(64, 256), (128, 768), (192, 2048)])
@pytest.mark.parametrize("M", [1, 7, 16, 17, 33, 64])
def test_linear(M, N, K, ksplit):
    """|got - ref| <= 2^-8 |ref| + K 2^-24 sinv[n] sum_k |x dec|: the bf16
    rounding of the output plus worst-case fp32 summation in any order (the
    products are exact in fp32)."""
    from prime_amd import ops

    if ksplit and (K // 256) % ksplit:
        pytest.skip("ksplit does not divide the chunk count")
    torch.manual_seed(M * 1000 + N + K)
    # row n carries 2^(n % 5 - 2): a wrong sinv index shows
    w = torch.randn(N, K) * 2.0 ** (torch.arange(N) % 5 - 2).unsqueeze(1)
    lw = ops.quant_weight_fp8(w.to(DEV, dtype=torch.bfloat16))
    x = torch.randn(M, K).to(DEV, dtype=torch.bfloat16)
    got = ops.linear_w8(x, lw, ksplit=ksplit)
    assert got.shape == (M, N) and got.dtype == torch.bfloat16
    assert torch.equal(got, ops.linear_w8(x, lw, ksplit=ksplit))

    host = ops.LinearW8(lw.w8.cpu(), lw.sinv.cpu(), N, K)
    dec = ops.weight_fp8_dequant(
        host._replace(sinv=torch.ones(N))).double()  # the bytes' values
    sinv, xd = host.sinv.double(), x.double().cpu()
    ref = sinv * (xd @ dec.T)
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * sinv * (xd.abs() @ dec.abs().T)
    err = (got.double().cpu() - ref).abs()
    print(f"max err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()

    # a captured graph replays on new contents of x
    graph, out = _captured(lambda: ops.linear_w8(x, lw, ksplit=ksplit))
    x.copy_(torch.randn(M, K))
    graph.replay()
    assert torch.equal(out, ops.linear_w8(x, lw, ksplit=ksplit))


def test_invalid():
    from prime_amd import ops
    from prime_amd.ops._lib import lib, ptr, stream_of

    lw = ops.quant_weight_fp8(torch.randn(64, 256).to(DEV, dtype=torch.bfloat16))
    x = torch.randn(65, 256).to(DEV, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):
        ops.linear_w8(x, lw)
    y = torch.empty(65, 64, device=DEV, dtype=torch.bfloat16)
    for args in ((ptr(x), ptr(lw.w8), ptr(lw.sinv), ptr(y), None, 8, 64, 192, 1),
                 (ptr(x), None, ptr(lw.sinv), ptr(y), None, 8, 64, 256, 1)):
        assert lib().prime_linear_w8(stream_of(x), *args) == 1


@torch.no_grad()
def test_model_step():
    """One ragged decode step over lossless weights (quantisation is exact, so
    only the kernel differs): with e = max |h - h_ref| against the fp32 CPU
    model, e_w8 <= 2 e_bf16. Both paths round at the same points and differ
    in summation order only; an indexing error is O(1)."""
    from prime_amd.models import Llama
    from prime_amd.models.configs import get_config
    from prime_amd.models.generate import generate_batch, prefill_chunked

    torch.manual_seed(0)
    cfg = get_config("llama_150m", n_layers=2, n_heads=12, n_kv_heads=6)
    m32 = Llama(cfg).eval()
    for lin in m32._prime_linears():
        lin.weight.copy_(lossless(lin.weight, spread=False)[0])
    model = Llama(cfg).to(DEV, dtype=torch.bfloat16).eval()
    model.load_state_dict(m32.state_dict())
    model.reset_rope(DEV)
    m32.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})

    g = torch.Generator().manual_seed(3)
    seqs = [torch.randint(0, cfg.vocab_size, (n + 1,), generator=g)
            for n in (5, 33, 64)]
    ref = torch.stack([m32(t[None])[0, -1] for t in seqs])
    caches = [tuple(torch.zeros(4, 128, cfg.n_kv_heads, cfg.head_dim, device=DEV,
                                dtype=torch.bfloat16) for _ in range(2))
              for _ in range(cfg.n_layers)]
    prefill_chunked(model, caches, [t[:-1].tolist() for t in seqs], 32)
    L = [len(t) - 1 for t in seqs] + [-1]
    tok = torch.tensor([int(t[-1]) for t in seqs] + [0], device=DEV)[:, None]
    pos = torch.tensor(L, dtype=torch.int32, device=DEV)
    seq_pos = {"pos": pos, "lens": (pos + 1).clamp(min=0)}

    def step():
        c = [(k.clone(), v.clone()) for k, v in caches]
        return model(tok, caches=c, seq_pos=seq_pos)[:3, 0].float().cpu()

    e_bf16 = (step() - ref).abs().max().item()
    assert model.quantize_decode_weights() == 4 * cfg.n_layers + 1
    e_w8 = (step() - ref).abs().max().item()
    model.drop_decode_weights()
    print(f"max abs err vs fp32 CPU model: e_bf16 {e_bf16:.4e}, e_w8 {e_w8:.4e}")
    assert e_w8 <= 2 * e_bf16

    prompts = [t[:-1].tolist() for t in seqs]
    eager = generate_batch(model, prompts, 6, use_graph=False, weight_dtype="fp8")
    graphed = generate_batch(model, prompts, 6, use_graph=True, weight_dtype="fp8")
    assert graphed == eager and [len(o) for o in eager] == [6, 6, 6]
    assert all(lin.w8 is None for lin in model._prime_linears())
