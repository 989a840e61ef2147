"""fp8 weight-only linear on the host: the LinearW8 format (quantisation rule,
pre-shuffled bytes, dequantisation) and the guards."""
import pytest
import torch


def lossless(w, spread=True):
    """w [N, K] snapped to rows that quantise without loss: e4m3 values times
    a power-of-two row scale, row max 448 * 2^j. Returns (w', j [N])."""
    w = w.float()
    if spread:  # rows of different magnitude: 2^(n % 5 - 2)
        w = w * 2.0 ** (torch.arange(w.shape[0]) % 5 - 2).unsqueeze(1)
    j = torch.log2(w.abs().amax(1) / 448).round()
    q = (w / 2.0 ** j.unsqueeze(1)).clamp(-448, 448)
    q = q.to(torch.float8_e4m3fn).float()
    top = w.abs().argmax(1, keepdim=True)
    q.scatter_(1, top, 448 * torch.sign(w.gather(1, top)))
    return q * 2.0 ** j.unsqueeze(1), j


def test_quant_matches_the_formula():
    from prime_amd import ops

    torch.manual_seed(0)
    N, K = 128, 512
    w = (torch.randn(N, K) * 0.05).to(torch.bfloat16)
    w[5] = 0
    lw = ops.quant_weight_fp8(w)
    assert (lw.N, lw.K) == (N, K) and lw.w8.dtype == torch.uint8
    assert lw.w8.shape == (N // 16, K // 64, 64, 16) and lw.w8.is_contiguous()
    m = w.float().abs().amax(1).clamp(min=1e-12)
    fm = torch.tensor(448.0)
    assert torch.equal(lw.sinv, m / fm)
    rows = (w.float() * (fm / m).unsqueeze(1)).clamp(-448, 448) \
        .to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(lw.w8, rows.view(N // 16, 16, K // 64, 4, 16)
                       .permute(0, 2, 3, 1, 4).reshape(lw.w8.shape))
    # lane l = lg*16 + li of tile (nt, kc): row nt*16 + li, cols kc*64 + lg*16..
    assert torch.equal(lw.w8[3, 5, 2 * 16 + 7], rows[3 * 16 + 7, 352:368])
    assert (lw.w8[0, :, 5::16] == 0).all() and lw.sinv[5] == 1e-12 / fm


def test_dequant_undoes_the_shuffle():
    from prime_amd import ops

    torch.manual_seed(1)
    w, j = lossless(torch.randn(192, 768))
    assert torch.equal(w.abs().amax(1), 448 * 2.0 ** j)
    assert torch.equal(w.to(torch.bfloat16).float(), w)  # bf16 holds it
    lw = ops.quant_weight_fp8(w.to(torch.bfloat16))
    assert torch.equal(lw.sinv, 2.0 ** j)
    assert torch.equal(ops.weight_fp8_dequant(lw), w)
    x = torch.randn(3, 5, 768).to(torch.bfloat16)
    want = torch.nn.functional.linear(x.float(), w).to(torch.bfloat16)
    assert torch.equal(ops.linear_w8(x, lw), want)  # the host path


@pytest.mark.parametrize("N,K", [(96, 256), (64, 192), (64, 0)])
def test_shape_errors(N, K):
    from prime_amd import ops

    with pytest.raises(ValueError):
        ops.quant_weight_fp8(torch.zeros(N, K, dtype=torch.bfloat16))


def test_generate_batch_needs_the_gpu():
    from prime_amd.models import build_model
    from prime_amd.models.generate import generate_batch

    model = build_model("llama_test")
    with pytest.raises(ValueError, match="GPU"):
        generate_batch(model, [[1, 2, 3]], 2, weight_dtype="fp8")
    with pytest.raises(ValueError, match="weight_dtype"):
        generate_batch(model, [[1, 2, 3]], 2, weight_dtype="int4")
    assert model.quantize_decode_weights() == 0  # no llama_test shape qualifies
