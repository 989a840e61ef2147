"""prime_attn_delta_dot: delta, the [B,H,S] row constants and dO^T in one
pass, against the two kernels it replaces in the attention backward
(prime_attn_delta_t followed by transpose_bshd(dO)). Every output must be
equal bit for bit: the tiled kernel walks the reduction tree of the old
one-wave-per-row kernel (see the comment at attn_delta_dot_kernel)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (2, 256, 20, 64) is 10240 rows: more than one grid-stride trip of the old
# kernel (2048 blocks of 4 rows)
SHAPES = [(1, 64, 1, 64), (2, 128, 3, 128), (2, 192, 6, 64), (1, 256, 5, 128),
          (2, 256, 20, 64)]


@pytest.mark.parametrize("B,S,H,D", SHAPES)
def test_delta_dot_equals_delta_t_plus_transpose(B, S, H, D):
    from prime_amd.ops._lib import check, lib, ptr, stream_of
    from prime_amd.ops.functional import transpose_bshd

    g = torch.Generator().manual_seed(7 + B * S * H + D)
    do = torch.randn(B, S, H, D, generator=g).bfloat16().to(DEV)
    o = torch.randn(B, S, H, D, generator=g).bfloat16().to(DEV)
    lse = (4.0 * torch.randn(B, S, H, generator=g)).to(DEV)
    nan = float("nan")

    delta0 = torch.full((B, S, H), nan, device=DEV)
    rowc0 = torch.full((2, B, H, S), nan, device=DEV)
    check(lib().prime_attn_delta_t(stream_of(do), ptr(do), ptr(o), ptr(lse), ptr(delta0),
                                   ptr(rowc0), B, S, H, D), "attn_delta_t")
    dot0 = transpose_bshd(do)

    delta1 = torch.full((B, S, H), nan, device=DEV)
    rowc1 = torch.full((2, B, H, S), nan, device=DEV)
    dot1 = torch.full((B, H, D, S), nan, device=DEV, dtype=torch.bfloat16)
    check(lib().prime_attn_delta_dot(stream_of(do), ptr(do), ptr(o), ptr(lse), ptr(delta1),
                                     ptr(rowc1), ptr(dot1), B, S, H, D), "attn_delta_dot")
    torch.cuda.synchronize()

    for name, got, want in (("delta", delta1, delta0), ("rowc_t", rowc1, rowc0),
                            ("dOt", dot1, dot0)):
        assert not bool(torch.isnan(got).any()), f"{name}: NaN left in the output"
        assert torch.equal(got, want), (
            f"{name}: {int((got != want).sum())} of {want.numel()} elements differ")
    # and the old pair is what it says it is
    assert torch.equal(dot0, do.permute(0, 2, 3, 1))
    assert torch.equal(rowc0[0], lse.permute(0, 2, 1))


def test_flash_backward_through_delta_dot_is_repeatable():
    """One causal backward at (2, 192, 6 heads / 2 kv heads, 128): finite
    gradients, equal in bits across two calls."""
    from prime_amd import ops

    B, S, H, Hkv, D = 2, 192, 6, 2, 128
    g = torch.Generator().manual_seed(11)
    q0 = torch.randn(B, S, H, D, generator=g).bfloat16().to(DEV)
    k0 = torch.randn(B, S, Hkv, D, generator=g).bfloat16().to(DEV)
    v0 = torch.randn(B, S, Hkv, D, generator=g).bfloat16().to(DEV)
    do = torch.randn(B, S, H, D, generator=g).bfloat16().to(DEV)

    def once():
        q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
        ops.flash_attention(q, k, v, causal=True).backward(do)
        return q.grad, k.grad, v.grad

    first, again = once(), once()
    for name, a, b in zip(("dq", "dk", "dv"), first, again):
        assert bool(torch.isfinite(a).all()), f"{name} is not finite"
        assert torch.equal(a, b), f"{name} differs between two calls"
