"""Flash attention with the stage prefetch in flight under the compute.

The double-buffered kernels (32x32 forward and dQ, 8-wave dK/dV) issue the
next tile's LDS-DMA behind the tile-boundary barrier and wait for it only
in front of the next barrier. What that can break: a tile read from a
buffer that is stale or has only half landed, a swizzle applied on one
side only, a wait missing on a path that skips a tile's compute. Each case

  (a) compares o, dq, dk, dv with an fp64 reference (the definition of
      ops.reference.attention, which itself computes in fp32, written out
      in double; autograd for the gradients), at the tolerances
      tests/test_ops_gpu.py and tests/test_attn_dkv_gpu.py use for the
      same quantities, and
  (b) calls the op 10 times on the same inputs and requires every output
      to be bit-equal: a race shows up as a run-to-run difference.

Inputs are seeded random with a different scale per 64-row tile (0.25 to
1.0 of the neighbouring tests' scale), so a tile taken from the wrong
buffer moves the result far outside the tolerance.

Shapes, the smallest that reach each path:
  - 32x32 forward and dQ (S % 256 == 0): S = 256 is one q-block, tiles 0-3
    with the prologue stage, one buffer wrap and the causal skip path;
    S = 512 adds a block whose waves skip while others still compute.
    Documents of 64 and 192 tokens alternate, so the second q-block of
    S = 512 begins past tile 0 and its waves skip leading tiles.
  - dK/dV <D,8,2>: S = 128 (one k-tile, no paired pass), S = 384 (odd
    tile count: the middle tile runs once, re-prime after a pass), and
    S = 256 / 512 from the cases above; <D,4,1> at S = 64 and 192 (left
    as it was). Both launch modes.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
O_TOL = 3e-2     # atol = rtol, tests/test_ops_gpu.py::test_flash_attention_fwd_bwd
GRAD_TOL = 5e-2  # the same test and tests/test_attn_dkv_gpu.py
MODES = {"direct": "1", "split": "0"}  # PRIME_ATTN_DKV_DIRECT
B, H, HKV = 1, 2, 1  # GQA group 2
REPEATS = 10


def _doc_start(S):
    """Documents of 64 and 192 tokens, alternating."""
    ds = torch.zeros(B, S, dtype=torch.int32)
    s, n = 0, 64
    while s < S:
        ds[:, s:] = s
        s, n = s + n, 256 - n
    return ds


def _tile_scaled(t, g):
    """Scale each 64-row tile of a [B,S,...] tensor by its own factor."""
    S = t.shape[1]
    f = torch.tensor([0.25 * (1 + (i * 3 + g) % 4) for i in range(S // 64)])
    return t * f.repeat_interleave(64).view(1, S, *([1] * (t.dim() - 2)))


def _reference(q, k, v, causal, ds):
    """ops.reference.attention in double."""
    S, D = q.shape[1], q.shape[3]
    k = k.repeat_interleave(H // HKV, dim=2)
    v = v.repeat_interleave(H // HKV, dim=2)
    qf, kf, vf = (t.transpose(1, 2) for t in (q, k, v))
    scores = qf @ kf.transpose(-1, -2) / (D**0.5)
    if causal:
        mask = torch.triu(torch.ones(S, S, dtype=torch.bool), 1)
        scores = scores.masked_fill(mask, float("-inf"))
    if ds is not None:
        j = torch.arange(S).view(1, 1, S)
        scores = scores.masked_fill((j < ds.long().view(B, S, 1)).unsqueeze(1), float("-inf"))
    return (scores.softmax(-1) @ vf).transpose(1, 2)


@functools.lru_cache(maxsize=None)
def _case(S, D, mask):
    """Inputs and fp64 reference outputs: computed once, never modified."""
    g = torch.Generator().manual_seed(977 + 13 * S + D + len(mask))
    q = _tile_scaled(0.5 * torch.randn(B, S, H, D, generator=g), 0).bfloat16()
    k = _tile_scaled(0.5 * torch.randn(B, S, HKV, D, generator=g), 1).bfloat16()
    v = _tile_scaled(0.5 * torch.randn(B, S, HKV, D, generator=g), 2).bfloat16()
    do = _tile_scaled(torch.randn(B, S, H, D, generator=g), 3).bfloat16()
    ds = _doc_start(S) if mask == "doc" else None
    causal = mask != "full"
    ref = [t.double().requires_grad_(True) for t in (q, k, v)]
    o = _reference(*ref, causal, ds)
    o.backward(do.double())
    want = (o.detach().float(),) + tuple(t.grad.float() for t in ref)
    return (q, k, v, do, ds, causal), want


def _run(inputs):
    from prime_amd import ops

    q, k, v, do, ds, causal = inputs
    q, k, v = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    o = ops.flash_attention(q, k, v, causal=causal,
                            doc_start=None if ds is None else ds.to(DEV))
    o.backward(do.to(DEV))
    return tuple(t.detach().float().cpu() for t in (o, q.grad, k.grad, v.grad))


def _check(S, D, mask, mode, monkeypatch):
    monkeypatch.setenv("PRIME_ATTN_DKV_DIRECT", MODES[mode])
    # two slices, so that the split mode strides its q loop and the direct
    # mode re-primes its stage per slice
    monkeypatch.setenv("PRIME_AMD_DKV_SPLITS", "2")
    inputs, want = _case(S, D, mask)
    first = _run(inputs)
    what = f"S={S} D={D} {mask} {mode}"
    for name, g, w, tol in zip(("o", "dq", "dk", "dv"), first, want,
                               (O_TOL, GRAD_TOL, GRAD_TOL, GRAD_TOL)):
        assert bool(torch.isfinite(g).all()), f"{what} {name} not finite"
        print(f"{what} {name}: max abs diff {float((g - w).abs().max()):.3e}")
        torch.testing.assert_close(g, w, atol=tol, rtol=tol,
                                   msg=lambda m, n=name: f"{what} {n}: {m}")
    for i in range(1, REPEATS):
        again = _run(inputs)
        for name, a, b in zip(("o", "dq", "dk", "dv"), first, again):
            assert torch.equal(a, b), f"{what} {name}: call {i} differs from call 0"


@pytest.mark.parametrize("mask", ["causal", "full", "doc"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [256, 512])
def test_v5_forward_dq_prefetch(S, D, mask, monkeypatch):
    _check(S, D, mask, "direct", monkeypatch)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("mask", ["causal", "full", "doc"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [128, 384, 64, 192])
def test_dkv_prefetch_both_shapes(S, D, mask, mode, monkeypatch):
    _check(S, D, mask, mode, monkeypatch)
