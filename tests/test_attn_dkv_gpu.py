"""dK/dV backward of flash attention on the GPU: the kernel in its two
launch modes (direct bf16 output with causal k-tile pairing, and the
grid-split q loop with fp32 partials), against the fp32 CPU reference.

Shapes are the smallest at which each piece can go wrong: S=128 is one
k-tile (the diagonal only), S=256 one causal pair, S=384 an odd tile count
whose middle tile pairs with itself, S=192 the 4-wave instantiation."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 5e-2  # atol = rtol, as test_flash_attention_fwd_bwd compares gradients
MODES = {"direct": "1", "split": "0"}  # PRIME_ATTN_DKV_DIRECT

# name -> (B, S, H, Hkv, D)
SHAPES = {
    "s128_d64_g4": (2, 128, 4, 1, 64),
    "s128_d128_g1": (2, 128, 2, 2, 128),
    "s256_d128_g4": (2, 256, 8, 2, 128),
    "s256_d64_g1": (2, 256, 1, 1, 64),
    "s384_d128_g4": (2, 384, 4, 1, 128),
    "s384_d64_g1": (2, 384, 2, 2, 64),
    "s192_d128_g4": (2, 192, 8, 2, 128),
    "s192_d64_g1": (2, 192, 1, 1, 64),
}

# name -> (shape, document starts per batch row); no boundary is a multiple
# of 16 except the ones that sit on a 128-key tile edge on purpose
DOC_CASES = {
    # row 0: a single-token document (0), one that ends exactly on the tile
    # edge (37..128); row 1: one that spans the edge (100..171)
    "doc256": ("s256_d128_g4", [[0, 1, 37, 128, 203], [0, 100, 171]]),
    # row 0: 50..256 spans the first edge and ends exactly on the second, a
    # single-token last document (383); row 1: a two-token document, and
    # 133..301 spans the second edge
    "doc384": ("s384_d64_g1", [[0, 50, 256, 383], [0, 131, 133, 301]]),
}


def _doc_start(starts, S):
    ds = torch.zeros(len(starts), S, dtype=torch.int32)
    for b, row in enumerate(starts):
        for s in row:
            ds[b, s:] = s
    return ds


def _split_qkv(qkv, H, Hkv, D):
    """q/k/v as strided views of one packed [B,S,(H+2Hkv)*D] buffer."""
    B, S, _ = qkv.shape
    q = qkv[..., : H * D].view(B, S, H, D)
    k = qkv[..., H * D: (H + Hkv) * D].view(B, S, Hkv, D)
    v = qkv[..., (H + Hkv) * D:].view(B, S, Hkv, D)
    return q, k, v


@functools.lru_cache(maxsize=None)
def _case(shape, causal, doc=None):
    """Inputs and the CPU fp32 reference gradients: computed once, shared by
    the tests that need them, never modified."""
    from prime_amd import ops

    B, S, H, Hkv, D = SHAPES[shape]
    g = torch.Generator().manual_seed(4321 + 7 * S + D + H)
    qkv = (0.5 * torch.randn(B, S, (H + 2 * Hkv) * D, generator=g)).bfloat16()
    do = torch.randn(B, S, H, D, generator=g).bfloat16()
    ds = None if doc is None else _doc_start(DOC_CASES[doc][1], S)
    ref = qkv.float().requires_grad_(True)
    qr, kr, vr = _split_qkv(ref, H, Hkv, D)
    ops.reference.attention(qr, kr, vr, causal=causal, doc_start=ds).backward(do.float())
    return (qkv, do, ds), tuple(t.contiguous() for t in _split_qkv(ref.grad, H, Hkv, D))


def _run(shape, qkv, do, ds, causal, mode, monkeypatch):
    from prime_amd import ops

    monkeypatch.setenv("PRIME_ATTN_DKV_DIRECT", MODES[mode])
    # two splits, so that the split mode really strides its q loop and sums
    # partials (these sequences are too short for the default to split)
    monkeypatch.setenv("PRIME_AMD_DKV_SPLITS", "2")
    _, _, H, Hkv, D = SHAPES[shape]
    buf = qkv.to(DEV).requires_grad_(True)
    q, k, v = _split_qkv(buf, H, Hkv, D)
    o = ops.flash_attention(q, k, v, causal=causal,
                            doc_start=None if ds is None else ds.to(DEV))
    o.backward(do.to(DEV))
    return tuple(t.float().cpu().contiguous() for t in _split_qkv(buf.grad, H, Hkv, D))


def _close(got, want, what):
    for name, g, w in zip(("dq", "dk", "dv"), got, want):
        assert bool(torch.isfinite(g).all()), f"{what} {name} not finite"
        print(f"{what} {name}: max abs diff {float((g - w).abs().max()):.3e}")
        torch.testing.assert_close(g, w, atol=TOL, rtol=TOL,
                                   msg=lambda m, n=name: f"{what} {n}: {m}")


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_dkv_both_modes_vs_reference(shape, causal, monkeypatch):
    (qkv, do, _), want = _case(shape, causal)
    got = {m: _run(shape, qkv, do, None, causal, m, monkeypatch) for m in MODES}
    for m in MODES:
        _close(got[m], want, f"{m} vs reference")
    _close(got["direct"], got["split"], "direct vs split")
    # direct mode adds the same q-loop slices in the same order
    assert torch.equal(got["direct"][1], got["split"][1]), "dK: modes differ in bits"
    assert torch.equal(got["direct"][2], got["split"][2]), "dV: modes differ in bits"


@pytest.mark.parametrize("doc", list(DOC_CASES))
def test_dkv_doc_mask_both_modes_vs_reference(doc, monkeypatch):
    shape = DOC_CASES[doc][0]
    (qkv, do, ds), want = _case(shape, True, doc)
    got = {m: _run(shape, qkv, do, ds, True, m, monkeypatch) for m in MODES}
    for m in MODES:
        _close(got[m], want, f"{m} vs reference")
    _close(got["direct"], got["split"], "direct vs split")
    # direct mode adds the same q-loop slices in the same order
    assert torch.equal(got["direct"][1], got["split"][1]), "dK: modes differ in bits"
    assert torch.equal(got["direct"][2], got["split"][2]), "dV: modes differ in bits"


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("doc", [None, "doc384"])
def test_dkv_is_repeatable(doc, mode, monkeypatch):
    shape = "s384_d128_g4" if doc is None else DOC_CASES[doc][0]
    (qkv, do, ds), _ = _case(shape, True, doc)
    first = _run(shape, qkv, do, ds, True, mode, monkeypatch)
    again = _run(shape, qkv, do, ds, True, mode, monkeypatch)
    assert torch.equal(first[1], again[1]), "dK differs between two calls"
    assert torch.equal(first[2], again[2]), "dV differs between two calls"


@pytest.mark.parametrize("B,S,H,D", [(2, 128, 4, 64), (2, 192, 6, 128)])
def test_delta_kernel_bhs_outputs(B, S, H, D):
    """The [B,H,S] copies are the [B,S,H] arrays permuted, bit for bit."""
    from prime_amd.ops._lib import check, lib, ptr, stream_of

    g = torch.Generator().manual_seed(99)
    do = torch.randn(B, S, H, D, generator=g).bfloat16().to(DEV)
    o = torch.randn(B, S, H, D, generator=g).bfloat16().to(DEV)
    lse = torch.randn(B, S, H, generator=g).to(DEV)
    delta = torch.full((B, S, H), float("nan"), device=DEV)
    rowc = torch.full((2, B, H, S), float("nan"), device=DEV)
    check(lib().prime_attn_delta_t(stream_of(do), ptr(do), ptr(o), ptr(lse), ptr(delta),
                                   ptr(rowc), B, S, H, D), "attn_delta")
    want = (do.float() * o.float()).sum(-1)
    torch.testing.assert_close(delta, want, atol=1e-3, rtol=1e-3)
    assert torch.equal(rowc[0], lse.permute(0, 2, 1))
    assert torch.equal(rowc[1], delta.permute(0, 2, 1))
