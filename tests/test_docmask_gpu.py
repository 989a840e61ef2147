"""Document-masked flash attention on the GPU: every kernel family the
default dispatch reaches (16x16 and 32x32 forward / dQ, the three dK/dV
instantiations, split q loops) against the fp32 CPU reference."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"

# name -> (B, S, H, Hkv, D, document starts per batch row)
CASES = {
    # 16x16 fwd/dq, dkv NW=8: one-token document, a boundary inside a
    # 16-wide sub-tile, a boundary on a tile edge
    "A": (1, 128, 2, 1, 64, [[0, 1, 37, 64, 100]]),
    # 32x32 fwd/dq: two documents in one 32-row wave (70), a q-block that
    # starts on a document (256), a block whose k/v loop starts at 256 while
    # its rows disagree (300), a one-token last document (511); row 1 plain
    "B": (2, 512, 4, 2, 128, [[0, 70, 256, 300, 511], [0]]),
    # S % 128 != 0: dkv NW=4
    "C": (1, 192, 2, 2, 128, [[0, 65, 130]]),
    # 32x32 D=64
    "D": (1, 256, 2, 1, 64, [[0, 200]]),
}


def _bf(x):
    return x.to(DEV, dtype=torch.bfloat16)


def _doc_start(starts, S):
    ds = torch.zeros(len(starts), S, dtype=torch.int32)
    for b, row in enumerate(starts):
        for s in row:
            ds[b, s:] = s
    return ds


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and the CPU fp32 reference of a case: computed once, shared by
    the tests that need them, never modified."""
    from prime_amd import ops

    B, S, H, Hkv, D, starts = CASES[name]
    g = torch.Generator().manual_seed(1234 + ord(name))
    q = (0.5 * torch.randn(B, S, H, D, generator=g)).bfloat16()
    k = (0.5 * torch.randn(B, S, Hkv, D, generator=g)).bfloat16()
    v = (0.5 * torch.randn(B, S, Hkv, D, generator=g)).bfloat16()
    do = torch.randn(B, S, H, D, generator=g).bfloat16()
    ds = _doc_start(starts, S)
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    o = ops.reference.attention(qr, kr, vr, causal=True, doc_start=ds)
    o.backward(do.float())
    return (q, k, v, do, ds), (o.detach(), qr.grad, kr.grad, vr.grad)


def _run(q, k, v, do, ds):
    from prime_amd import ops

    q, k, v = (_bf(t).requires_grad_(True) for t in (q, k, v))
    o = ops.flash_attention(q, k, v, causal=True,
                            doc_start=None if ds is None else ds.to(DEV))
    o.backward(_bf(do))
    return tuple(t.float().cpu() for t in (o.detach(), q.grad, k.grad, v.grad))


def _check(got, want):
    for name, g, w, tol in zip(("o", "dq", "dk", "dv"), got, want,
                               (3e-2, 5e-2, 5e-2, 5e-2)):
        assert bool(torch.isfinite(g).all()), f"{name} not finite"
        print(f"{name}: max abs err {float((g - w).abs().max()):.3e}")
        torch.testing.assert_close(g, w, atol=tol, rtol=tol, msg=lambda m: f"{name}: {m}")


# 1. forward and backward against the reference
@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E"])
def test_doc_mask_fwd_bwd_vs_reference(case, monkeypatch):
    if case == "E":  # B with a non-power-of-two split stride and empty splits
        monkeypatch.setenv("PRIME_AMD_DKV_SPLITS", "3")
        case = "B"
    inputs, want = _case(case)
    _check(_run(*inputs), want)


# 2. a corpus without EOS: the option changes nothing, bit for bit
@pytest.mark.parametrize("case", ["A", "B"])
def test_all_zero_doc_start_is_bit_identical(case):
    (q, k, v, do, ds), _ = _case(case)
    plain = _run(q, k, v, do, None)
    zero = _run(q, k, v, do, torch.zeros_like(ds))
    for name, a, b in zip(("o", "dq", "dk", "dv"), plain, zero):
        assert torch.equal(a, b), name


# 3. nothing leaks across a boundary: a weight of 1e-4 on the poisoned
# document would move the other documents' outputs by ~0.1
def test_poisoned_document_does_not_leak():
    from prime_amd import ops

    (q, k, v, _, ds), _ = _case("B")
    v = v.clone()
    v[0, 70:256] *= 1e3  # the second document of row 0
    want = ops.reference.attention(q.float(), k.float(), v.float(), causal=True,
                                   doc_start=ds)
    got = ops.flash_attention(_bf(q), _bf(k), _bf(v), causal=True,
                              doc_start=ds.to(DEV)).float().cpu()
    assert bool(torch.isfinite(got).all())
    clean = torch.ones(2, 512, dtype=torch.bool)
    clean[0, 70:256] = False
    torch.testing.assert_close(got[clean], want[clean], atol=3e-2, rtol=3e-2)


# 4. q/k/v as the model passes them: slices of one packed projection output
def test_doc_mask_strided_views():
    from prime_amd import ops

    (q, k, v, do, ds), want = _case("D")
    B, S, H, Hkv, D, _ = CASES["D"]
    packed = _bf(torch.cat([q.flatten(2), k.flatten(2), v.flatten(2)], dim=-1))
    packed.requires_grad_(True)
    qs, ks, vs = packed.split([H * D, Hkv * D, Hkv * D], dim=-1)
    qs, ks, vs = qs.view(B, S, H, D), ks.view(B, S, Hkv, D), vs.view(B, S, Hkv, D)
    assert not qs.is_contiguous()
    o = ops.flash_attention(qs, ks, vs, causal=True, doc_start=ds.to(DEV))
    o.backward(_bf(do))
    g = packed.grad.float().cpu()
    dq, dk, dv = g.split([H * D, Hkv * D, Hkv * D], dim=-1)
    _check((o.detach().float().cpu(), dq.view(B, S, H, D), dk.view(B, S, Hkv, D),
            dv.view(B, S, Hkv, D)), want)


def test_doc_start_validation_on_gpu():
    from prime_amd import ops

    q = _bf(torch.randn(1, 64, 2, 64))
    ds = torch.zeros(1, 64, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="causal"):
        ops.flash_attention(q, q, q, causal=False, doc_start=ds)
    with pytest.raises(ValueError, match="is on"):
        ops.flash_attention(q, q, q, causal=True, doc_start=ds.cpu())
    with pytest.raises(TypeError, match="int32"):
        ops.flash_attention(q, q, q, causal=True, doc_start=ds.long())


# 5. end to end through the Trainer
def test_trainer_doc_mask_end_to_end(tmp_path):
    from prime_amd.train import Trainer
    from prime_amd.utils.config import (DataSection, DilocoConfig, MetricsConfig,
                                        ModelConfig, TrainConfig)

    eos = 2
    rng = np.random.default_rng(0)
    toks = rng.integers(3, 32000, size=257 * 16).astype(np.uint16)
    toks[rng.random(toks.size) < 0.01] = eos  # an EOS roughly every 100 tokens
    path = tmp_path / "toks.bin"
    toks.tofile(path)

    first = {}
    for key in (eos, None):
        cfg = TrainConfig(
            run_name="docmask_gpu", steps=3,
            model=ModelConfig(name="llama_150m", seq_len=256),
            data=DataSection(kind="token_file", path=str(path), micro_batch_size=2,
                             shuffle=False, doc_mask_eos_id=key),
            diloco=DilocoConfig(H=100),
            metrics=MetricsConfig(log_interval=100),
        )
        tr = Trainer(cfg, run_dir=tmp_path / f"run_{key}")
        try:
            losses = [float(tr.train_step()) for _ in range(3 if key is not None else 1)]
        finally:
            tr.close()
        assert all(np.isfinite(losses)), losses
        first[key] = losses[0]
    print(f"first loss masked {first[eos]:.6f} plain {first[None]:.6f}")
    assert first[eos] != first[None]
