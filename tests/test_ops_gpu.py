"""GPU numerics tests: every HIP kernel vs the PyTorch fp32 reference.

All inputs are RANDOM and ASYMMETRIC (guide §3: symmetric inputs silently
pass transposed MFMA layouts)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _bf(x):
    return x.to(DEV, dtype=torch.bfloat16)


@pytest.fixture(scope="module", autouse=True)
def _seed():
    torch.manual_seed(1234)


def test_hip_lib_loads():
    from prime_amd.ops import have_lib

    assert have_lib(), "HIP kernel library must load on GPU machines"


def test_mfma_layout_vs_matmul():
    """16x16x32 MFMA fragment-map verification with asymmetric random A,B."""
    from prime_amd import ops

    A = torch.randn(16, 32).clamp(-2, 2)
    B = torch.randn(32, 16).clamp(-2, 2)
    got = ops.mfma_probe(_bf(A).contiguous(), _bf(B).contiguous())
    torch.cuda.synchronize()
    want = _bf(A).float() @ _bf(B).float()
    torch.testing.assert_close(got.cpu(), want.cpu(), atol=1e-3, rtol=1e-3)


def test_rmsnorm_fwd_bwd():
    from prime_amd import ops

    x = _bf(torch.randn(33, 1024)).requires_grad_(True)
    w = _bf(torch.randn(1024)).requires_grad_(True)
    y = ops.rmsnorm(x, w)
    dy = _bf(torch.randn_like(y.detach()))
    y.backward(dy)

    xr = x.detach().float().cpu().requires_grad_(True)
    wr = w.detach().float().cpu().requires_grad_(True)
    yr = ops.reference.rmsnorm(xr, wr)
    yr.backward(dy.float().cpu())

    torch.testing.assert_close(y.detach().float().cpu(), yr.detach(), atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(x.grad.float().cpu(), xr.grad, atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(w.grad.float().cpu(), wr.grad, atol=0.1, rtol=3e-2)


def test_cross_block_reductions_are_repeatable():
    """dw of both norm backwards and the gradient square norm are summed
    across thread blocks in a fixed order: repeated calls on the same input
    give the same bits (a float-atomic sum does not), and dw stays correct
    when there are more rows than the 1024 partial rows (R = 2500, odd).

    dw tolerance: the sum is kept in fp32 and rounded once to bf16, so
    |err| <= 2^-8 |dw| (rtol 2^-7 leaves a factor 2) plus the fp32
    accumulation error, at most R * 2^-24 * max|term| ~ 2500 * 6e-8 * 25
    = 4e-3 (atol)."""
    from prime_amd import ops

    R, D = 2500, 512
    x = _bf(torch.randn(R, D))
    res = _bf(torch.randn(R, D))
    w = _bf(torch.randn(D))
    dy = _bf(torch.randn(R, D))

    def norm_dw():
        wl = w.clone().requires_grad_(True)
        ops.rmsnorm(x, wl).backward(dy)
        return wl.grad

    def add_norm_dw():
        wl = w.clone().requires_grad_(True)
        xl = x.clone().requires_grad_(True)
        y, s = ops.fused_add_rmsnorm(xl, res, wl)
        torch.autograd.backward([y, s], [dy, dy])
        return wl.grad

    def sqnorm():
        sq = torch.zeros(1, device=DEV)
        ops.grad_sqnorm(g, sq)
        return sq

    g = _bf(torch.randn(2048 * 256 * 8 + 4099) * 3)  # grid at its cap + tail
    for fn in (norm_dw, add_norm_dw, sqnorm):
        first = fn()
        for _ in range(4):
            assert torch.equal(fn(), first), fn.__name__

    for s_in, got in ((x, norm_dw()), (x.float() + res.float(), add_norm_dw())):
        sf = s_in.float().cpu()
        rstd = torch.rsqrt(sf.pow(2).mean(-1, keepdim=True) + 1e-5)
        # as the kernel: rstd from the fp32 sum, xhat from the stored bf16 sum
        xhat = sf.bfloat16().float() * rstd
        want = (dy.double().cpu() * xhat.double()).sum(0).float()
        torch.testing.assert_close(got.float().cpu(), want, rtol=2**-7, atol=4e-3)
    # no rows at all: dw is zero, not an error
    wl = w.clone().requires_grad_(True)
    ops.rmsnorm(x[:0], wl).backward(dy[:0])
    y, s = ops.fused_add_rmsnorm(x[:0].clone().requires_grad_(True), res[:0], wl)
    torch.autograd.backward([y, s], [dy[:0], dy[:0]])
    assert wl.grad.shape == w.shape and torch.count_nonzero(wl.grad) == 0
    # positive terms, fp32: 64 serial adds per thread then trees, error well
    # under 100 ulp = 6e-6 relative
    want = g.double().pow(2).sum().float().cpu().reshape(1)
    torch.testing.assert_close(sqnorm().cpu(), want, rtol=1e-5, atol=0)


def test_rope_fwd_bwd():
    from prime_amd import ops
    from prime_amd.ops import reference as ref

    B, S, H, D = 2, 128, 4, 128
    cos, sin = ref.rope_tables(D, 256, device=DEV)
    x = _bf(torch.randn(B, S, H, D)).requires_grad_(True)
    y = ops.apply_rope(x, cos, sin)
    dy = _bf(torch.randn_like(y.detach()))
    y.backward(dy)

    xr = x.detach().float().cpu().requires_grad_(True)
    yr = ref.apply_rope(xr, cos.cpu(), sin.cpu())
    yr.backward(dy.float().cpu())
    torch.testing.assert_close(y.detach().float().cpu(), yr.detach(), atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(x.grad.float().cpu(), xr.grad, atol=2e-2, rtol=2e-2)


def test_swiglu_fwd_bwd():
    from prime_amd import ops

    gu = _bf(torch.randn(65, 512)).requires_grad_(True)
    y = ops.swiglu(gu)
    dy = _bf(torch.randn_like(y.detach()))
    y.backward(dy)

    gr = gu.detach().float().cpu().requires_grad_(True)
    yr = ops.reference.swiglu(gr)
    yr.backward(dy.float().cpu())
    torch.testing.assert_close(y.detach().float().cpu(), yr.detach(), atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(gu.grad.float().cpu(), gr.grad, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("gqa", [False, True])
def test_flash_attention_fwd_bwd(causal, gqa):
    from prime_amd import ops

    B, S, H, D = 2, 256, 4, 128
    Hkv = 2 if gqa else H
    q = _bf(0.5 * torch.randn(B, S, H, D)).requires_grad_(True)
    k = _bf(0.5 * torch.randn(B, S, Hkv, D)).requires_grad_(True)
    v = _bf(0.5 * torch.randn(B, S, Hkv, D)).requires_grad_(True)
    o = ops.flash_attention(q, k, v, causal=causal)
    do = _bf(torch.randn_like(o.detach()))
    o.backward(do)

    qr = q.detach().float().cpu().requires_grad_(True)
    kr = k.detach().float().cpu().requires_grad_(True)
    vr = v.detach().float().cpu().requires_grad_(True)
    orf = ops.reference.attention(qr, kr, vr, causal=causal)
    orf.backward(do.float().cpu())

    torch.testing.assert_close(o.detach().float().cpu(), orf.detach(), atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(q.grad.float().cpu(), qr.grad, atol=5e-2, rtol=5e-2)
    torch.testing.assert_close(k.grad.float().cpu(), kr.grad, atol=5e-2, rtol=5e-2)
    torch.testing.assert_close(v.grad.float().cpu(), vr.grad, atol=5e-2, rtol=5e-2)


def test_flash_attention_head_dim_64():
    from prime_amd import ops

    B, S, H, D = 1, 128, 2, 64
    q = _bf(torch.randn(B, S, H, D))
    k = _bf(torch.randn(B, S, H, D))
    v = _bf(torch.randn(B, S, H, D))
    o = ops.flash_attention(q, k, v, causal=True)
    want = ops.reference.attention(
        q.float().cpu(), k.float().cpu(), v.float().cpu(), causal=True
    )
    torch.testing.assert_close(o.float().cpu(), want, atol=3e-2, rtol=3e-2)


def test_cross_entropy_fwd_bwd():
    from prime_amd import ops
    import torch.nn.functional as F

    R, V = 64, 32000
    logits = _bf(torch.randn(R, V)).requires_grad_(True)
    tgt = torch.randint(0, V, (R,), device=DEV)
    tgt[5] = -100
    loss = ops.cross_entropy(logits, tgt)
    loss.backward()

    lr = logits.detach().float().cpu().requires_grad_(True)
    want = F.cross_entropy(lr, tgt.cpu(), ignore_index=-100)
    want.backward()
    torch.testing.assert_close(loss.float().cpu(), want.detach(), atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(
        logits.grad.float().cpu(), lr.grad, atol=2e-3, rtol=5e-2
    )


def test_fused_adamw_vs_reference():
    from prime_amd import ops
    from prime_amd.ops import reference as ref

    N = 4096 + 3  # exercise the scalar tail
    p32 = torch.randn(N, device=DEV)
    p16 = p32.bfloat16()
    g = _bf(torch.randn(N))
    m = torch.zeros(N, device=DEV)
    v = torch.zeros(N, device=DEV)

    p32r, mr, vr = p32.cpu().clone(), m.cpu().clone(), v.cpu().clone()
    for step in (1, 2, 3):
        ops.fused_adamw(p32, p16, g, m, v, lr=1e-2, beta1=0.9, beta2=0.95,
                        eps=1e-8, wd=0.1, step=step)
        ref.adamw_step(p32r, g.float().cpu(), mr, vr, 1e-2, 0.9, 0.95, 1e-8, 0.1, step)
    torch.testing.assert_close(p32.cpu(), p32r, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(m.cpu(), mr, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(v.cpu(), vr, atol=1e-5, rtol=1e-5)
    # the bf16 model weight is the fp32 master rounded once, nothing else
    assert torch.equal(p16, p32.bfloat16())


def test_quant_int8_gpu_vs_reference():
    from prime_amd import ops
    from prime_amd.ops import reference as ref

    x = torch.randn(ops.QBLK * 7, device=DEV) * 0.01
    q, s = ops.quant_int8(x)
    qr, sr = ref.quant_int8_blockwise(x.cpu())
    torch.testing.assert_close(s.cpu(), sr, atol=1e-7, rtol=1e-5)
    # rounding ties may differ by 1 lsb
    assert (q.cpu().int() - qr.int()).abs().max() <= 1
    out = torch.empty_like(x)
    ops.dequant_int8(q, s, out)
    torch.testing.assert_close(out, x, atol=float(x.abs().max() / 127), rtol=0)


def test_nesterov_outer_gpu():
    from prime_amd import ops

    N = 2048
    theta = torch.randn(N, device=DEV)
    master = torch.randn(N, device=DEV)
    p16 = torch.empty(N, device=DEV, dtype=torch.bfloat16)
    buf = torch.randn(N, device=DEV)
    delta = torch.randn(N, device=DEV)
    theta0, buf0 = theta.clone(), buf.clone()

    ops.nesterov_outer(theta, master, p16, buf, delta, lr=0.7, mu=0.9)
    want_buf = 0.9 * buf0 + delta
    want_theta = theta0 - 0.7 * (delta + 0.9 * want_buf)
    torch.testing.assert_close(buf.cpu(), want_buf.cpu(), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(theta.cpu(), want_theta.cpu(), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(master.cpu(), want_theta.cpu(), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(p16.float().cpu(), want_theta.cpu(), atol=1e-2, rtol=1e-2)


def test_pseudograd_gpu():
    from prime_amd import ops

    outer = torch.randn(1024, device=DEV)
    master = torch.randn(1024, device=DEV)
    delta = torch.empty(1024, device=DEV)
    ops.pseudograd(outer, master, delta)
    torch.testing.assert_close(delta, outer - master)


def test_transpose_bshd():
    from prime_amd.ops.functional import transpose_bshd

    B, S, H, D = 2, 128, 3, 128
    x = torch.randn(B, S, H, D, device=DEV).bfloat16()
    got = transpose_bshd(x)
    want = x.permute(0, 2, 3, 1).contiguous()
    assert got.shape == want.shape
    torch.testing.assert_close(got, want)
    # strided view input (like a qkv split)
    big = torch.randn(B, S, H * 2, D, device=DEV).bfloat16()
    view = big[:, :, :H, :]
    torch.testing.assert_close(transpose_bshd(view), view.permute(0, 2, 3, 1).contiguous())


def test_fused_add_rmsnorm_gpu():
    from prime_amd import ops

    x = _bf(torch.randn(33, 1024)).requires_grad_(True)
    res = _bf(torch.randn(33, 1024)).requires_grad_(True)
    w = _bf(torch.randn(1024)).requires_grad_(True)
    y, s = ops.fused_add_rmsnorm(x, res, w)
    dy = _bf(torch.randn_like(y.detach()))
    dsr = _bf(torch.randn_like(s.detach()))
    torch.autograd.backward([y, s], [dy, dsr])

    xr = x.detach().float().cpu().requires_grad_(True)
    rr = res.detach().float().cpu().requires_grad_(True)
    wr = w.detach().float().cpu().requires_grad_(True)
    sr = xr + rr
    yr = ops.reference.rmsnorm(sr, wr)
    torch.autograd.backward([yr, sr], [dy.float().cpu(), dsr.float().cpu()])
    torch.testing.assert_close(y.detach().float().cpu(), yr.detach(), atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(s.detach().float().cpu(), sr.detach(), atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(x.grad.float().cpu(), xr.grad, atol=5e-2, rtol=5e-2)
    torch.testing.assert_close(res.grad.float().cpu(), rr.grad, atol=5e-2, rtol=5e-2)
    torch.testing.assert_close(w.grad.float().cpu(), wr.grad, atol=0.15, rtol=5e-2)


def test_attn_decode_vs_reference():
    from prime_amd import ops

    B, H, Hkv, D, Smax, L = 2, 8, 2, 128, 512, 300
    q = _bf(torch.randn(B, H, D))
    kc = _bf(torch.randn(B, Smax, Hkv, D))
    vc = _bf(torch.randn(B, Smax, Hkv, D))
    got = ops.attn_decode(q, kc, vc, length=L)
    want = ops.reference.attention(
        q.float().cpu().unsqueeze(1), kc[:, :L].float().cpu(),
        vc[:, :L].float().cpu(), causal=False,
    ).squeeze(1)
    torch.testing.assert_close(got.float().cpu(), want, atol=3e-2, rtol=3e-2)


def test_attn_decode_head_dim_64():
    from prime_amd import ops

    B, H, Hkv, D, Smax, L = 1, 4, 4, 64, 256, 129
    q = _bf(torch.randn(B, H, D))
    kc = _bf(torch.randn(B, Smax, Hkv, D))
    vc = _bf(torch.randn(B, Smax, Hkv, D))
    got = ops.attn_decode(q, kc, vc, length=L)
    want = ops.reference.attention(
        q.float().cpu().unsqueeze(1), kc[:, :L].float().cpu(),
        vc[:, :L].float().cpu(), causal=False,
    ).squeeze(1)
    torch.testing.assert_close(got.float().cpu(), want, atol=3e-2, rtol=3e-2)


def test_mfma32_layout_vs_matmul():
    from prime_amd.ops.functional import mfma_probe32

    A = torch.randn(32, 16).clamp(-2, 2)
    B = torch.randn(16, 32).clamp(-2, 2)
    got = mfma_probe32(_bf(A).contiguous(), _bf(B).contiguous())
    torch.cuda.synchronize()
    want = _bf(A).float() @ _bf(B).float()
    torch.testing.assert_close(got.cpu(), want.cpu(), atol=1e-3, rtol=1e-3)


def test_adamw_fused_clip_matches_explicit():
    from prime_amd import ops

    N = 8192
    g = _bf(torch.randn(N) * 3)
    p32a = torch.randn(N, device=DEV)
    p32b = p32a.clone()
    p16a, p16b = p32a.bfloat16(), p32b.bfloat16()
    ma, va = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    mb, vb = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)

    # path a: explicit clip then adamw
    max_norm = 1.0
    norm = g.float().norm()
    ga = (g.float() * (max_norm / (norm + 1e-6)).clamp(max=1.0)).bfloat16()
    ops.fused_adamw(p32a, p16a, ga, ma, va, lr=1e-2, beta1=0.9, beta2=0.95,
                    eps=1e-8, wd=0.0, step=1)
    # path b: fused gscale
    sq = torch.zeros(1, device=DEV)
    ops.grad_sqnorm(g, sq)
    torch.testing.assert_close(sq.sqrt().cpu(), norm.cpu().reshape(1), atol=1e-1, rtol=1e-3)
    gs = (max_norm / (sq.sqrt() + 1e-6)).clamp(max=1.0)
    ops.fused_adamw(p32b, p16b, g, mb, vb, lr=1e-2, beta1=0.9, beta2=0.95,
                    eps=1e-8, wd=0.0, step=1, gscale=gs)
    # bf16 rounding of the pre-scaled grad differs slightly; compare loosely
    torch.testing.assert_close(p32a.cpu(), p32b.cpu(), atol=2e-4, rtol=1e-3)


def test_tuned_linear_matches_reference():
    """Layout-tuned linear (NT fwd, cached-W^T dX, dY^T-NN dW) must match
    plain F.linear numerics, including after an in-place weight update
    (cache invalidation)."""
    import torch.nn.functional as F

    from prime_amd import ops

    ops.set_linear_tuned(True)
    try:
        M, K, N = 4096, 512, 1024
        x = _bf(torch.randn(M, K)).requires_grad_(True)
        w = _bf(torch.randn(N, K)).requires_grad_(True)
        y = ops.tuned_linear(x, w)
        dy = _bf(torch.randn_like(y.detach()))
        y.backward(dy)
        xr = x.detach().clone().requires_grad_(True)
        wr = w.detach().clone().requires_grad_(True)
        yr = F.linear(xr, wr)
        yr.backward(dy)
        torch.testing.assert_close(y.detach(), yr.detach(), atol=3e-2, rtol=3e-2)
        torch.testing.assert_close(x.grad, xr.grad, atol=5e-2, rtol=5e-2)
        torch.testing.assert_close(w.grad, wr.grad, atol=5e-1, rtol=3e-2)
        # in-place weight update must invalidate the cached W^T
        with torch.no_grad():
            w.mul_(2.0)
        ops.invalidate_wt_cache()
        x.grad = None
        ops.tuned_linear(x, w).backward(dy)
        xr.grad = None
        F.linear(xr, wr.detach().mul(2.0).requires_grad_(True)).backward(dy)
        torch.testing.assert_close(x.grad, xr.grad, atol=1e-1, rtol=5e-2)
    finally:
        ops.set_linear_tuned(False)


def test_gemm_nt_vs_library():
    """Custom 256^2-tile MFMA GEMM (the measured in-repo baseline the
    GEMM study in profiles/ cites): exact-shape NT, bf16, fp32 accum —
    must match hipBLASLt numerically."""
    from prime_amd.ops._lib import check, lib, ptr, stream_of

    M, N, K = 512, 768, 256
    a = _bf(torch.randn(M, K))
    w = _bf(torch.randn(N, K))
    c = torch.empty(M, N, device=a.device, dtype=torch.bfloat16)
    check(lib().prime_gemm_nt(stream_of(a), ptr(a), ptr(w), ptr(c),
                              M, N, K, 0), "gemm_nt")
    torch.cuda.synchronize()
    ref = a @ w.T
    torch.testing.assert_close(c, ref, atol=3e-2, rtol=3e-2)
    # unsupported shape must refuse loudly, not corrupt
    rc = lib().prime_gemm_nt(stream_of(a), ptr(a), ptr(w), ptr(c),
                             M + 1, N, K, 0)
    assert rc != 0


def test_fp8_linear_matches_bf16_loosely():
    """Opt-in fp8 forward: same math as the bf16 linear within fp8's
    dynamic-scaled precision; backward stays the bf16 layout-tuned path
    and must match tightly."""
    import torch.nn.functional as F

    from prime_amd import ops

    ops.set_linear_fp8(True)
    try:
        M, K, N = 4096, 512, 1024
        x = _bf(0.5 * torch.randn(M, K)).requires_grad_(True)
        w = _bf(0.5 * torch.randn(N, K)).requires_grad_(True)
        y = ops.tuned_linear(x, w)
        yr = F.linear(x.detach(), w.detach())
        # fp8 e4m3: ~2 decimal digits; compare relative to the output scale
        rel = (y.detach() - yr).float().norm() / yr.float().norm()
        assert float(rel) < 0.06, float(rel)  # e4m3 per-tensor-scale noise
        dy = _bf(torch.randn_like(y.detach()))
        y.backward(dy)
        xr = x.detach().clone().requires_grad_(True)
        wr = w.detach().clone().requires_grad_(True)
        F.linear(xr, wr).backward(dy)
        torch.testing.assert_close(x.grad, xr.grad, atol=5e-2, rtol=5e-2)
        torch.testing.assert_close(w.grad, wr.grad, atol=5e-1, rtol=5e-2)
        # full recipe incl. the fused transpose-quant wgrad path; run the
        # backward twice so the second pass uses seeded (delayed) scales
        ops.set_linear_fp8(True, dgrad=True, wgrad=True)
        for _ in range(2):
            x.grad = w.grad = None
            ops.tuned_linear(x, w).backward(dy)
        rel_w = (w.grad - wr.grad).float().norm() / wr.grad.float().norm()
        rel_x = (x.grad - xr.grad).float().norm() / xr.grad.float().norm()
        assert float(rel_w) < 0.08, float(rel_w)
        assert float(rel_x) < 0.08, float(rel_x)
    finally:
        ops.set_linear_fp8(False)


def test_rowwise_quant_fp8_numerics():
    """Per-row fp8 quantize kernel vs a plain torch fp32 reference: the
    emitted sinv must be rowmax/448 (or /57344 for e5m2) and the cast
    must reconstruct each row within fp8 quantization error."""
    from prime_amd.ops.functional import _quant_rowwise_fp8

    torch.manual_seed(5)
    R, C = 513, 1024  # non-power-of-two row count exercises the grid loop
    # give rows wildly different scales — the case per-row scaling is for
    mags = torch.logspace(-3, 3, R).unsqueeze(1)
    x = _bf(torch.randn(R, C) * mags)
    for e5m2, fmax in ((False, 448.0), (True, 57344.0)):
        x8, sinv = _quant_rowwise_fp8(x, e5m2=e5m2)
        torch.cuda.synchronize()
        assert sinv.shape == (R, 1)
        ref_sinv = x.float().abs().amax(dim=1, keepdim=True).clamp_min(1e-12) / fmax
        torch.testing.assert_close(sinv, ref_sinv, atol=0, rtol=1e-6)
        recon = x8.float() * sinv
        rel = (recon - x.float()).norm(dim=1) / x.float().norm(dim=1)
        # e4m3 ~2^-3 relative step per element; row-norm error far below
        assert float(rel.max()) < (0.12 if e5m2 else 0.03), float(rel.max())


def test_fp8_rowwise_forward_matches(monkeypatch):
    """PRIME_AMD_FP8_ROWWISE=1: the forward GEMM uses per-row activation
    + per-output-channel weight scales and must match bf16 at least as
    tightly as the per-tensor path, including rows of very different
    magnitude (the outlier case per-tensor scaling saturates on)."""
    import torch.nn.functional as F

    from prime_amd import ops

    monkeypatch.setenv("PRIME_AMD_FP8_ROWWISE", "1")
    ops.set_linear_fp8(True)
    try:
        M, K, N = 2048, 512, 1024
        mags = torch.logspace(-2, 2, M).unsqueeze(1)
        x = _bf(0.5 * torch.randn(M, K) * mags)
        w = _bf(0.5 * torch.randn(N, K))
        y = ops.tuned_linear(x, w)
        yr = F.linear(x, w)
        rel = ((y - yr).float().norm(dim=1) / yr.float().norm(dim=1).clamp_min(1e-6))
        # per-ROW relative error stays at e4m3 level even for tiny rows,
        # which per-tensor scaling flushes toward zero
        assert float(rel.max()) < 0.08, float(rel.max())
    finally:
        ops.set_linear_fp8(False)
