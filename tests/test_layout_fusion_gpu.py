"""Layout-fusion kernels and direct wgrad: the fused producers (swiglu
backward + dgu^T, strided RoPE forward, qkv grad pack, the two fused
projection functions, dW written into the flat gradient) must give exactly
what the ops they replace give. Everything here is a bitwise comparison:
the new kernels share their element math with the old ones and the GEMMs
see identical operands."""
import pytest
import torch

gpu = pytest.mark.gpu


def _bf(t):
    return t.to("cuda", dtype=torch.bfloat16)


def _rand(*shape, seed, scale=1.0, shift=0.0):
    """Asymmetric random bf16 tensor (non-zero mean, seeded)."""
    g = torch.Generator().manual_seed(seed)
    return _bf(torch.randn(*shape, generator=g) * scale + shift)


# ------------------------------------------------------- swiglu_bwd + T
@gpu
@pytest.mark.parametrize("R,I", [(64, 64), (192, 320)])
def test_swiglu_bwd_t_matches_backward_and_transpose(R, I):
    from prime_amd import ops

    gu = _rand(R, 2 * I, seed=1, shift=0.3).requires_grad_(True)
    dout = _rand(R, I, seed=2, shift=-0.2)
    ops.swiglu(gu).backward(dout)
    dgu, dgut = ops.swiglu_bwd_t(dout, gu.detach())
    assert dgu.shape == (R, 2 * I) and dgut.shape == (2 * I, R)
    assert torch.equal(dgu, gu.grad)
    assert torch.equal(dgut, dgu.t().contiguous())


@gpu
def test_swiglu_bwd_t_fallback_shape():
    """R = 65 does not tile by 64: plain kernel + transpose, same dgu."""
    from prime_amd import ops

    R, I = 65, 512
    gu = _rand(R, 2 * I, seed=3, shift=0.3).requires_grad_(True)
    dout = _rand(R, I, seed=4, shift=-0.2)
    ops.swiglu(gu).backward(dout)
    dgu, dgut = ops.swiglu_bwd_t(dout, gu.detach())
    assert torch.equal(dgu, gu.grad)
    assert torch.equal(dgut, dgu.t().contiguous())


# ----------------------------------------------- strided RoPE / qkv pack
_B, _S, _H, _HKV = 2, 128, 4, 2


def _tables(D, rows=256):
    from prime_amd.ops import reference

    cos, sin = reference.rope_tables(D, rows, 10000.0, device="cuda")
    return cos.contiguous(), sin.contiguous()


@gpu
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pos_offset", [0, 64])
def test_rope_strided_forward_matches_dense(D, pos_offset):
    from prime_amd import ops

    C = (_H + 2 * _HKV) * D
    qkv = _rand(_B, _S, C, seed=5, shift=0.1)
    cos, sin = _tables(D)
    q = qkv[..., : _H * D].view(_B, _S, _H, D)
    k = qkv[..., _H * D : (_H + _HKV) * D].view(_B, _S, _HKV, D)
    for view in (q, k):
        assert not view.is_contiguous()
        want = ops.apply_rope(view.contiguous(), cos, sin, pos_offset=pos_offset)
        assert torch.equal(ops.rope_packed_fwd(view, cos, sin, pos_offset), want)
        # the autograd op takes the same route for such views
        assert torch.equal(ops.apply_rope(view, cos, sin, pos_offset=pos_offset),
                           want)


@gpu
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pos_offset", [0, 64])
def test_qkv_grad_pack_matches_rope_bwd_cat_transpose(D, pos_offset):
    from prime_amd import ops

    cos, sin = _tables(D)
    dq = _rand(_B, _S, _H, D, seed=6, shift=0.2)
    dk = _rand(_B, _S, _HKV, D, seed=7, shift=-0.1)
    dv = _rand(_B, _S, _HKV, D, seed=8, shift=0.05)

    def rope_bwd(g):
        x = torch.zeros_like(g).requires_grad_(True)
        ops.apply_rope(x, cos, sin, pos_offset=pos_offset).backward(g)
        return x.grad

    M = _B * _S
    want = torch.cat([rope_bwd(dq).view(M, -1), rope_bwd(dk).view(M, -1),
                      dv.view(M, -1)], dim=1)
    dqkv, dqkvt = ops.qkv_grad_pack(dq, dk, dv, cos, sin, pos_offset)
    assert torch.equal(dqkv, want)
    assert torch.equal(dqkvt, want.t().contiguous())


# ------------------------------------------ fused functions vs composition
@pytest.fixture
def tuned():
    from prime_amd import ops

    ops.set_linear_fp8(False)  # the fused paths are bf16-only
    ops.set_linear_tuned(True)
    yield ops
    ops.set_linear_tuned(False)


@gpu
def test_gateup_swiglu_matches_composition(tuned):
    """GEMM operands are identical on both sides and hipBLASLt reproduces
    bitwise across calls on this stack, so: torch.equal."""
    ops = tuned
    M, K, I = 4096, 512, 512
    x = _rand(M, K, seed=10, shift=0.1).requires_grad_(True)
    w = _rand(2 * I, K, seed=11, scale=0.05, shift=0.01).requires_grad_(True)
    dout = _rand(M, I, seed=12, shift=-0.1)
    xr = x.detach().clone().requires_grad_(True)
    wr = w.detach().clone().requires_grad_(True)

    assert ops.functional._fused_layout_ok(x, w)
    y = ops.gateup_swiglu(x, w)
    assert type(y.grad_fn).__name__.startswith("_GateUpSwiGLU")
    y.backward(dout)
    yr = ops.swiglu(ops.tuned_linear(xr, wr))
    yr.backward(dout)
    assert torch.equal(y, yr)
    assert torch.equal(x.grad, xr.grad)
    assert torch.equal(w.grad, wr.grad)


@gpu
def test_qkv_rope_matches_composition(tuned):
    """Same argument as test_gateup_swiglu_matches_composition."""
    ops = tuned
    B, S, K, H, Hkv, D = 2, 2048, 512, 4, 2, 128
    C = (H + 2 * Hkv) * D
    cos, sin = _tables(D, rows=S)
    x = _rand(B, S, K, seed=13, shift=0.1).requires_grad_(True)
    w = _rand(C, K, seed=14, scale=0.05, shift=0.01).requires_grad_(True)
    gq = _rand(B, S, H, D, seed=15, shift=0.1)
    gk = _rand(B, S, Hkv, D, seed=16, shift=-0.1)
    gv = _rand(B, S, Hkv, D, seed=17, shift=0.05)
    xr = x.detach().clone().requires_grad_(True)
    wr = w.detach().clone().requires_grad_(True)

    q, k, v = ops.qkv_rope(x, w, cos, sin, H, Hkv, D)
    assert type(q.grad_fn).__name__.startswith("_QkvRope")
    assert not v.is_contiguous()  # a view of the packed projection output
    torch.autograd.backward([q, k, v], [gq, gk, gv])

    qkv = ops.tuned_linear(xr, wr)
    q2, k2, v2 = qkv.split([H * D, Hkv * D, Hkv * D], dim=-1)
    q2 = ops.apply_rope(q2.view(B, S, H, D), cos, sin)
    k2 = ops.apply_rope(k2.view(B, S, Hkv, D), cos, sin)
    v2 = v2.view(B, S, Hkv, D)
    torch.autograd.backward([q2, k2, v2], [gq, gk, gv])

    assert torch.equal(q, q2) and torch.equal(k, k2) and torch.equal(v, v2)
    assert torch.equal(x.grad, xr.grad)
    assert torch.equal(w.grad, wr.grad)


# ------------------------------------------------------------ direct wgrad
@gpu
def test_cross_entropy_small_vocab_is_finite():
    """V = 512 leaves most of the CE block's 256 threads without a column;
    merging two such empty partials used to produce NaN (the model below
    has this vocab). fp32 reference on the same bf16 logits; 1e-3 covers
    the kernel's fast exp/log over 512 terms with room to spare."""
    from prime_amd import ops

    logits = _rand(192, 512, seed=30, scale=2.0, shift=0.3).requires_grad_(True)
    g = torch.Generator().manual_seed(31)
    tgt = torch.randint(0, 512, (192,), generator=g).cuda()
    loss = ops.cross_entropy(logits, tgt)
    loss.backward()
    ref_logits = logits.detach().float().requires_grad_(True)
    want = torch.nn.functional.cross_entropy(ref_logits, tgt)
    want.backward()
    assert torch.isfinite(loss) and torch.isfinite(logits.grad.float()).all()
    torch.testing.assert_close(loss.float(), want, atol=1e-3, rtol=1e-3)
    # bf16 gradient of magnitude <= 1/192: half an ulp of that is 2e-5
    torch.testing.assert_close(logits.grad.float(), ref_logits.grad,
                               atol=4e-5, rtol=1e-2)


def _small_model(**kw):
    from prime_amd.models import build_model

    torch.manual_seed(0)
    m = build_model("llama_test", dim=256, n_heads=4, n_kv_heads=2,
                    intermediate=512, vocab_size=512, max_seq=2048, **kw)
    m = m.to("cuda", dtype=torch.bfloat16)
    m.reset_rope("cuda")
    return m


def _batch():
    g = torch.Generator().manual_seed(21)
    x = torch.randint(0, 512, (2, 2048), generator=g).cuda()
    y = torch.randint(0, 512, (2, 2048), generator=g).cuda()
    return x, y


@pytest.fixture
def wgrad_switch(tuned):
    yield tuned
    tuned.set_direct_wgrad(False)


def _two_backwards(flat, model, on, ops):
    """zero_grad + backward, then a second backward without zero_grad;
    returns flat_grad after each."""
    x, y = _batch()
    ops.set_direct_wgrad(on)
    flat.zero_grad()
    model.loss(x, y).backward()
    if on:  # every registered weight saw its first gradient of the step
        assert flat._direct_step and not any(s[1] for s in flat._slots)
    flat.finalize_grads()
    g1 = flat.flat_grad.clone()
    model.loss(x, y).backward()
    flat.finalize_grads()
    return g1, flat.flat_grad.clone()


@gpu
@pytest.mark.parametrize("tie", [False, True])
def test_direct_wgrad_matches_autograd_accumulate(wgrad_switch, tie):
    from prime_amd.parallel.flat import FlatParamSpace

    ops = wgrad_switch
    kw = {"tie_embeddings": True} if tie else {}
    m_on, m_off = _small_model(**kw), _small_model(**kw)
    f_on, f_off = FlatParamSpace(m_on), FlatParamSpace(m_off)
    assert torch.equal(f_on.flat_w, f_off.flat_w)
    names = {n for n, _ in f_on.params}
    n_direct = len(f_on.direct_ranges)
    if tie:
        assert "lm_head.weight" not in names
        o, k, _ = f_on.offsets["tok_embeddings.weight"]
        assert all(b <= o or a >= o + k for a, b in f_on.direct_ranges)
        assert n_direct == 4 * len(m_on.layers)
    else:
        assert n_direct == 4 * len(m_on.layers) + 1
    # stale values in the ranges zero_grad() skips must never survive
    f_on.flat_grad.fill_(3.0)
    on1, on2 = _two_backwards(f_on, m_on, True, ops)
    off1, off2 = _two_backwards(f_off, m_off, False, ops)
    assert torch.equal(on1, off1)
    assert torch.equal(on2, off2)
    assert float(off1.float().abs().sum()) > 0
    assert not torch.equal(off1, off2)


@gpu
def test_direct_wgrad_untouched_weight_reads_zero(wgrad_switch):
    from prime_amd.parallel.flat import FlatParamSpace

    ops = wgrad_switch
    m = _small_model()
    flat = FlatParamSpace(m)
    x, _ = _batch()
    ops.set_direct_wgrad(True)
    flat.flat_grad.fill_(3.0)
    flat.zero_grad()
    m(x).float().sum().backward()  # lm_head stays out of the graph
    flat.finalize_grads()
    o, k, _ = flat.offsets["lm_head.weight"]
    assert float(flat.flat_grad[o : o + k].float().abs().sum()) == 0.0
    o, k, _ = flat.offsets["layers.0.mlp.w_gateup.weight"]
    assert float(flat.flat_grad[o : o + k].float().abs().sum()) > 0.0
    assert not bool((flat.flat_grad == 3.0).all())


# ----------------------------------------------------------------- CPU
def test_zero_and_direct_ranges_partition_flat_space():
    """zero_grad()'s ranges plus the registered weight ranges cover
    [0, numel_padded) exactly once; tied weights are never registered."""
    from prime_amd.models import build_model
    from prime_amd.parallel.flat import FlatParamSpace

    for tie in (False, True):
        torch.manual_seed(0)
        m = build_model("llama_test", tie_embeddings=tie)
        flat = FlatParamSpace(m)
        spans = sorted(flat.zero_ranges + flat.direct_ranges)
        assert spans[0][0] == 0 and spans[-1][1] == flat.numel_padded
        for (a0, b0), (a1, b1) in zip(spans, spans[1:]):
            assert a0 < b0 and b0 == a1
        linear = {"wqkv", "wo", "w_gateup", "w_down"} | (set() if tie else {"lm_head"})
        want = sorted(
            (o, o + k) for n, (o, k, _) in flat.offsets.items()
            if n.split(".")[-2] in linear)
        assert flat.direct_ranges == want
        emb = flat.offsets["tok_embeddings.weight"]
        assert all(b <= emb[0] or a >= emb[0] + emb[1]
                   for a, b in flat.direct_ranges)
