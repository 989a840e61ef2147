"""Edge-shape GPU tests of the memory-bound and fp8 kernels against the
float64 oracles of tests/kernel_oracles.py: shapes that leave threads idle,
give a thread more than one vector, are no multiple of a tile, or cross the
grid cap of 2048 blocks of 256 threads; null optional operands; saturated
and degenerate inputs. The tolerances and their derivations live next to the
oracles; tests/test_kernel_oracles_cpu.py shows that the helpers reject
subtly wrong results."""
import pytest
import torch

from tests import kernel_oracles as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

NORM = ko.norm_cases()
ROPE = ko.rope_cases()
SWIGLU = ko.swiglu_cases()
CE = ko.ce_cases()
ADAMW = ko.adamw_cases()
INT8 = ko.int8_cases()
OUTER = ko.outer_cases()


def _ids(cases):
    return [c[0] for c in cases]


def _d(t):
    return None if t is None else t.to(DEV)


def _raw():
    from prime_amd.ops._lib import check, lib, ptr, stream_of

    return check, lib(), ptr, stream_of


# ------------------------------------------------- rmsnorm / add_rmsnorm
@pytest.mark.parametrize("name,c", NORM, ids=_ids(NORM))
def test_rmsnorm_edges(name, c):
    from prime_amd import ops

    o = ko.oracle_norm(c["x"], c["w"], c["dy"])
    x = _d(c["x"]).requires_grad_(True)
    w = _d(c["w"]).requires_grad_(True)
    y = ops.rmsnorm(x, w, ko.NORM_EPS)
    y.backward(_d(c["dy"]))
    # rstd is reached only through the library call
    check, lib, ptr, stream_of = _raw()
    R, D = c["x"].shape
    y2 = torch.empty_like(y)
    rstd = torch.empty(R, device=DEV, dtype=torch.float32)
    check(lib.prime_rmsnorm_fwd(stream_of(y2), ptr(x), ptr(w), ptr(y2), ptr(rstd),
                                R, D, ko.NORM_EPS), "rmsnorm_fwd")
    assert torch.equal(y2, y.detach())
    ko.assert_norm_fwd(o, y, rstd=rstd, what=f"rmsnorm {name}")
    ko.assert_norm_bwd(o, x.grad, w.grad, what=f"rmsnorm {name}")


@pytest.mark.parametrize("name,c", NORM, ids=_ids(NORM))
def test_add_rmsnorm_edges(name, c):
    from prime_amd import ops

    o = ko.oracle_norm(c["x"], c["w"], c["dy"], res=c["res"], ds=c["ds"])
    x = _d(c["x"]).requires_grad_(True)
    res = _d(c["res"]).requires_grad_(True)
    w = _d(c["w"]).requires_grad_(True)
    y, s = ops.fused_add_rmsnorm(x, res, w, ko.NORM_EPS)
    torch.autograd.backward([y, s], [_d(c["dy"]), _d(c["ds"])])
    check, lib, ptr, stream_of = _raw()
    R, D = c["x"].shape
    s2, y2 = torch.empty_like(s), torch.empty_like(y)
    rstd = torch.empty(R, device=DEV, dtype=torch.float32)
    check(lib.prime_add_rmsnorm_fwd(stream_of(y2), ptr(x), ptr(res), ptr(w), ptr(s2),
                                    ptr(y2), ptr(rstd), R, D, ko.NORM_EPS), "add_rmsnorm_fwd")
    assert torch.equal(y2, y.detach()) and torch.equal(s2, s.detach())
    ko.assert_norm_fwd(o, y, s=s, rstd=rstd, what=f"add_rmsnorm {name}")
    ko.assert_norm_bwd(o, x.grad, w.grad, what=f"add_rmsnorm {name}")
    assert torch.equal(res.grad, x.grad)


@pytest.mark.parametrize("name", ["33x264", "5x2056"])
def test_add_rmsnorm_null_operands(name):
    """res=None and an absent ds_res reach the kernels as null pointers."""
    from prime_amd import ops

    c = dict(NORM)[name]
    # no residual: s is x itself
    o = ko.oracle_norm(c["x"], c["w"], c["dy"], res=None, ds=c["ds"])
    x = _d(c["x"]).requires_grad_(True)
    w = _d(c["w"]).requires_grad_(True)
    y, s = ops.fused_add_rmsnorm(x, None, w, ko.NORM_EPS)
    torch.autograd.backward([y, s], [_d(c["dy"]), _d(c["ds"])])
    ko.assert_norm_fwd(o, y, s=s, what="add_rmsnorm res=None")
    ko.assert_norm_bwd(o, x.grad, w.grad, what="add_rmsnorm res=None")
    # only y used downstream: no gradient arrives for s
    o = ko.oracle_norm(c["x"], c["w"], c["dy"], res=c["res"], ds=None)
    x = _d(c["x"]).requires_grad_(True)
    res = _d(c["res"]).requires_grad_(True)
    w = _d(c["w"]).requires_grad_(True)
    y, s = ops.fused_add_rmsnorm(x, res, w, ko.NORM_EPS)
    y.backward(_d(c["dy"]))
    ko.assert_norm_bwd(o, x.grad, w.grad, what="add_rmsnorm ds_res absent")
    assert torch.equal(res.grad, x.grad)


# -------------------------------------------------------------------- RoPE
@pytest.mark.parametrize("name,c", ROPE, ids=_ids(ROPE))
def test_rope_edges(name, c):
    from prime_amd import ops

    x, dy, off = c["x"], c["dy"], c["off"]
    cos, sin = _d(c["cos"]), _d(c["sin"])
    assert x.shape[1] + off <= cos.shape[0]      # never a position past the table
    xg = _d(x).requires_grad_(True)
    y = ops.apply_rope(xg, cos, sin, pos_offset=off)
    y.backward(_d(dy))
    ko.assert_rope(y, x, c["cos"], c["sin"], off, what=f"rope fwd {name}")
    ko.assert_rope(xg.grad, dy, c["cos"], c["sin"], off, -1.0, what=f"rope bwd {name}")
    if off:
        pos = torch.tensor([off], device=DEV, dtype=torch.int32)
        y_dev = ops.apply_rope(_d(x), cos, sin, pos_offset=0, pos_dev=pos)
        assert torch.equal(y_dev, y.detach()), "pos_dev differs from pos_offset"


# ------------------------------------------------------------------ SwiGLU
@pytest.mark.parametrize("name,c", SWIGLU, ids=_ids(SWIGLU))
def test_swiglu_edges(name, c):
    from prime_amd import ops

    o = ko.oracle_swiglu(c["gu"], c["dout"])
    gu = _d(c["gu"]).requires_grad_(True)
    out = ops.swiglu(gu)
    out.backward(_d(c["dout"]))
    ko.assert_swiglu(o, out=out, dgu=gu.grad, what=f"swiglu {name}")


# ----------------------------------------------------------- cross entropy
@pytest.mark.parametrize("name,c", CE, ids=_ids(CE))
def test_cross_entropy_edges(name, c):
    from prime_amd import ops

    z, tgt = c["z"], c["tgt"]
    R, V = z.shape
    o = ko.oracle_ce(z, tgt)
    zg = _d(z).requires_grad_(True)
    loss = ops.cross_entropy(zg, _d(tgt))
    (ko.CE_GRAD_OUT * loss).backward()
    with torch.no_grad():
        loss_ng = ops.cross_entropy(_d(z), _d(tgt))
    assert torch.equal(loss_ng, loss.detach()), "no_grad loss bits differ"
    # the per-row loss is reached only through the library call
    check, lib, ptr, stream_of = _raw()
    zd, t32 = _d(z), _d(tgt).to(torch.int32)
    row = torch.empty(R, device=DEV, dtype=torch.float32)
    check(lib.prime_cross_entropy(stream_of(zd), ptr(zd), ptr(t32), ptr(row), ptr(zd),
                                  R, V, 1.0, ko.CE_IGNORE, 0), "cross_entropy")
    ko.assert_ce(o, row=row, mean=loss, grad=zg.grad, what=f"ce {name}")
    if "all-ignored" in name:
        assert float(loss) == 0.0 and int(torch.count_nonzero(zg.grad)) == 0


# ------------------------------------------------------- AdamW, grad_sqnorm
@pytest.mark.parametrize("name,c", ADAMW, ids=_ids(ADAMW))
def test_adamw_edges(name, c):
    from prime_amd import ops

    hp = dict(ko.ADAMW_HP, wd=c["wd"], step=c["step"])
    o = ko.oracle_adamw(c["p32"], c["g"], c["m"], c["v"], gscale=c["gscale"], **hp)
    p32, g, m, v = _d(c["p32"]).clone(), _d(c["g"]), _d(c["m"]).clone(), _d(c["v"]).clone()
    p16 = torch.zeros_like(p32, dtype=torch.bfloat16)
    gs = None if c["gscale"] is None else torch.tensor([c["gscale"]], device=DEV)
    ops.fused_adamw(p32, p16, g, m, v, gscale=gs, **hp)
    ko.assert_adamw(o, p32, p16, m, v, what=f"adamw {name}")
    if c["step"] == 1:
        sq = torch.zeros(1, device=DEV)
        ops.grad_sqnorm(g, sq)
        ko.assert_sqnorm(sq, c["g"], what=f"grad_sqnorm N={g.numel()}")


# ------------------------------------------------------------ int8 quant
@pytest.mark.parametrize("name,c", INT8, ids=_ids(INT8))
def test_int8_edges(name, c):
    from prime_amd import ops

    x = c["x"]
    q, s = ops.quant_int8(_d(x))
    ko.assert_int8(q, s, x, what=f"quant_int8 {name}")
    if s.numel() > 2:   # the all-zero block
        assert float(s[1]) == 0.0 and int(torch.count_nonzero(q[ko.QBLK:2 * ko.QBLK])) == 0
    out = torch.full((x.numel(),), float("nan"), device=DEV)
    ops.dequant_int8(q, s, out)
    ko.assert_dequant(out, q, s, what=f"dequant_int8 {name}")
    acc = _d(c["dst"]).clone()
    ops.dequant_int8(q, s, acc, accumulate=True)
    ko.assert_dequant(acc, q, s, dst=c["dst"], what=f"dequant_int8 {name}")


# ------------------------------------------------ nesterov outer, pseudograd
@pytest.mark.parametrize("name,c", OUTER, ids=_ids(OUTER))
def test_outer_edges(name, c):
    from prime_amd import ops

    o = ko.oracle_nesterov(c["theta"], c["buf"], c["delta"], **ko.OUTER_HP)
    N = c["theta"].numel()
    delta = torch.full((N,), float("nan"), device=DEV)
    ops.pseudograd(_d(c["theta"]), _d(c["master"]), delta)
    ko.assert_pseudograd(delta, c["theta"], c["master"], what=f"pseudograd {name}")
    theta, master, buf = _d(c["theta"]).clone(), _d(c["master"]).clone(), _d(c["buf"]).clone()
    inner16 = torch.zeros(N, device=DEV, dtype=torch.bfloat16)
    ops.nesterov_outer(theta, master, inner16, buf, _d(c["delta"]), **ko.OUTER_HP)
    ko.assert_nesterov(o, theta, master, inner16, buf, what=f"nesterov {name}")


# --------------------------------------------------------------- transpose
@pytest.mark.parametrize("shape", ko.TRANSPOSE_SHAPES, ids=str)
def test_transpose_bshd_edges(shape):
    from prime_amd.ops.functional import transpose_bshd

    B, S, H, D = shape
    g = ko.gen(800)
    x = ko.bf(torch.randn(B, S, H, D, generator=g))
    ko.assert_transpose(transpose_bshd(_d(x)), x, what="dense")
    # q-like view of a packed buffer: heads 1 .. H of 2H + 1
    big = ko.bf(torch.randn(B, S, 2 * H + 1, D, generator=g))
    view = _d(big)[:, :, 1:H + 1]
    assert not view.is_contiguous()
    ko.assert_transpose(transpose_bshd(view), big[:, :, 1:H + 1], what="packed view")
    # batch stride different from S * ss: the first S of S + 64 positions
    big = ko.bf(torch.randn(B, S + 64, H, D, generator=g))
    view = _d(big)[:, :S]
    assert B == 1 or view.stride(0) != S * view.stride(1)
    ko.assert_transpose(transpose_bshd(view), big[:, :S], what="batch-strided view")


# --------------------------------------------------------------------- fp8
@pytest.fixture
def fp8_state():
    from prime_amd import ops

    ops.set_linear_fp8(False)
    try:
        yield
    finally:
        ops.set_linear_fp8(False)


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("prev_kind", ["small", "large", "zero"])
@pytest.mark.parametrize("n", ko.FP8_NS)
def test_quant_fp8_delayed_edges(n, prev_kind, fmt, fp8_state):
    """prime_quant_fp8 through _quant_act_fp8 with a seeded site: bytes,
    amax_next and sinv are exact; saturation gives +-fmax, never NaN."""
    from prime_amd.ops import functional as F

    x = ko.fp8_values((n,), 900)
    prev = ko.fp8_prev(x, prev_kind)
    o = ko.oracle_fp8(x, prev, fmt)
    site = ("edge-test", n, prev_kind, fmt)
    old = torch.tensor([prev], device=DEV, dtype=torch.float32)
    F._FP8_ACT[site] = {"amax": old, "next": torch.full((1,), 7.0, device=DEV),
                        "sinv": torch.full((1,), float("nan"), device=DEV)}
    x8, sinv = F._quant_act_fp8(_d(x), site, e5m2=(fmt == "e5m2"))
    st = F._FP8_ACT[site]
    assert st["next"] is old          # the states swapped: amax now holds this call's
    ko.assert_fp8(o, fmt, x8, sinv=sinv, amax_next=st["amax"], what=f"quant_fp8 n={n}")


def _tq_direct(x_view, prev, fmt):
    check, lib, ptr, stream_of = _raw()
    M, C = x_view.shape
    x8 = torch.zeros(C, M, device=DEV, dtype=ko.FP8[fmt][0])
    amax = torch.tensor([prev], device=DEV, dtype=torch.float32)
    nxt = torch.zeros(1, device=DEV)
    sinv = torch.full((1,), float("nan"), device=DEV)
    check(lib.prime_transpose_fp8(stream_of(x_view), ptr(x_view), ptr(x8), 1, M, C // 128, 128,
                                  x_view.stride(0) * M, x_view.stride(0), 128,
                                  ptr(amax), ptr(nxt), ptr(sinv), 1 if fmt == "e5m2" else 0),
          "transpose_fp8")
    return x8, sinv, nxt


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("shape", ko.FP8_TQ_SHAPES, ids=str)
def test_transpose_fp8_edges(shape, fmt, fp8_state, monkeypatch):
    """The opt-in fused transpose + quantize kernel, directly (dense and a
    source view with row stride above C) and through _transpose_quant_fp8."""
    from prime_amd.ops import functional as F

    M, C = shape
    x = ko.fp8_values(shape, 910)
    for kind in ("small", "large", "zero"):
        prev = ko.fp8_prev(x, kind)
        o = ko.oracle_fp8(x.t().contiguous(), prev, fmt)
        x8, sinv, nxt = _tq_direct(_d(x), prev, fmt)
        ko.assert_fp8(o, fmt, x8, sinv=sinv, amax_next=nxt, what=f"transpose_fp8 {kind}")
    wide = ko.fp8_values((M, C + 64), 911)
    view = _d(wide)[:, :C]
    prev = ko.fp8_prev(wide[:, :C], "small")
    o = ko.oracle_fp8(wide[:, :C].t().contiguous(), prev, fmt)
    x8, sinv, nxt = _tq_direct(view, prev, fmt)
    ko.assert_fp8(o, fmt, x8, sinv=sinv, amax_next=nxt, what="transpose_fp8 strided")
    # through the wrapper: the bootstrap call seeds amax with max|x1|, the
    # second call runs the fused kernel with it
    monkeypatch.setenv("PRIME_AMD_FUSED_TQ", "1")
    x1 = ko.fp8_values(shape, 912)
    site = ("edge-tq", M, C, fmt)
    F._transpose_quant_fp8(_d(x1), site, e5m2=(fmt == "e5m2"))
    x8, sinv = F._transpose_quant_fp8(_d(x), site, e5m2=(fmt == "e5m2"))
    o = ko.oracle_fp8(x.t().contiguous(), float(x1.float().abs().max()), fmt)
    ko.assert_fp8(o, fmt, x8, sinv=sinv, amax_next=F._FP8_ACT[site]["amax"],
                  what="transpose_fp8 via wrapper")


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("shape", ko.FP8_ROW_SHAPES, ids=str)
def test_rowwise_fp8_edges(shape, fmt):
    from prime_amd.ops.functional import _quant_rowwise_fp8

    x = ko.fp8_values(shape, 920)
    x[shape[0] // 2] = 0       # a zero row: bytes zero, sinv = 1e-12 / fmax
    o = ko.oracle_fp8_rowwise(x, fmt)
    x8, sinv = _quant_rowwise_fp8(_d(x), e5m2=(fmt == "e5m2"))
    ko.assert_fp8(o, fmt, x8, sinv=sinv, what=f"rowwise fp8 {shape}")


# ------------------------------------------------------------- empty inputs
def test_empty_inputs_give_empty_outputs():
    """Every op whose wrapper can be handed an empty tensor returns empty
    outputs (and zero reductions) without an error."""
    from prime_amd import ops
    from prime_amd.ops import reference as ref
    from prime_amd.ops.functional import _quant_rowwise_fp8, transpose_bshd

    e = torch.empty(0, 64, device=DEV, dtype=torch.bfloat16)
    w = torch.ones(64, device=DEV, dtype=torch.bfloat16)
    assert ops.rmsnorm(e, w).shape == (0, 64)
    y, s = ops.fused_add_rmsnorm(e, e, w)
    assert y.shape == s.shape == (0, 64)
    assert ops.swiglu(e).shape == (0, 32)
    cos, sin = ref.rope_tables(64, 8, device=DEV)
    assert ops.apply_rope(e.view(0, 4, 1, 64), cos, sin).shape == (0, 4, 1, 64)
    loss = ops.cross_entropy(e, torch.empty(0, device=DEV, dtype=torch.long))
    assert float(loss) == 0.0
    q, sc = ops.quant_int8(torch.empty(0, device=DEV))
    assert q.numel() == 0 and sc.numel() == 0
    ops.dequant_int8(q, sc, torch.empty(0, device=DEV))
    for e5m2 in (False, True):
        x8, sinv = _quant_rowwise_fp8(e, e5m2=e5m2)
        assert x8.shape == (0, 64) and sinv.shape == (0, 1)
    assert transpose_bshd(torch.empty(0, 64, 2, 64, device=DEV, dtype=torch.bfloat16)).shape \
        == (0, 2, 64, 64)
    sq = torch.zeros(1, device=DEV)
    ops.grad_sqnorm(e.view(-1), sq)
    torch.cuda.synchronize()
    assert float(sq) == 0.0
