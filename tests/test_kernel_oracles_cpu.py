"""The assert helpers of tests/kernel_oracles.py bite, shown without a GPU.

For every op: (1) the oracle's own result, rounded to the kernel's output
dtype, passes the helper at every shape the GPU lane runs; (2) the op's CPU
path, where it has one, passes too; (3) named wrong results, built from the
oracle's intermediates, are rejected."""
import pytest
import torch

from prime_amd import ops
from prime_amd.ops import reference as ref
from tests import kernel_oracles as ko

bf = ko.bf

NORM = ko.norm_cases()
ROPE = ko.rope_cases()
SWIGLU = ko.swiglu_cases()
CE = ko.ce_cases()
ADAMW = ko.adamw_cases()
INT8 = ko.int8_cases()
OUTER = ko.outer_cases()


def _ids(cases):
    return [c[0] for c in cases]


def _case(cases, name):
    return dict(cases)[name]


# ------------------------------------------------- rmsnorm / add_rmsnorm
@pytest.mark.parametrize("name,c", NORM, ids=_ids(NORM))
@pytest.mark.parametrize("add", [False, True], ids=["rmsnorm", "add_rmsnorm"])
def test_norm_oracle_and_cpu_path_pass(name, c, add):
    res, ds = (c["res"], c["ds"]) if add else (None, None)
    o = ko.oracle_norm(c["x"], c["w"], c["dy"], res=res, ds=ds)
    ko.assert_norm_fwd(o, bf(o["y"]), s=o["s"], rstd=o["rstd"].float())
    ko.assert_norm_bwd(o, bf(o["dx"]), bf(o["dw"].float()))
    # CPU path: fp32 reference arithmetic, one rounding to bf16
    x = c["x"].clone().requires_grad_(True)
    w = c["w"].clone().requires_grad_(True)
    if add:
        r = res.clone().requires_grad_(True)
        y, s = ops.fused_add_rmsnorm(x, r, w)
        torch.autograd.backward([y, s], [c["dy"], ds])
        # the CPU path takes rstd from the stored bf16 s, the kernel from the
        # fp32 sum before that rounding; with few columns the two differ by
        # more than the fp32 allowance, so only s is held to the fused
        # oracle and the rest to the oracle of rmsnorm(s)
        ko.check_equal(s, o["s"], "cpu add_rmsnorm: s")
        o = ko.oracle_norm(o["s"], c["w"], c["dy"], ds=ds)
        ko.assert_norm_fwd(o, y)
        assert torch.equal(r.grad, x.grad)
    else:
        y = ops.rmsnorm(x, w)
        y.backward(c["dy"])
        ko.assert_norm_fwd(o, y)
    ko.assert_norm_bwd(o, x.grad, w.grad)


def test_add_norm_optional_operands():
    c = _case(NORM, "33x264")
    o = ko.oracle_norm(c["x"], c["w"], c["dy"], res=None, ds=c["ds"])
    ko.assert_norm_fwd(o, bf(o["y"]), s=o["s"], rstd=o["rstd"].float())
    ko.assert_norm_bwd(o, bf(o["dx"]), bf(o["dw"].float()))
    assert torch.equal(o["s"], c["x"])
    o = ko.oracle_norm(c["x"], c["w"], c["dy"], res=c["res"], ds=None)
    ko.assert_norm_bwd(o, bf(o["dx"]), bf(o["dw"].float()))


@pytest.mark.parametrize("name", ["33x264", "33x264-spread", "5x2056", "1029x264"])
def test_norm_wrong_results_rejected(name):
    c = _case(NORM, name)
    x, res, w, dy, ds = c["x"], c["res"], c["w"], c["dy"], c["ds"]
    o = ko.oracle_norm(x, w, dy, res=res, ds=ds)
    D = x.shape[-1]
    s32 = x.float() + res.float()
    sd, wd = o["s"].double(), w.double()

    def fwd_rej(y=None, rstd=None):
        return ko.rejects(ko.assert_norm_fwd, o, bf(o["y"] if y is None else y),
                          s=o["s"], rstd=(o["rstd"] if rstd is None else rstd).float())

    # eps dropped: always seen in rstd, and in y where eps matters
    r_noeps = s32.double().pow(2).mean(-1).rsqrt()
    assert fwd_rej(rstd=r_noeps)
    if "spread" in name:
        assert ko.rejects(ko.assert_norm_fwd, o, bf(sd * r_noeps.unsqueeze(-1) * wd))
    # the last 8 columns left out of the mean
    r_short = (s32.double()[:, :-8].pow(2).sum(-1) / D + ko.f32(ko.NORM_EPS)).rsqrt()
    assert fwd_rej(rstd=r_short)
    if 4 / D > 2 * ko.RTOL_BF16:   # rstd moves by 4 / D: beyond D = 256 y cannot show it
        assert ko.rejects(ko.assert_norm_fwd, o, bf(sd * r_short.unsqueeze(-1) * wd))
    # w shifted by one vector
    assert fwd_rej(y=sd * o["rstd"].unsqueeze(-1) * wd.roll(8))
    # last row of y stale
    y = o["y"].clone()
    y[-1] = y[0]
    assert fwd_rej(y=y)
    # s not rounded from the fp32 sum
    assert ko.rejects(ko.assert_norm_fwd, o, bf(o["y"]), s=x)

    def bwd_rej(dx=None, dw=None):
        return ko.rejects(ko.assert_norm_bwd, o, bf(o["dx"] if dx is None else dx),
                          bf((o["dw"] if dw is None else dw).float()))

    rs = o["rstd"].unsqueeze(-1)
    # dx projection term x0.9
    assert bwd_rej(dx=rs * (o["dyw"] - 0.9 * o["shat"] * o["mean_dot"]) + ds.double())
    # ds_res not added
    assert bwd_rej(dx=o["dx"] - ds.double())
    # dw missing the last row
    assert bwd_rej(dw=o["dw"] - o["dw_term"][-1])
    # dw from the un-normalized input
    assert bwd_rej(dw=(dy.double() * sd).sum(0))


# -------------------------------------------------------------------- RoPE
@pytest.mark.parametrize("name,c", ROPE, ids=_ids(ROPE))
def test_rope_oracle_and_cpu_path_pass(name, c):
    x, dy, cos, sin, off = c["x"], c["dy"], c["cos"], c["sin"], c["off"]
    ko.assert_rope(bf(ko.oracle_rope(x, cos, sin, off)[0]), x, cos, sin, off)
    ko.assert_rope(bf(ko.oracle_rope(dy, cos, sin, off, -1.0)[0]), dy, cos, sin, off, -1.0)
    xg = x.clone().requires_grad_(True)
    y = ops.apply_rope(xg, cos, sin, pos_offset=off)
    y.backward(dy)
    ko.assert_rope(y, x, cos, sin, off)
    ko.assert_rope(xg.grad, dy, cos, sin, off, -1.0)


def test_rope_wrong_results_rejected():
    c = _case(ROPE, "2x37x3x64-off7")
    x, dy, cos, sin, off = c["x"], c["dy"], c["cos"], c["sin"], c["off"]
    B, S, H, D = x.shape
    # pos_offset ignored
    assert ko.rejects(ko.assert_rope, bf(ko.oracle_rope(x, cos, sin, 0)[0]), x, cos, sin, off)
    # position not taken modulo S for b > 0 (needs a longer table to build)
    cl, sl = ref.rope_tables(D, B * S + 8)
    pos = (torch.arange(B * S) + off).view(B, S)
    assert ko.rejects(ko.assert_rope, bf(ko.oracle_rope(x, cl, sl, off, pos=pos)[0]),
                      x, cos, sin, off)
    # backward with the forward sign
    assert ko.rejects(ko.assert_rope, bf(ko.oracle_rope(dy, cos, sin, off, 1.0)[0]),
                      dy, cos, sin, off, -1.0)
    # interleaved instead of half-split pairing
    assert ko.rejects(ko.assert_rope,
                      bf(ko.oracle_rope(x, cos, sin, off, interleaved=True)[0]),
                      x, cos, sin, off)
    # heads and positions confused: position taken from row % S
    rows = torch.arange(B * S * H).view(B, S, H)
    wrong = torch.stack([ko.oracle_rope(x[:, :, h:h + 1], cos, sin, 0,
                                        pos=rows[:, :, h] % S + off)[0] for h in range(H)], 2)
    assert ko.rejects(ko.assert_rope, bf(wrong.squeeze(3)), x, cos, sin, off)


# ------------------------------------------------------------------ SwiGLU
@pytest.mark.parametrize("name,c", SWIGLU, ids=_ids(SWIGLU))
def test_swiglu_oracle_and_cpu_path_pass(name, c):
    o = ko.oracle_swiglu(c["gu"], c["dout"])
    assert torch.isfinite(o["out"]).all() and torch.isfinite(o["dgu"]).all()
    ko.assert_swiglu(o, out=bf(o["out"]), dgu=bf(o["dgu"]))
    gu = c["gu"].clone().requires_grad_(True)
    out = ops.swiglu(gu)
    out.backward(c["dout"])
    ko.assert_swiglu(o, out=out, dgu=gu.grad)


@pytest.mark.parametrize("name", ["65x520", "saturated"])
def test_swiglu_wrong_results_rejected(name):
    c = _case(SWIGLU, name)
    o = ko.oracle_swiglu(c["gu"], c["dout"])
    # gate and up swapped
    sw = ko.oracle_swiglu(c["gu"], c["dout"], swapped=True)
    assert ko.rejects(ko.assert_swiglu, o, out=bf(sw["out"]))
    # dg without the g * (1 - sigmoid) term
    dg = o["d"] * o["u"] * o["sg"]
    du = o["d"] * o["g"] * o["sg"]
    assert ko.rejects(ko.assert_swiglu, o, dgu=bf(torch.cat([dg, du], -1)))
    # dg and du written to each other's half
    I = dg.shape[-1]
    assert ko.rejects(ko.assert_swiglu, o, dgu=bf(o["dgu"].roll(I, -1)))
    if name == "saturated":
        # a sigmoid that overflows to NaN instead of saturating
        out = o["out"].clone()
        out[o["g"] < -80] = float("nan")
        assert ko.rejects(ko.assert_swiglu, o, out=bf(out))


# ----------------------------------------------------------- cross entropy
@pytest.mark.parametrize("name,c", CE, ids=_ids(CE))
def test_ce_oracle_and_cpu_path_pass(name, c):
    z, tgt = c["z"], c["tgt"]
    o = ko.oracle_ce(z, tgt)
    # as the kernel rounds: bf16(p - onehot), times the bf16 scale, in bf16
    unit = bf((o["p"] - o["onehot"]) * o["valid"].unsqueeze(1))
    grad = bf(unit.double() * o["sc"])
    ko.assert_ce(o, row=o["row"].float(), mean=o["mean"].float(), grad=grad)
    if "all-ignored" in name:
        assert float(o["mean"]) == 0.0 and not bool(o["grad"].any())
        return  # F.cross_entropy returns NaN for an all-ignored batch
    # CPU path (F.cross_entropy on fp32 logits): its gradient is rounded once
    # and uses the unrounded scale, inside the twice-rounded tolerance
    zg = z.clone().requires_grad_(True)
    loss = ops.cross_entropy(zg, tgt)
    (ko.CE_GRAD_OUT * loss).backward()
    ko.assert_ce(o, mean=loss, grad=zg.grad)


@pytest.mark.parametrize("name", ["64x2056", "16x32000", "2053x512"])
def test_ce_wrong_results_rejected(name):
    c = _case(CE, name)
    z, tgt = c["z"], c["tgt"]
    o = ko.oracle_ce(z, tgt)
    R, V = z.shape
    good = bf(o["grad"])
    ko.assert_ce(o, grad=good)
    # non-target gradient zero
    assert ko.rejects(ko.assert_ce, o, grad=bf(o["grad"] * o["onehot"]))
    # ignored row holding 1e-3
    g = good.clone()
    g[3, 17 % V] = 1e-3
    assert ko.rejects(ko.assert_ce, o, grad=g)
    row = o["row"].float().clone()
    row[3] = 1e-3
    assert ko.rejects(ko.assert_ce, o, row=row)
    # mean over R instead of n_valid
    wrong = ko.oracle_ce(z, tgt, mean_over_rows=True)
    assert ko.rejects(ko.assert_ce, o, mean=wrong["mean"].float())
    assert ko.rejects(ko.assert_ce, o, grad=bf(wrong["grad"]))
    # running sum not rescaled when a new maximum arrives (one thread's scan)
    zd = z.double()
    m = torch.full((R,), float("-inf"), dtype=torch.float64)
    s = torch.zeros(R, dtype=torch.float64)
    for j in range(V):
        f = zd[:, j]
        new = f > m
        s = torch.where(new, s + 1.0, s + torch.exp(f - m))
        m = torch.where(new, f, m)
    lse_bad = m + s.log()
    t = torch.where(o["valid"], tgt, torch.zeros_like(tgt))
    row_bad = torch.where(o["valid"], lse_bad - zd.gather(1, t.view(-1, 1)).squeeze(1),
                          torch.zeros(R, dtype=torch.float64))
    assert ko.rejects(ko.assert_ce, o, row=row_bad.float())
    p_bad = torch.exp(zd - lse_bad.unsqueeze(1))
    assert ko.rejects(ko.assert_ce, o,
                      grad=bf((p_bad - o["onehot"]) * o["valid"].unsqueeze(1) * o["sc"]))
    # the -1 placed at column tgt + 1
    shifted = o["onehot"].roll(1, dims=1)
    assert ko.rejects(ko.assert_ce, o,
                      grad=bf((o["p"] - shifted) * o["valid"].unsqueeze(1) * o["sc"]))
    # gradient scaled by an unrounded 1/R-ish scale far from the bf16 one
    assert ko.rejects(ko.assert_ce, o, grad=bf(o["grad"] * 1.02))


# ------------------------------------------------------------------- AdamW
@pytest.mark.parametrize("name,c", ADAMW, ids=_ids(ADAMW))
def test_adamw_oracle_and_reference_pass(name, c):
    hp = dict(ko.ADAMW_HP, wd=c["wd"], step=c["step"], gscale=c["gscale"])
    o = ko.oracle_adamw(c["p32"], c["g"], c["m"], c["v"], **hp)
    p = o["p"].float()
    ko.assert_adamw(o, p, p.bfloat16(), o["m"].float(), o["v"].float())
    # fp32 reference (its gradient is pre-scaled: the kernel scales in fp32)
    p32, m, v = c["p32"].clone(), c["m"].clone(), c["v"].clone()
    g = c["g"].float() * (1.0 if c["gscale"] is None else ko.f32(c["gscale"]))
    ref.adamw_step(p32, g, m, v, ko.ADAMW_HP["lr"], ko.ADAMW_HP["beta1"],
                   ko.ADAMW_HP["beta2"], ko.ADAMW_HP["eps"], c["wd"], c["step"])
    ko.assert_adamw(o, p32, p32.bfloat16(), m, v)
    ko.assert_sqnorm(c["g"].float().pow(2).sum().reshape(1), c["g"])


@pytest.mark.parametrize("name", [n for n in _ids(ADAMW) if n.startswith("N4099")])
def test_adamw_wrong_results_rejected(name):
    c = _case(ADAMW, name)
    hp = dict(ko.ADAMW_HP, wd=c["wd"], step=c["step"], gscale=c["gscale"])
    o = ko.oracle_adamw(c["p32"], c["g"], c["m"], c["v"], **hp)

    def rej(w, p16=None):
        p = w["p"].float()
        return ko.rejects(ko.assert_adamw, o, p, p.bfloat16() if p16 is None else p16,
                          w["m"].float(), w["v"].float())

    assert not rej(o)
    # v without bias correction (1 - beta2^1000 is 1: nothing to see there)
    if c["step"] <= 2:
        assert rej(ko.oracle_adamw(c["p32"], c["g"], c["m"], c["v"], v_bias_correction=False, **hp))
    # tail elements untouched
    tail = 4096
    w = {k: o[k].clone() for k in "pmv"}
    w["p"][tail:], w["m"][tail:], w["v"][tail:] = c["p32"][tail:].double(), c["m"][tail:].double(), c["v"][tail:].double()
    assert rej(w)
    # v alone untouched in the tail
    w = {k: o[k].clone() for k in "pmv"}
    w["v"][tail:] = c["v"][tail:].double()
    assert rej(w)
    # gscale applied to m but not v
    if c["gscale"] is not None:
        assert rej(ko.oracle_adamw(c["p32"], c["g"], c["m"], c["v"], gscale_on_v=False, **hp))
    # decay taken from the updated parameter
    if c["wd"]:
        assert rej(ko.oracle_adamw(c["p32"], c["g"], c["m"], c["v"], decay_from_updated=True, **hp))
    # p16 one bf16 step off in one element
    p16 = o["p"].float().bfloat16()
    p16[5] = (p16[5:6].view(torch.int16) + 1).view(torch.bfloat16)[0]
    assert rej(o, p16=p16)
    # sqnorm missing the scalar tail
    assert ko.rejects(ko.assert_sqnorm, c["g"][:4096].double().pow(2).sum().float().reshape(1), c["g"])


# ------------------------------------------------------------ int8 quant
@pytest.mark.parametrize("name,c", INT8, ids=_ids(INT8))
def test_int8_reference_passes_and_one_ulp_of_inv_stays_inside(name, c):
    x = c["x"]
    q, s = ref.quant_int8_blockwise(x)
    ko.assert_int8(q, s, x)
    N = x.numel()
    nblk = s.numel()
    if nblk > 2:
        assert s[1] == 0 and not bool(q[ko.QBLK:2 * ko.QBLK].any())
        blk = x[2 * ko.QBLK:3 * ko.QBLK]
        assert blk[blk.abs().argmax()] < 0 and int(q[2 * ko.QBLK + 77]) == -127
    # a 1-ulp change of inv moves few codes: the cap is far from the reference
    inv = torch.where(s > 0, 1.0 / s, torch.zeros_like(s))
    for direction in (float("inf"), 0.0):
        inv2 = torch.nextafter(inv, torch.full_like(inv, direction))
        inv2 = torch.where(s > 0, inv2, inv)
        idx = torch.arange(N) // ko.QBLK
        q2 = (x * inv2[idx]).round().clamp(-127, 127).to(torch.int8)
        n_diff = int((q2 != q).sum())
        assert n_diff <= max(1e-4 * N, 1 if N > 1000 else 0), n_diff
        ko.assert_int8(q2, s, x)
    # dequant: exact without accumulate, fp32 class with
    want, _ = ko.oracle_dequant(q, s)
    ko.assert_dequant(want, q, s)
    assert not bool(torch.isnan(want).any())
    acc, _ = ko.oracle_dequant(q, s, c["dst"])
    ko.assert_dequant(acc.float(), q, s, dst=c["dst"])
    ko.assert_dequant(c["dst"] + want, q, s, dst=c["dst"])
    if N > 1:
        assert ko.rejects(ko.assert_dequant, want, q, s, dst=c["dst"])  # not accumulated
        bad = want.clone()
        bad[-1] = q[-1].float() * s[max(nblk - 2, 0)] + (1.0 if nblk == 1 else 0.0)
        if bad[-1] != want[-1]:
            assert ko.rejects(ko.assert_dequant, bad, q, s)             # wrong block's scale


@pytest.mark.parametrize("name", ["N1023", f"N{ko.QBLK * 7 + 517}"])
def test_int8_wrong_results_rejected(name):
    x = _case(INT8, name)["x"]
    N = x.numel()
    q, s = ref.quant_int8_blockwise(x)
    idx = torch.arange(N) // ko.QBLK
    # scale amax / 128
    s128 = s * 127.0 / 128.0
    assert ko.rejects(ko.assert_int8, q, s128, x)
    q128 = (x / s128[idx]).nan_to_num(0.0).round().clamp(-127, 127).to(torch.int8)
    assert ko.rejects(ko.assert_int8, q128, s, x)
    # truncation instead of round-to-nearest
    inv = torch.where(s > 0, 1.0 / s, torch.zeros_like(s))
    assert ko.rejects(ko.assert_int8, (x * inv[idx]).trunc().to(torch.int8), s, x)
    # tail block's amax taken over 1024 elements of whatever follows the data
    nblk = s.numel()
    follow = torch.cat([x, 10 * x.abs().max() * torch.ones(nblk * ko.QBLK - N)])
    _, s_over = ref.quant_int8_blockwise(follow)
    assert ko.rejects(ko.assert_int8, q, s_over, x)
    # a code off by 2
    q2 = q.clone()
    q2[0] = q2[0] + (2 if q2[0] < 100 else -2)
    assert ko.rejects(ko.assert_int8, q2, s, x)


# ------------------------------------------------ nesterov outer, pseudograd
@pytest.mark.parametrize("name,c", OUTER, ids=_ids(OUTER))
def test_outer_oracle_passes_and_wrong_results_rejected(name, c):
    o = ko.oracle_nesterov(c["theta"], c["buf"], c["delta"], **ko.OUTER_HP)
    t, b = o["theta"].float(), o["buf"].float()
    ko.assert_nesterov(o, t, t.clone(), t.bfloat16(), b)
    # fp32 evaluation in the kernel's order
    b32 = 0.9 * c["buf"] + c["delta"]
    t32 = c["theta"] - 0.7 * (c["delta"] + 0.9 * b32)
    ko.assert_nesterov(o, t32, t32.clone(), t32.bfloat16(), b32)
    ko.assert_pseudograd(c["theta"] - c["master"], c["theta"], c["master"])
    # master left at its old value; inner16 rounded from the old theta
    assert ko.rejects(ko.assert_nesterov, o, t, c["master"], t.bfloat16(), b)
    assert ko.rejects(ko.assert_nesterov, o, t, t.clone(), c["theta"].bfloat16(), b)
    # plain momentum instead of the Nesterov look-ahead
    plain = (c["theta"].double() - ko.f32(0.7) * o["buf"]).float()
    assert ko.rejects(ko.assert_nesterov, o, plain, plain.clone(), plain.bfloat16(), b)
    # pseudograd with the operands swapped, or rounded through bf16
    assert ko.rejects(ko.assert_pseudograd, c["master"] - c["theta"], c["theta"], c["master"])
    assert ko.rejects(ko.assert_pseudograd, c["theta"] - c["master"].bfloat16().float(),
                      c["theta"], c["master"])


# --------------------------------------------------------------- transpose
@pytest.mark.parametrize("shape", ko.TRANSPOSE_SHAPES, ids=str)
def test_transpose_helper(shape):
    B, S, H, D = shape
    x = bf(torch.randn(B, S, H, D, generator=ko.gen(800)))
    good = x.permute(0, 2, 3, 1).contiguous()
    ko.assert_transpose(good, x)
    # rows and columns swapped inside a 64x64 tile only
    bad = good.clone()
    bad[0, 0, :64, :64] = good[0, 0, :64, :64].t()
    assert ko.rejects(ko.assert_transpose, bad, x)
    # a NaN that equals nothing, not even itself
    bad = good.clone()
    bad[-1, -1, -1, -1] = float("nan")
    assert ko.rejects(ko.assert_transpose, bad, x)


# --------------------------------------------------------------------- fp8
def _fp8_trunc(o, fmt):
    """Round toward zero: where RNE rounded away from zero, one code less."""
    dt, _ = ko.FP8[fmt]
    b = o["bytes"].clone()
    away = b.view(dt).float().abs() > o["q32"].abs()
    b[away] -= 1
    return b


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("prev_kind", ["small", "large", "zero"])
@pytest.mark.parametrize("n", ko.FP8_NS)
def test_fp8_oracle_passes_and_wrong_results_rejected(n, prev_kind, fmt):
    dt, fmax = ko.FP8[fmt]
    x = ko.fp8_values((n,), 900)
    prev = ko.fp8_prev(x, prev_kind)
    o = ko.oracle_fp8(x, prev, fmt)
    x8 = o["bytes"].view(dt)
    ko.assert_fp8(o, fmt, x8, sinv=o["sinv"], amax_next=o["amax_next"])
    deq = x8.float()
    assert float(deq.abs().max()) <= fmax
    if prev_kind != "large":
        assert float(deq.abs().max()) == fmax          # saturation is reached
    # sinv as the reciprocal of s instead of prev / fmax, where that differs
    alt = 1.0 / o["s"]
    if not torch.equal(alt, o["sinv"]):
        assert ko.rejects(ko.assert_fp8, o, fmt, x8, sinv=alt)
    # truncation instead of round-to-nearest-even
    trunc = _fp8_trunc(o, fmt)
    if prev_kind != "zero" and n > 8:
        assert not torch.equal(trunc, o["bytes"])
    if not torch.equal(trunc, o["bytes"]):
        assert ko.rejects(ko.assert_fp8, o, fmt, trunc.view(dt))
    # no saturation
    if prev_kind == "small":
        unsat = (x.float() * o["s"]).to(dt)
        assert ko.rejects(ko.assert_fp8, o, fmt, unsat)
    # amax_next missing the last partial stride (it holds the largest value)
    stride = ko.GRID_CAP * ko.BLOCK * 8
    cut = (n // stride) * stride if n > stride else n - 8
    short = x[:cut].float().abs().max().reshape(1) if cut else torch.zeros(1)
    assert ko.rejects(ko.assert_fp8, o, fmt, x8, amax_next=short)
    # the other format's encoding
    other = "e5m2" if fmt == "e4m3" else "e4m3"
    assert ko.rejects(ko.assert_fp8, o, fmt, o["q32"].to(ko.FP8[other][0]).view(dt))


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("shape", ko.FP8_TQ_SHAPES, ids=str)
def test_fp8_transpose_oracle(shape, fmt):
    dt, _ = ko.FP8[fmt]
    x = ko.fp8_values(shape, 910)
    xt = x.t().contiguous()
    o = ko.oracle_fp8(xt, ko.fp8_prev(x, "small"), fmt)
    ko.assert_fp8(o, fmt, o["bytes"].view(dt), sinv=o["sinv"], amax_next=o["amax_next"])
    # not transposed inside one 64x64 tile
    bad = o["bytes"].clone()
    bad[:64, :64] = o["bytes"][:64, :64].t()
    assert ko.rejects(ko.assert_fp8, o, fmt, bad.view(dt))


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("shape", ko.FP8_ROW_SHAPES, ids=str)
def test_fp8_rowwise_oracle(shape, fmt):
    dt, fmax = ko.FP8[fmt]
    x = ko.fp8_values(shape, 920)
    x[shape[0] // 2] = 0
    o = ko.oracle_fp8_rowwise(x, fmt)
    ko.assert_fp8(o, fmt, o["bytes"].view(dt), sinv=o["sinv"])
    z = shape[0] // 2
    assert not bool(o["bytes"][z].any())
    assert float(o["sinv"][z]) == float(torch.tensor(1e-12) / torch.tensor(fmax))
    if shape[0] > 1:
        # one scale for the whole tensor instead of one per row
        whole = ko.oracle_fp8(x, float(x.float().abs().max()), fmt)
        assert ko.rejects(ko.assert_fp8, o, fmt, whole["bytes"].view(dt))
        # the next row's scale
        assert ko.rejects(ko.assert_fp8, o, fmt, o["bytes"].view(dt), sinv=o["sinv"].roll(1, 0))
