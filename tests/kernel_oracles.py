"""float64 oracles, assert helpers and the edge-shape cases of the
memory-bound and fp8 kernels.

Used by tests/test_kernel_oracles_cpu.py (proves, without a GPU, that every
helper accepts the oracle's own result and rejects named wrong results) and
by tests/test_ops_edges_gpu.py (runs the HIP kernels through the helpers).

An oracle runs on the CPU in float64 on exactly the bf16 / fp32 values the
kernel is given, and mirrors only the rounding points the design chose (a
stored bf16 tensor that is read back, a bf16-rounded scale). Everything else
is exact arithmetic, and the helper's tolerance pays for what the kernel does
in fp32.

Tolerance classes (u = 2^-24, the fp32 unit roundoff):

exact
    torch.equal on NaN-free tensors. Moves, casts of one fp32 value, single
    correctly-rounded fp32 operations (the library is built -O3 without
    fast-math, so + - * / and sqrt are IEEE).
bf16, rounded once
    One round-to-nearest to bf16 is at most 2^-8 |want|; RTOL_BF16 = 2^-7
    leaves the factor 2 that test_cross_block_reductions_are_repeatable
    uses. The atol pays for the fp32 arithmetic before the rounding: depth *
    u * max|term| with the depth read from the kernel's loops; each oracle
    returns it as a tensor next to the value it belongs to.
fp32, a few operations
    -ffp-contract may fuse a multiply into an add, so bits can differ from
    any one CPU evaluation order: RTOL_F32 = 2^-20 against the float64
    oracle, atol = 2^-20 * max|intermediate|.
fast intrinsics (__expf, __logf, rsqrtf feeding an fp32 output)
    Their error cannot be read from the code: measured once on an MI355X
    against these oracles over the cases below, tolerance = 4 x the largest
    error seen (the margin is for other inputs and seeds). See RSTD_RTOL,
    CE_LOSS_TOL, CE_MEAN_TOL.
int8 codes
    Equal to reference.quant_int8_blockwise except +-1 at rounding ties of
    x * inv, on at most INT8_MAX_DIFF_FRAC of the elements; scales within
    one fp32 ulp.
"""
from __future__ import annotations

import math

import torch

from prime_amd.ops import reference as ref

U = 2.0 ** -24
RTOL_BF16 = 2.0 ** -7
RTOL_F32 = 2.0 ** -20
# smallest normal fp32 / bf16 magnitude: below it a product may be flushed
# or lose bits, so relative bounds stop holding and this absolute one starts
TINY = 2.0 ** -126

GRID_CAP = 2048   # PRIME_MAX_GRID
BLOCK = 256
QBLK = 1024

# --- class "fast intrinsics": measured on an MI355X, tolerance = 4 x measured
# rstd = rsqrtf(ss / D + eps): largest |got / want - 1| over all norm cases
# below was 1.224e-07 (2 ulp: the fp32 sum of squares plus rsqrtf).
RSTD_MEASURED = 1.224e-07
RSTD_RTOL = 4 * RSTD_MEASURED
# CE row loss = M + __logf(S) - z[tgt], in units of max(1, max|z_row|) (the
# fp32 sum M + log S is rounded at the magnitude of the logits): largest
# |got - want| / max(1, max|z_row|) over all CE cases was 3.350e-07.
CE_LOSS_MEASURED = 3.350e-07
CE_LOSS_TOL = 4 * CE_LOSS_MEASURED
# mean loss (torch sum of the row losses / n_valid), same unit with the
# largest |z| of the batch: largest scaled error was 7.348e-09 (the mean is
# itself an fp32 number: half an ulp of a loss of 10 in a batch whose
# largest logit is 85 is already 5.6e-09 in this unit).
CE_MEAN_MEASURED = 7.348e-09
CE_MEAN_TOL = 4 * CE_MEAN_MEASURED

# CE gradient: the kernel stores bf16(p - onehot) and the backward multiplies
# it by a bf16 scale in bf16, so the value is rounded to bf16 twice:
# (1 + 2^-8)^2 - 1 < 2^-7 + 2^-15. p itself carries fp32 error: __expf of an
# argument of magnitude a <= 256 is off by about (a + 2) u relatively, the
# sum S by its depth (V / 2048 * 8 serial adds + 8 merges, < 256) * u, 1 / S
# and two products by 4 u: under 2^9 * u = 2^-15. 2^-10 covers both with room.
CE_GRAD_RTOL = 2.0 ** -7 + 2.0 ** -10

INT8_MAX_DIFF_FRAC = 1e-3

FP8 = {
    "e4m3": (torch.float8_e4m3fn, 448.0),
    "e5m2": (torch.float8_e5m2, 57344.0),
}


def gen(seed: int) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def bf(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16)


def f32(x: float) -> float:
    """The double value of x after the cast to float the C API applies."""
    return float(torch.tensor(x, dtype=torch.float32))


# ------------------------------------------------------------------ helpers
def check_close(got, want, rtol, atol, what: str) -> None:
    """|got - want| <= rtol |want| + atol elementwise, in float64; got must
    be finite. atol is a float or a tensor broadcastable to want."""
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), \
        f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    g, w = got.double(), want.double()
    if not bool(torch.isfinite(g).all()):
        raise AssertionError(f"{what}: {int((~torch.isfinite(g)).sum())} non-finite values")
    tol = (rtol * w.abs() + atol).expand_as(w)
    over = (g - w).abs() - tol
    if bool((over > 0).any()):
        i = int(over.argmax())
        raise AssertionError(
            f"{what}: {int((over > 0).sum())} of {w.numel()} outside tolerance; "
            f"worst at flat index {i}: got {g.flatten()[i].item():.9g}, want "
            f"{w.flatten()[i].item():.9g}, tol {tol.flatten()[i].item():.3g}")


def check_equal(got, want, what: str) -> None:
    """Bitwise-equal values (torch.equal), NaN-free."""
    got = got.detach().cpu()
    want = want.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), \
        f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} != {want.dtype}"
    if got.is_floating_point() and got.dtype not in (torch.float8_e4m3fn, torch.float8_e5m2):
        assert not bool(torch.isnan(got).any()), f"{what}: NaN in result"
    if not torch.equal(got, want):
        ne = got != want
        i = int(ne.flatten().int().argmax())
        raise AssertionError(
            f"{what}: {int(ne.sum())} of {want.numel()} differ; first at flat "
            f"index {i}: got {got.flatten()[i].item()!r}, want {want.flatten()[i].item()!r}")


def rejects(fn, *args, **kw) -> bool:
    """True when the helper call raises AssertionError."""
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


# ------------------------------------------------- rmsnorm / add_rmsnorm
NORM_SHAPES = [(3, 8), (33, 264), (5, 2056), (1029, 264), (2053, 64), (4, 8192)]
NORM_EPS = 1e-5


def norm_cases():
    """[(id, dict)] with x, res, w, dy, ds (bf16 CPU tensors). dy carries a
    component along x, as the gradient of any loss on the norm output does,
    so the projection term of dx is not noise. The `spread` case has row
    magnitudes 1e-4 .. 1e2: eps decides rstd on the small rows."""
    out = []
    for i, (R, D) in enumerate(NORM_SHAPES + [(33, 264)]):
        g = gen(100 + i)
        spread = i == len(NORM_SHAPES)
        x = torch.randn(R, D, generator=g)
        res = torch.randn(R, D, generator=g)
        if spread:
            mag = torch.logspace(-4, 2, R).unsqueeze(1)
            x, res = x * mag, res * mag
        w = 1.0 + 0.3 * torch.randn(D, generator=g)
        s = x + res
        dirn = s / s.pow(2).mean(-1, keepdim=True).sqrt()
        dy = torch.randn(R, D, generator=g) + 0.5 * dirn
        ds = torch.randn(R, D, generator=g)
        name = f"{R}x{D}" + ("-spread" if spread else "")
        out.append((name, dict(x=bf(x), res=bf(res), w=bf(w), dy=bf(dy), ds=bf(ds))))
    return out


def _norm_depth(D: int) -> int:
    """Adds on the longest path of a row reduction: 8 per owned vector, then
    6 shuffle steps in the wave and up to 4 across the waves."""
    return 8 * math.ceil(D / (8 * BLOCK)) + 10


def oracle_norm(x, w, dy=None, res=None, ds=None, eps=NORM_EPS):
    """rmsnorm (res=None: s is x itself) and fused_add_rmsnorm. Mirrors: s is
    the fp32 sum x + res stored as bf16; rstd comes from the fp32 sum before
    that rounding; y and the backward read the stored bf16 s.

    Returns float64 values and, as `<name>_atol`, the fp32-arithmetic part of
    each tolerance:
      y   rstd is off by at most depth*u (sum of squares, all positive) plus
          4u (division, eps, rsqrtf), and two products: (depth + 8) u |y|.
      dx  with t = dy w shat, mean_dot is off by (depth + 3) u mean|t|; the
          kernel's fp32 rstd enters three times at <= 4u and the remaining
          products and adds cost another few u of the two terms that cancel:
          rstd u ((depth + 3) |shat| mean|t| + 16 (|dy w| + |shat mean_dot|))
          plus u |ds| for the residual add.
      dw  R terms summed in fp32 (per block, then the partial rows), each
          term with two roundings and rstd: (R + 8) u max_r |dy shat|.
    """
    eps = f32(eps)
    x32 = x.float()
    s32 = x32 if res is None else x32 + res.float()   # one fp32 add, as the kernel
    s_bf = s32.bfloat16()
    D = x.shape[-1]
    R = x.numel() // D
    depth = _norm_depth(D)
    rstd = (s32.double().pow(2).mean(-1, keepdim=True) + eps).rsqrt() if D else \
        torch.zeros(*x.shape[:-1], 1, dtype=torch.float64)
    sd, wd = s_bf.double(), w.double()
    y = sd * rstd * wd
    o = dict(s=s_bf, rstd=rstd.squeeze(-1), y=y, y_atol=(depth + 8) * U * y.abs())
    if dy is None:
        return o
    shat = sd * rstd
    dyw = dy.double() * wd
    t = dyw * shat
    mean_dot = t.mean(-1, keepdim=True)
    dx = rstd * (dyw - shat * mean_dot)
    dx_atol = rstd * U * ((depth + 3) * shat.abs() * t.abs().mean(-1, keepdim=True)
                          + 16 * (dyw.abs() + (shat * mean_dot).abs()))
    if ds is not None:
        dx = dx + ds.double()
        dx_atol = dx_atol + U * ds.double().abs()
    term = (dy.double() * shat).reshape(R, D)
    o.update(dx=dx, dx_atol=dx_atol, dw=term.sum(0), dw_term=term,
             dw_atol=(R + 8) * U * (term.abs().amax(0) if R else torch.zeros(D, dtype=torch.float64)),
             shat=shat, dyw=dyw, mean_dot=mean_dot)
    return o


def assert_norm_fwd(o, y, s=None, rstd=None, what="norm"):
    check_close(y, o["y"], RTOL_BF16, o["y_atol"], f"{what}: y")
    if s is not None:
        # fp32 add of two bf16 values, rounded to bf16: the same two IEEE
        # roundings on both sides
        check_equal(s, o["s"], f"{what}: s")
    if rstd is not None:
        check_close(rstd, o["rstd"], RSTD_RTOL, 0.0, f"{what}: rstd")


def assert_norm_bwd(o, dx, dw, what="norm"):
    check_close(dx, o["dx"], RTOL_BF16, o["dx_atol"], f"{what}: dx")
    check_close(dw, o["dw"], RTOL_BF16, o["dw_atol"], f"{what}: dw")


# -------------------------------------------------------------------- RoPE
ROPE_SHAPES = [(2, 37, 3, 64), (1, 5, 1, 128), (1, 1100, 30, 128)]
ROPE_OFFSETS = (0, 7)
ROPE_TABLE_EXTRA = 8   # tables hold S + 8 rows: enough for every offset used


def rope_cases():
    out = []
    for i, (B, S, H, D) in enumerate(ROPE_SHAPES):
        g = gen(200 + i)
        x = bf(torch.randn(B, S, H, D, generator=g))
        dy = bf(torch.randn(B, S, H, D, generator=g))
        cos, sin = ref.rope_tables(D, S + ROPE_TABLE_EXTRA)
        for off in ROPE_OFFSETS:
            out.append((f"{B}x{S}x{H}x{D}-off{off}",
                        dict(x=x, dy=dy, cos=cos, sin=sin, off=off)))
    return out


def oracle_rope(x, cos, sin, off: int, sign: float = 1.0, pos=None, interleaved=False):
    """NeoX half-split rotation at position s + off of every batch entry;
    sign = -1 is the backward. `pos` ([B, S] long) and `interleaved` exist to
    build wrong results. atol: two products and one add in fp32 (or one
    product and an fma): 3 u (|a c| + |b s|)."""
    B, S, H, D = x.shape
    half = D // 2
    if pos is None:
        pos = (torch.arange(S) + off).expand(B, S)
    c = cos.double()[pos].view(B, S, 1, half)
    s = sin.double()[pos].view(B, S, 1, half) * sign
    xd = x.double()
    if interleaved:
        a, b = xd[..., 0::2], xd[..., 1::2]
        y = torch.stack([a * c - b * s, b * c + a * s], dim=-1).flatten(-2)
        return y, None
    a, b = xd[..., :half], xd[..., half:]
    y = torch.cat([a * c - b * s, b * c + a * s], dim=-1)
    mag = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], dim=-1)
    return y, 3 * U * mag


def assert_rope(got, x, cos, sin, off, sign=1.0, what="rope"):
    want, atol = oracle_rope(x, cos, sin, off, sign)
    check_close(got, want, RTOL_BF16, atol, what)


# ------------------------------------------------------------------ SwiGLU
SWIGLU_SHAPES = [(1, 8), (65, 520), (1025, 4104)]


def swiglu_cases():
    out = []
    for i, (R, I) in enumerate(SWIGLU_SHAPES):
        g = gen(300 + i)
        gu = bf(torch.randn(R, 2 * I, generator=g) * 2)
        dout = bf(torch.randn(R, I, generator=g))
        out.append((f"{R}x{I}", dict(gu=gu, dout=dout)))
    # saturated sigmoid branches and exact zeros
    g = gen(310)
    R, I = 3, 24
    gates = torch.tensor([20., -20., 60., -60., 90., -90., 1e4, -1e4, 0., -0.,
                          1., -1.278])
    gate = gates.repeat(R * I // gates.numel()).view(R, I)
    up = torch.randn(R, I, generator=g)
    up[0, :4] = 0.0
    out.append(("saturated", dict(gu=bf(torch.cat([gate, up], -1)),
                                  dout=bf(torch.randn(R, I, generator=g)))))
    return out


def oracle_swiglu(gu, dout=None, swapped=False):
    """out = g sigmoid(g) u; dg = d u sg (1 + g (1 - sg)); du = d g sg.

    atol: __expf(-g) = exp2(-g log2 e) rounds its argument, so e^-g and with
    it sigmoid are off by about (|g| + 2) u relatively, plus one division and
    two products: (|g| + 8) u |want|. Once sigmoid drops below the smallest
    normal fp32 (g < -87.3; __expf(-g) overflows at g < -88.7) the kernel may
    hold 0 for it: TINY times the factors that multiply it. For dg the factor
    1 + g (1 - sg) passes through zero near g = -1.278, so the fp32 error of
    that factor, (|g| + 8) u (1 + |g|), is paid on |d u sg| absolutely.
    """
    I = gu.shape[-1] // 2
    g, u = gu[..., :I].double(), gu[..., I:].double()
    if swapped:
        g, u = u, g
    sg = torch.sigmoid(g)
    out = g * sg * u
    rel = (g.abs() + 8) * U
    o = dict(out=out, out_atol=rel * out.abs() + TINY * (1 + g.abs() * u.abs()), sg=sg, g=g, u=u)
    if dout is None:
        return o
    d = dout.double()
    fac = 1 + g * (1 - sg)
    dg = d * u * sg * fac
    du = d * g * sg
    dg_atol = (d * u * sg).abs() * rel * (1 + g.abs()) + TINY * (1 + (d * u).abs() * (1 + g.abs()))
    du_atol = rel * du.abs() + TINY * (1 + (d * g).abs())
    o.update(dgu=torch.cat([dg, du], -1), dgu_atol=torch.cat([dg_atol, du_atol], -1), d=d)
    return o


def assert_swiglu(o, out=None, dgu=None, what="swiglu"):
    if out is not None:
        check_close(out, o["out"], RTOL_BF16, o["out_atol"], f"{what}: out")
    if dgu is not None:
        check_close(dgu, o["dgu"], RTOL_BF16, o["dgu_atol"], f"{what}: dgu")


# ----------------------------------------------------------- cross entropy
CE_SHAPES = [(5, 8), (64, 2056), (2053, 512), (16, 32000)]
CE_IGNORE = -100
CE_GRAD_OUT = 3.0   # (3 * loss).backward()


def ce_cases():
    """Logits: rows cycle through plain, +80, -80, spread 30, and 80 + spread
    30. Targets at column 0, at V - 1 and in the last vector a thread owns
    (V - 5); ignored rows; a row whose target dominates (p ~ 1); rows whose
    maximum is the first / the last column. Last case: every row ignored."""
    out = []
    for i, (R, V) in enumerate(CE_SHAPES + [(5, 8)]):
        g = gen(400 + i)
        z = torch.randn(R, V, generator=g)
        r = torch.arange(R)
        shift = torch.tensor([0., 80., -80., 0., 0., 0., 0., 80.])[r % 8]
        spread = torch.tensor([1., 1., 1., 30., 1., 4., 1., 30.])[r % 8]
        z = z * spread.unsqueeze(1) + shift.unsqueeze(1)
        tgt = torch.randint(0, V, (R,), generator=g)
        tgt[0], tgt[1], tgt[2] = 0, V - 1, V - 5
        z[4, tgt[4]] = z[4].max() + 40          # target dominates
        a, b = (5, 6) if R > 6 else (0, 1)
        z[a, 0] = z[a].max() + 3                # maximum in the first column
        z[b, V - 1] = z[b].max() + 3            # maximum in the last column
        tgt[3] = CE_IGNORE
        if R > 8:
            tgt[R - 1] = CE_IGNORE
            tgt[r % 17 == 9] = CE_IGNORE
        all_ign = i == len(CE_SHAPES)
        if all_ign:
            tgt[:] = CE_IGNORE
        out.append((f"{R}x{V}" + ("-all-ignored" if all_ign else ""),
                    dict(z=bf(z), tgt=tgt)))
    return out


def oracle_ce(z, tgt, grad_out=CE_GRAD_OUT, ignore=CE_IGNORE, mean_over_rows=False):
    """Row loss lse(z) - z[tgt] (0 for ignored rows), mean over the valid
    rows, and the gradient (softmax - onehot) * sc with sc the bf16-rounded
    fp32 quotient grad_out / n_valid, as the backward applies it. Ignored
    rows have gradient exactly zero.

    grad_atol: TINY everywhere (p below the normal range may be flushed);
    in the target column p - 1 cancels, leaving the absolute fp32 error of p
    (< 2^-15, see CE_GRAD_RTOL) times sc."""
    R, V = z.shape
    zd = z.double()
    valid = tgt != ignore
    t = torch.where(valid, tgt, torch.zeros_like(tgt))
    lse = torch.logsumexp(zd, dim=-1)
    row = torch.where(valid, lse - zd.gather(1, t.view(-1, 1)).squeeze(1),
                      torch.zeros(R, dtype=torch.float64))
    n_valid = max(int(valid.sum()), 1)
    denom = R if mean_over_rows else n_valid
    mean = row.sum() / denom
    p = torch.softmax(zd, dim=-1)
    onehot = torch.zeros_like(p).scatter_(1, t.view(-1, 1), 1.0)
    sc = (torch.tensor(grad_out, dtype=torch.float32)
          / torch.tensor(float(denom), dtype=torch.float32)).bfloat16().double()
    unit = (p - onehot) * valid.unsqueeze(1)
    grad = unit * sc
    atol = torch.full_like(p, TINY) + onehot * (2.0 ** -15) * sc.abs()
    zmax = zd.abs().amax(-1).clamp(min=1.0) if V else torch.ones(R, dtype=torch.float64)
    return dict(row=row, mean=mean, grad=grad, grad_atol=atol, valid=valid, p=p,
                onehot=onehot, sc=sc, zmax=zmax, n_valid=n_valid, lse=lse)


def assert_ce(o, row=None, mean=None, grad=None, what="ce"):
    if row is not None:
        check_close(row, o["row"], 0.0, CE_LOSS_TOL * o["zmax"], f"{what}: row loss")
        check_equal(row.detach().cpu()[~o["valid"]],
                    torch.zeros(int((~o["valid"]).sum())), f"{what}: loss of ignored rows")
    if mean is not None:
        check_close(mean.reshape(()), o["mean"], 0.0,
                    CE_MEAN_TOL * float(o["zmax"].max()), f"{what}: mean loss")
    if grad is not None:
        check_close(grad, o["grad"], CE_GRAD_RTOL, o["grad_atol"], f"{what}: grad")
        ign = grad.detach().cpu()[~o["valid"]]
        check_equal(ign, torch.zeros_like(ign), f"{what}: grad of ignored rows")


# ------------------------------------------------------- AdamW, grad_sqnorm
ADAMW_NS = [3, 4099, 4 * 524288 + 1203]
# (step, wd, gscale): steps 1, 2, 1000; wd 0 and 0.1; with and without gscale
ADAMW_VARIANTS = [(1, 0.0, None), (2, 0.1, 0.37), (1000, 0.1, None), (1000, 0.0, 0.37)]
ADAMW_HP = dict(lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-8)


def adamw_cases():
    out = []
    for i, N in enumerate(ADAMW_NS):
        g = gen(500 + i)
        st = dict(p32=torch.randn(N, generator=g), g=bf(torch.randn(N, generator=g) * 2),
                  m=0.1 * torch.randn(N, generator=g),
                  v=torch.randn(N, generator=g).pow(2) * 0.5 + 1e-3)
        for step, wd, gs in ADAMW_VARIANTS:
            out.append((f"N{N}-step{step}-wd{wd}-gs{gs}", dict(st, step=step, wd=wd, gscale=gs)))
    return out


def oracle_adamw(p32, g, m, v, *, lr, beta1, beta2, eps, wd, step, gscale=None,
                 v_bias_correction=True, decay_from_updated=False, gscale_on_v=True):
    """Decoupled-decay AdamW in float64 on the float-cast hyper-parameters;
    the keyword switches build wrong results. Returns p, m, v and the atol of
    each: 2^-20 * max|intermediate| (the two addends of m and of v; the
    parameter and its update)."""
    lr, b1, b2, eps, wd = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(wd)
    gs = 1.0 if gscale is None else f32(gscale)
    gd = g.double() * gs
    gv = gd if gscale_on_v else g.double()
    m1 = b1 * m.double() + (1 - b1) * gd
    v1 = b2 * v.double() + (1 - b2) * gv * gv
    c1 = 1 / (1 - b1 ** step)
    c2 = 1 / (1 - b2 ** step) if v_bias_correction else 1.0
    adam = (m1 * c1) / ((v1 * c2).sqrt() + eps)
    p0 = p32.double()
    if decay_from_updated:
        p1 = p0 - lr * adam
        p1 = p1 - lr * wd * p1
    else:
        p1 = p0 - lr * (adam + wd * p0)

    def amax(*ts):
        return max([float(t.abs().max()) for t in ts if t.numel()] + [0.0])

    return dict(p=p1, m=m1, v=v1,
                p_atol=RTOL_F32 * amax(p0, lr * adam),
                m_atol=RTOL_F32 * amax(m.double(), gd),
                v_atol=RTOL_F32 * amax(v.double(), gd * gd))


def assert_adamw(o, p32, p16, m, v, what="adamw"):
    check_close(p32, o["p"], RTOL_F32, o["p_atol"], f"{what}: p32")
    check_close(m, o["m"], RTOL_F32, o["m_atol"], f"{what}: m")
    check_close(v, o["v"], RTOL_F32, o["v_atol"], f"{what}: v")
    check_equal(p16, p32.detach().cpu().bfloat16(), f"{what}: p16 vs p32.bfloat16()")


def sqnorm_rtol(N: int) -> float:
    """Positive terms, so the relative error is at most depth * u: 8 serial
    adds per owned vector, 10 for the block tree, 32 for torch's sum of the
    2048 partials (a few per thread, then a tree)."""
    return (8 * math.ceil(max(N, 1) / (8 * GRID_CAP * BLOCK)) + 10 + 32) * U


def assert_sqnorm(got, g, what="grad_sqnorm"):
    want = g.double().pow(2).sum().reshape(1)
    check_close(got, want, sqnorm_rtol(g.numel()), 0.0, what)


# ------------------------------------------------------------ int8 quant
INT8_NS = [1, 1023, QBLK * 7 + 517, 2049 * QBLK + 517]


def int8_cases():
    """x ~ 0.01 N(0,1) with block magnitudes spread over 1e-3 .. 1e3; block 1
    all zero and block 2 with a negative maximum where those blocks exist
    (N = 1 holds one negative value). `dst` is the accumulate target."""
    out = []
    for i, N in enumerate(INT8_NS):
        g = gen(600 + i)
        x = torch.randn(N, generator=g) * 0.01
        nblk = (N + QBLK - 1) // QBLK
        x = x * torch.logspace(-3, 3, nblk).repeat_interleave(QBLK)[:N]
        if N == 1:
            x[0] = -0.3
        if nblk > 2:
            x[QBLK:2 * QBLK] = 0.0
            x[2 * QBLK + 77] = -5 * x[2 * QBLK:3 * QBLK].abs().max()
        out.append((f"N{N}", dict(x=x, dst=torch.randn(N, generator=g))))
    return out


def _ulp(t: torch.Tensor) -> torch.Tensor:
    return (torch.nextafter(t.abs(), torch.full_like(t, float("inf"))) - t.abs()).double()


def assert_int8(q, scales, x, what="quant_int8"):
    qr, sr = ref.quant_int8_blockwise(x, QBLK)
    q, scales = q.detach().cpu(), scales.detach().cpu()
    assert q.dtype == torch.int8 and tuple(q.shape) == tuple(qr.shape), f"{what}: codes {q.dtype} {tuple(q.shape)}"
    check_close(scales, sr.double(), 0.0, _ulp(sr), f"{what}: scales")
    diff = (q.int() - qr.int()).abs()
    if int(diff.max()) > 1:
        raise AssertionError(f"{what}: a code differs by {int(diff.max())} from the reference")
    n_diff = int((diff != 0).sum())
    if n_diff > INT8_MAX_DIFF_FRAC * q.numel():
        raise AssertionError(f"{what}: {n_diff} of {q.numel()} codes differ from the "
                             f"reference (cap {INT8_MAX_DIFF_FRAC:g})")


def oracle_dequant(q, scales, dst=None):
    """Without dst: the single fp32 product q * scale (exact class). With
    dst: float64 dst + q * scale and its atol (fp32 class)."""
    idx = torch.arange(q.numel()) // QBLK
    if dst is None:
        return q.float() * scales[idx], None
    v = q.double() * scales.double()[idx]
    amax = max(float(v.abs().max()), float(dst.abs().max())) if q.numel() else 0.0
    return dst.double() + v, RTOL_F32 * amax


def assert_dequant(got, q, scales, dst=None, what="dequant_int8"):
    want, atol = oracle_dequant(q.detach().cpu(), scales.detach().cpu(), dst)
    if dst is None:
        check_equal(got, want, what)
    else:
        check_close(got, want, RTOL_F32, atol, what + " (accumulate)")


# ------------------------------------------------ nesterov outer, pseudograd
OUTER_NS = [1, 2048, 524288 + 77]
OUTER_HP = dict(lr=0.7, mu=0.9)


def outer_cases():
    out = []
    for i, N in enumerate(OUTER_NS):
        g = gen(700 + i)
        out.append((f"N{N}", dict(theta=torch.randn(N, generator=g),
                                   master=torch.randn(N, generator=g),
                                   buf=torch.randn(N, generator=g),
                                   delta=torch.randn(N, generator=g) * 0.1)))
    return out


def oracle_nesterov(theta, buf, delta, *, lr, mu):
    lr, mu = f32(lr), f32(mu)
    d = delta.double()
    b = mu * buf.double() + d
    t = theta.double() - lr * (d + mu * b)
    amax = max(float(theta.abs().max()), float(b.abs().max()), float(d.abs().max()))
    return dict(theta=t, buf=b, atol=RTOL_F32 * amax)


def assert_nesterov(o, theta, master, inner16, buf, what="nesterov"):
    check_close(theta, o["theta"], RTOL_F32, o["atol"], f"{what}: theta")
    check_close(buf, o["buf"], RTOL_F32, o["atol"], f"{what}: buf")
    check_equal(master, theta, f"{what}: master32 vs theta")
    check_equal(inner16, theta.detach().cpu().bfloat16(), f"{what}: inner16 vs theta.bfloat16()")


def assert_pseudograd(got, outer, master, what="pseudograd"):
    check_equal(got, outer - master, what)   # one fp32 subtraction


# --------------------------------------------------------------- transpose
TRANSPOSE_SHAPES = [(1, 64, 1, 64), (2, 192, 3, 192), (2, 128, 3, 128)]


def assert_transpose(got, x, what="transpose_bshd"):
    check_equal(got, x.detach().cpu().permute(0, 2, 3, 1).contiguous(), what)


# --------------------------------------------------------------------- fp8
FP8_NS = [8, 4104, 8 * 524288 + 8 * 300]
FP8_TQ_SHAPES = [(64, 128), (128, 256), (192, 384)]
FP8_ROW_SHAPES = [(1, 8), (3, 2056), (2051, 64)]


def fp8_values(shape, seed: int) -> torch.Tensor:
    """bf16 values over a wide dynamic range (so the fp8 subnormals and the
    saturation region are both populated), some exact zeros, and the largest
    magnitude near the end: for a flat tensor of n elements that is inside
    the last, partial grid stride of the delayed-scaling kernel."""
    g = gen(seed)
    x = torch.randn(shape, generator=g) * torch.exp(2 * torch.randn(shape, generator=g))
    flat = x.view(-1)
    flat[::13] = 0.0
    flat[-3] = -2.5 * flat.abs().max()
    return bf(x)


def fp8_prev(x: torch.Tensor, kind: str) -> float:
    """amax_prev below max|x| (saturation), above it, or zero."""
    amax = float(x.float().abs().max())
    return {"small": 0.25 * amax, "large": 4.0 * amax, "zero": 0.0}[kind]


def oracle_fp8(x, prev, fmt: str):
    """Delayed scaling: prev = max(amax_prev, 1e-12), s = fmax / prev and
    sinv = prev / fmax as correctly rounded fp32 quotients, bytes = RNE cast
    of clamp(x * s, -fmax, fmax) (an fp32 product), amax_next = max|x|.
    `prev` is a float (per tensor) or an fp32 tensor broadcastable to x
    (per row)."""
    dt, fmax = FP8[fmt]
    prev = torch.as_tensor(prev, dtype=torch.float32).clamp(min=1e-12)
    fm = torch.tensor(fmax, dtype=torch.float32)
    s = fm / prev
    q32 = (x.float() * s).clamp(-fmax, fmax)
    amax = x.float().abs().max().reshape(1) if x.numel() else torch.zeros(1)
    return dict(bytes=q32.to(dt).view(torch.uint8), q32=q32, sinv=prev / fm,
                amax_next=amax, s=s)


def fp8_has_nan(b: torch.Tensor, fmt: str) -> bool:
    """NaN (or, for e5m2, inf) codes in a uint8 tensor."""
    if fmt == "e4m3":
        return bool(((b & 0x7F) == 0x7F).any())
    return bool(((b & 0x7C) == 0x7C).any())


def assert_fp8(o, fmt, x8, sinv=None, amax_next=None, what="fp8"):
    b = x8.detach().cpu().view(torch.uint8)
    assert not fp8_has_nan(b, fmt), f"{what}: NaN / inf code"
    check_equal(b, o["bytes"], f"{what}: bytes")
    if sinv is not None:
        check_equal(sinv.reshape(o["sinv"].shape), o["sinv"], f"{what}: sinv")
    if amax_next is not None:
        check_equal(amax_next.reshape(1), o["amax_next"], f"{what}: amax_next")


def oracle_fp8_rowwise(x, fmt: str):
    """Per-row scaling: prev is the row's own max|x| (1e-12 for a zero row,
    whose bytes are zero and whose sinv is 1e-12 / fmax)."""
    amax = x.float().abs().amax(dim=1, keepdim=True) if x.shape[1] else \
        torch.zeros(x.shape[0], 1)
    return oracle_fp8(x, amax, fmt)
