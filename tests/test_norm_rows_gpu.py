"""The row-in-registers add_rmsnorm kernels against the generic ones.

prime_add_rmsnorm_fwd / _bwd dispatch on D: D % 8 == 0 up to 8192 goes to
the kernels that keep a thread's NV = ceil(D/8/256) vectors of the row in
registers, everything else to the generic kernels, which are also exported
as prime_add_rmsnorm_{fwd,bwd}_generic. Both families share their
per-element arithmetic and their reduction, so every output must be equal
bit for bit: y, s, rstd, ds and each of the G rows of dw_part.

Shapes: the edge cases of tests/kernel_oracles.py (NV = 1, 2 and 4, idle
threads, a partial last vector, more rows than blocks), plus
  (2, 4096), (1, 8192)  NV = 2 and 4 with no partial vector
  (3, 8200)             D > 8192: must take the generic path
  (4100, 4096)          forward blocks own 2 and 3 rows, backward blocks 4
                        and 5: the next-row prefetch and its last-row edge
  (1029, 2056)          partial last vector with several rows per block
each with all operands, with res = None, and with ds_res absent. The added
shapes also go through the float64 oracle with its own tolerances.
"""
import pytest
import torch

from tests import kernel_oracles as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DW_ROWS = 1024   # functional._DW_ROWS: G = min(R, 1024) partial rows

ADDED_SHAPES = [(2, 4096), (1, 8192), (3, 8200), (4100, 4096), (1029, 2056)]


def _added_cases():
    """Same recipe as ko.norm_cases(): dy carries a component along s."""
    out = []
    for i, (R, D) in enumerate(ADDED_SHAPES):
        g = ko.gen(150 + i)
        x = torch.randn(R, D, generator=g)
        res = torch.randn(R, D, generator=g)
        w = 1.0 + 0.3 * torch.randn(D, generator=g)
        s = x + res
        dirn = s / s.pow(2).mean(-1, keepdim=True).sqrt()
        dy = torch.randn(R, D, generator=g) + 0.5 * dirn
        ds = torch.randn(R, D, generator=g)
        out.append((f"{R}x{D}", dict(x=ko.bf(x), res=ko.bf(res), w=ko.bf(w),
                                     dy=ko.bf(dy), ds=ko.bf(ds))))
    return out


ADDED = _added_cases()
ADDED_IDS = {name for name, _ in ADDED}
CASES = ko.norm_cases() + ADDED
VARIANTS = ["full", "no_res", "no_ds"]


def _d(t):
    return None if t is None else t.to(DEV)


def _nan(*shape, dtype):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _run(generic: bool, x, res, w, dy, ds):
    from prime_amd.ops._lib import check, lib, ptr, stream_of

    L = lib()
    fwd = L.prime_add_rmsnorm_fwd_generic if generic else L.prime_add_rmsnorm_fwd
    bwd = L.prime_add_rmsnorm_bwd_generic if generic else L.prime_add_rmsnorm_bwd
    R, D = x.shape
    G = max(1, min(R, DW_ROWS))
    s = _nan(R, D, dtype=torch.bfloat16)
    y = _nan(R, D, dtype=torch.bfloat16)
    rstd = _nan(R, dtype=torch.float32)
    check(fwd(stream_of(x), ptr(x), ptr(res), ptr(w), ptr(s), ptr(y), ptr(rstd),
              R, D, ko.NORM_EPS), "add_rmsnorm_fwd")
    dx = _nan(R, D, dtype=torch.bfloat16)
    dw_part = _nan(G, D, dtype=torch.float32)
    check(bwd(stream_of(x), ptr(dy), ptr(ds), ptr(s), ptr(w), ptr(rstd), ptr(dx),
              ptr(dw_part), R, D, G, ko.NORM_EPS), "add_rmsnorm_bwd")
    torch.cuda.synchronize()
    return dict(y=y, s=s, rstd=rstd, ds=dx, dw_part=dw_part)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name,c", CASES, ids=[n for n, _ in CASES])
def test_rows_kernels_equal_generic(name, c, variant):
    res = None if variant == "no_res" else c["res"]
    ds = None if variant == "no_ds" else c["ds"]
    args = (_d(c["x"]), _d(res), _d(c["w"]), _d(c["dy"]), _d(ds))
    got = _run(False, *args)
    want = _run(True, *args)
    for k in ("y", "s", "rstd", "ds", "dw_part"):
        assert not bool(torch.isnan(got[k]).any()), f"{name} {variant}: NaN left in {k}"
        assert torch.equal(got[k], want[k]), (
            f"{name} {variant}: {k} differs from the generic kernel in "
            f"{int((got[k] != want[k]).sum())} of {got[k].numel()} elements")
    if name in ADDED_IDS:
        o = ko.oracle_norm(c["x"], c["w"], c["dy"], res=res, ds=ds)
        what = f"add_rmsnorm {name} {variant}"
        ko.assert_norm_fwd(o, got["y"], s=got["s"], rstd=got["rstd"], what=what)
        dw = got["dw_part"].sum(0).to(torch.bfloat16)   # as _AddRMSNorm.backward
        ko.assert_norm_bwd(o, got["ds"], dw, what=what)
