"""Standalone timing of the row-wise passes of the layer loop at the bench
shape: fused add+rmsnorm forward and backward (R = 16384, D = 4096), and the
attention backward's delta / row constants / dO^T pass (B = 8, S = 2048,
H = 32, D = 128).

Usage (GPU box): python tools/perf_rowops.py [iters] [--repeats R] [--sets N]

Each pair is old against new in one process: the generic norm entry points
against the dispatched ones, prime_attn_delta_t + transpose_bshd(dO) against
prime_attn_delta_dot. Every variant is warmed first, then the variants
alternate, R repeats of `iters` calls each, timed with device events. Calls
rotate through N buffer sets (default 4, 1.6-2.1 GB per op) so that no call
finds its operands in the 256 MiB Infinity Cache. Printed: median us per
call (min-max over the repeats) and bytes/time, with the bytes the op has to
move computed from the shapes below.
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from prime_amd.ops._lib import check, lib, ptr, stream_of
from prime_amd.ops.functional import transpose_bshd

DEV = "cuda:0"
EPS = 1e-5
BF16, F32 = 2, 4


def norm_bytes(R, D, G):
    """fwd: x, res in; s, y out; w in; rstd out.
    bwd: dy, ds_res, s in; ds out; w, rstd in; dw_part [G, D] out."""
    fwd = 4 * R * D * BF16 + D * BF16 + R * F32
    bwd = 4 * R * D * BF16 + D * BF16 + R * F32 + G * D * F32
    return fwd, bwd


def delta_bytes(B, S, H, D):
    """What the result needs: dO, O, lse in; dOt, delta, lse^T, delta^T out.
    The old pair moves dO once more (`extra`)."""
    rows = B * S * H
    need = 3 * rows * D * BF16 + 4 * rows * F32
    extra = rows * D * BF16
    return need, extra


def time_variants(variants, iters, repeats):
    """variants: [(name, fn(i))]. Returns name -> sorted list of us/call."""
    for _, fn in variants:
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    out = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                fn(i)
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {k: sorted(v) for k, v in out.items()}


def report(times, nbytes):
    for name, ts in times.items():
        med = ts[len(ts) // 2]
        print(f"  {name:<34} {med:8.1f} us  ({ts[0]:.1f}-{ts[-1]:.1f})  "
              f"{nbytes[name] / 1e6:7.1f} MB  {nbytes[name] / med / 1e6:5.2f} TB/s")


def bench_norm(iters, repeats, nsets):
    R, D = 16384, 4096
    G = min(R, 1024)
    L = lib()
    sets = []
    for _ in range(nsets):
        t = lambda: torch.randn(R, D, device=DEV).bfloat16()  # noqa: E731
        sets.append(dict(x=t(), res=t(), dy=t(), ds=t(), s=torch.empty(R, D, device=DEV, dtype=torch.bfloat16),
                         y=torch.empty(R, D, device=DEV, dtype=torch.bfloat16),
                         dx=torch.empty(R, D, device=DEV, dtype=torch.bfloat16),
                         rstd=torch.empty(R, device=DEV),
                         dw=torch.empty(G, D, device=DEV)))
    w = (1.0 + 0.3 * torch.randn(D, device=DEV)).bfloat16()

    def fwd(entry):
        def run(i):
            b = sets[i % nsets]
            check(entry(stream_of(w), ptr(b["x"]), ptr(b["res"]), ptr(w), ptr(b["s"]),
                        ptr(b["y"]), ptr(b["rstd"]), R, D, EPS), "add_rmsnorm_fwd")
        return run

    def bwd(entry):
        def run(i):
            b = sets[i % nsets]
            check(entry(stream_of(w), ptr(b["dy"]), ptr(b["ds"]), ptr(b["s"]), ptr(w),
                        ptr(b["rstd"]), ptr(b["dx"]), ptr(b["dw"]), R, D, G, EPS),
                  "add_rmsnorm_bwd")
        return run

    for i in range(nsets):  # s and rstd of every set, for the backward
        fwd(L.prime_add_rmsnorm_fwd)(i)
    fb, bb = norm_bytes(R, D, G)
    print(f"add_rmsnorm R={R} D={D} G={G}")
    report(time_variants([("fwd generic", fwd(L.prime_add_rmsnorm_fwd_generic)),
                          ("fwd dispatched", fwd(L.prime_add_rmsnorm_fwd))], iters, repeats),
           {"fwd generic": fb, "fwd dispatched": fb})
    report(time_variants([("bwd generic", bwd(L.prime_add_rmsnorm_bwd_generic)),
                          ("bwd dispatched", bwd(L.prime_add_rmsnorm_bwd))], iters, repeats),
           {"bwd generic": bb, "bwd dispatched": bb})


def bench_delta(iters, repeats, nsets):
    B, S, H, D = 8, 2048, 32, 128
    L = lib()
    sets = []
    for _ in range(nsets):
        sets.append(dict(do=torch.randn(B, S, H, D, device=DEV).bfloat16(),
                         o=torch.randn(B, S, H, D, device=DEV).bfloat16(),
                         lse=torch.randn(B, S, H, device=DEV),
                         delta=torch.empty(B, S, H, device=DEV),
                         rowc=torch.empty(2, B, H, S, device=DEV),
                         dot=torch.empty(B, H, D, S, device=DEV, dtype=torch.bfloat16)))

    def old(i):
        b = sets[i % nsets]
        check(L.prime_attn_delta_t(stream_of(b["do"]), ptr(b["do"]), ptr(b["o"]), ptr(b["lse"]),
                                   ptr(b["delta"]), ptr(b["rowc"]), B, S, H, D), "attn_delta_t")
        transpose_bshd(b["do"])

    def new(i):
        b = sets[i % nsets]
        check(L.prime_attn_delta_dot(stream_of(b["do"]), ptr(b["do"]), ptr(b["o"]), ptr(b["lse"]),
                                     ptr(b["delta"]), ptr(b["rowc"]), ptr(b["dot"]),
                                     B, S, H, D), "attn_delta_dot")

    need, extra = delta_bytes(B, S, H, D)
    names = ("delta_t + transpose_bshd(dO)", "delta_dot")
    print(f"attention delta / row constants / dO^T  B={B} S={S} H={H} D={D}")
    report(time_variants([(names[0], old), (names[1], new)], iters, repeats),
           {names[0]: need + extra, names[1]: need})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("iters", nargs="?", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sets", type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "perf_rowops.py needs a GPU"
    torch.manual_seed(0)
    bench_norm(args.iters, args.repeats, args.sets)
    torch.cuda.empty_cache()
    bench_delta(args.iters, args.repeats, args.sets)


if __name__ == "__main__":
    main()
