"""Ragged batched decode: kernel-level and end-to-end measurements.

  python tools/perf_decode_ragged.py kernel   # attn_decode vs attn_decode_ragged
  python tools/perf_decode_ragged.py e2e      # N x generate vs one generate_batch

The parent process never touches the GPU: every measurement step runs in a
fresh child process under its own time limit, and the first step that
fails, faults or runs out of time ends the run (nothing more is started).
Within a step the variants are warmed once, then alternated `--repeats`
times; the tables give the median and (min-max) of the repeats.

Kernel steps rotate over enough separate KV caches (>= 1 GiB in total) that
a timing is not served from the 256 MiB Infinity Cache; GB/s is one pass
over the live K and V rows divided by the time of one call.
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

H, HKV, D = 32, 8, 128
KERNEL_SHAPES = [(1, 4096), (8, 4096), (8, 512)]  # (B, L) uniform
MIXED = [128, 695, 1262, 1829, 2396, 2963, 3530, 4096]  # B=8, Smax=4096


def _fmt(xs, scale=1.0, digits=3):
    xs = [x * scale for x in xs]
    return (f"{statistics.median(xs):.{digits}f} "
            f"({min(xs):.{digits}f}-{max(xs):.{digits}f})")


# ------------------------------------------------------------ child steps
def _time_calls(fns, iters, repeats):
    """fns: {name: callable(i)}; returns {name: [seconds per call] * repeats},
    variants alternating inside every repeat."""
    import torch

    for fn in fns.values():  # warm every variant (code objects, workspace)
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(iters):
                fn(i)
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) / 1e3 / iters)
    return out


def step_kernel(B, smax, lens, iters, repeats, with_old):
    import torch

    from prime_amd import ops

    torch.manual_seed(0)
    dev = "cuda"
    set_bytes = 2 * B * smax * HKV * D * 2
    nbuf = max(2, -(-(1 << 30) // set_bytes))
    q = torch.randn(B, H, D, device=dev).bfloat16()
    kcs = [torch.randn(B, smax, HKV, D, device=dev).bfloat16() for _ in range(nbuf)]
    vcs = [torch.randn(B, smax, HKV, D, device=dev).bfloat16() for _ in range(nbuf)]
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    fns = {"ragged": lambda i: ops.attn_decode_ragged(
        q, kcs[i % nbuf], vcs[i % nbuf], lens_t)}
    if with_old:
        L = lens[0]
        fns["attn_decode"] = lambda i: ops.attn_decode(
            q, kcs[i % nbuf], vcs[i % nbuf], length=L)
        a = ops.attn_decode_ragged(q, kcs[0], vcs[0], lens_t).float()
        b = ops.attn_decode(q, kcs[0], vcs[0], length=L).float()
        maxdiff = (a - b).abs().max().item()
    else:
        maxdiff = None
    t = _time_calls(fns, iters, repeats)
    live = 2 * sum(lens) * HKV * D * 2  # K and V rows actually attended to
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rows = ops.decode_ragged_split(B, HKV, smax, n_cu)
    return {"B": B, "smax": smax, "lens": lens, "nbuf": nbuf, "times": t,
            "live_bytes": live, "split_rows": rows,
            "nsplit": -(-smax // rows), "maxdiff": maxdiff}


def step_e2e(model_name, n_prompts, new, repeats):
    import torch

    from prime_amd.models import build_model
    from prime_amd.models.generate import generate, generate_batch

    torch.manual_seed(0)
    with torch.device("cuda"):
        m = build_model(model_name)
    m = m.to(dtype=torch.bfloat16)
    m.reset_rope("cuda")
    lo, hi = 64, 1024
    lengths = [lo + (hi - lo) * i // max(n_prompts - 1, 1) for i in range(n_prompts)]
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, m.cfg.vocab_size, (n,), generator=g).tolist()
               for n in lengths]

    def sequential():
        for p in prompts:
            generate(m, torch.tensor([p], device="cuda"), new)

    def batched():
        generate_batch(m, prompts, new)

    fns = {"sequential generate": sequential, "generate_batch": batched}
    for fn in fns.values():  # warm-up: graph captures, GEMM selection
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[name].append(time.perf_counter() - t0)
    return {"model": model_name, "lengths": lengths, "new": new, "times": out,
            "tokens": n_prompts * new}


# ----------------------------------------------------------------- parent
def _child(step_args, limit):
    """Run one step in a fresh process under its own time limit."""
    cmd = [sys.executable, str(Path(__file__).resolve()), "--step",
           json.dumps(step_args)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"step {step_args} failed with exit status "
                         f"{r.returncode}; stopping")
    return json.loads(r.stdout.strip().splitlines()[-1])


def run_kernel(args):
    print(f"H={H} Hkv={HKV} D={D} bf16, {args.iters} calls per timing, "
          f"{args.repeats} alternating repeats; us per call, median (min-max)")
    print("| B | L | splits x rows | attn_decode us | ragged us | "
          "attn_decode GB/s | ragged GB/s | speedup | max abs diff |")
    print("|---|---|---|---|---|---|---|---|---|")
    uniform4096 = None
    for B, L in KERNEL_SHAPES:
        r = _child({"kind": "kernel", "B": B, "smax": L, "lens": [L] * B,
                    "iters": args.iters, "repeats": args.repeats,
                    "with_old": True}, args.step_limit)
        old, new = r["times"]["attn_decode"], r["times"]["ragged"]
        mo, mn = statistics.median(old), statistics.median(new)
        print(f"| {B} | {L} | {r['nsplit']} x {r['split_rows']} | "
              f"{_fmt(old, 1e6, 1)} | {_fmt(new, 1e6, 1)} | "
              f"{r['live_bytes'] / mo / 1e9:.0f} | {r['live_bytes'] / mn / 1e9:.0f} | "
              f"{mo / mn:.2f}x | {r['maxdiff']:.2e} |", flush=True)
        if (B, L) == (8, 4096):
            uniform4096 = mn
    r = _child({"kind": "kernel", "B": 8, "smax": 4096, "lens": MIXED,
                "iters": args.iters, "repeats": args.repeats,
                "with_old": False}, args.step_limit)
    mn = statistics.median(r["times"]["ragged"])
    print(f"\nmixed batch B=8 Smax=4096 lens={MIXED}: ragged "
          f"{_fmt(r['times']['ragged'], 1e6, 1)} us, "
          f"{r['live_bytes'] / mn / 1e9:.0f} GB/s over the live rows")
    if uniform4096:
        print(f"time ratio mixed / uniform-4096 = {mn / uniform4096:.3f}; "
              f"sum(lens) / (B * max) = {sum(MIXED) / (8 * 4096):.3f}")


def run_e2e(args):
    r = _child({"kind": "e2e", "model": args.model, "n": args.prompts,
                "new": args.new, "repeats": args.repeats}, args.step_limit)
    print(f"{r['model']}: {len(r['lengths'])} prompts of lengths {r['lengths']}, "
          f"{r['new']} new tokens each, {args.repeats} alternating repeats")
    print("| variant | seconds | new tokens/s |")
    print("|---|---|---|")
    for name, ts in r["times"].items():
        print(f"| {name} | {_fmt(ts)} | "
              f"{_fmt([r['tokens'] / t for t in ts], 1.0, 0)} |")
    a = statistics.median(r["times"]["sequential generate"])
    b = statistics.median(r["times"]["generate_batch"])
    print(f"generate_batch is {a / b:.2f}x the sequential throughput")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("mode", nargs="?", choices=["kernel", "e2e"])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--model", default="llama_1b")
    ap.add_argument("--prompts", type=int, default=8)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--step-limit", type=float, default=240.0,
                    help="time limit of each GPU step in seconds")
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:  # child: one measurement, one JSON line
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("perf_decode_ragged needs a GPU")
        s = json.loads(args.step)
        if s["kind"] == "kernel":
            r = step_kernel(s["B"], s["smax"], s["lens"], s["iters"],
                            s["repeats"], s["with_old"])
        else:
            r = step_e2e(s["model"], s["n"], s["new"], s["repeats"])
        print(json.dumps(r))
        return
    if args.mode is None:
        ap.error("mode is required: kernel or e2e")
    (run_kernel if args.mode == "kernel" else run_e2e)(args)


if __name__ == "__main__":
    main()
