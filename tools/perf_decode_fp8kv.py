"""fp8 KV cache: attn_decode_ragged (bf16 cache) vs attn_decode_ragged_fp8,
and generate_batch end to end with both cache dtypes.

  python tools/perf_decode_fp8kv.py kernel
  python tools/perf_decode_fp8kv.py e2e

Same method as tools/perf_decode_ragged.py (whose shapes and helpers this
uses): the parent never touches the GPU, every step is a fresh child process
under its own time limit, the first failing step ends the run; inside a step
the variants are warmed, then alternate `--repeats` times, and the tables
give the median and (min-max). Each variant rotates over its own >= 1 GiB of
separate caches, so the Infinity Cache serves nothing. GB/s is one pass over
the live rows: 2 * D * 2 bytes per row and kv head for bf16, 2 * (D + 4) for
fp8 (bytes plus the fp32 scale).
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

from tools.perf_decode_ragged import (  # noqa: E402
    D, H, HKV, KERNEL_SHAPES, MIXED, _fmt, _time_calls)


def step_kernel(B, smax, lens, iters, repeats):
    import torch

    from prime_amd import ops

    torch.manual_seed(0)
    dev = "cuda"
    rows_b = 2 * B * smax * HKV  # K and V head rows of one cache set
    n16 = max(2, -(-(1 << 30) // (rows_b * D * 2)))
    n8 = max(2, -(-(1 << 30) // (rows_b * (D + 4))))
    q = torch.randn(B, H, D, device=dev).bfloat16()
    c16, c8 = [], []
    for i in range(max(n16, n8)):
        k = torch.randn(B, smax, HKV, D, device=dev).bfloat16()
        v = torch.randn(B, smax, HKV, D, device=dev).bfloat16()
        if i < n8:
            c = ops.kv_cache_fp8(B, smax, HKV, D, dev)
            ops.kv_store_fp8(c, k, v, 0)
            c8.append(c)
        if i < n16:
            c16.append((k, v))
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    fns = {
        "bf16": lambda i: ops.attn_decode_ragged(
            q, c16[i % n16][0], c16[i % n16][1], lens_t),
        "fp8": lambda i: ops.attn_decode_ragged_fp8(q, c8[i % n8], lens_t),
    }
    a = ops.attn_decode_ragged(q, *c16[0], lens_t).float()
    b = ops.attn_decode_ragged_fp8(q, c8[0], lens_t).float()
    t = _time_calls(fns, iters, repeats)
    live_rows = 2 * sum(lens) * HKV
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rows = ops.decode_ragged_split(B, HKV, smax, n_cu)
    return {"B": B, "smax": smax, "lens": lens, "n16": n16, "n8": n8,
            "times": t, "live16": live_rows * D * 2, "live8": live_rows * (D + 4),
            "split_rows": rows, "nsplit": -(-smax // rows),
            "maxdiff": (a - b).abs().max().item()}


def step_e2e(model_name, n_prompts, new, repeats):
    import torch

    from prime_amd.models import build_model
    from prime_amd.models.generate import generate_batch

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
    outs = {}

    def run(dt):
        outs[dt] = generate_batch(m, prompts, new, kv_dtype=dt)

    fns = {"bf16": lambda: run("bf16"), "fp8": lambda: run("fp8")}
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
    same = [sum(1 for x, y in zip(a, b) if x == y) for a, b in
            zip(outs["bf16"], outs["fp8"])]
    cfg = m.cfg
    per_tok = 2 * cfg.n_layers * cfg.n_kv_heads
    return {"model": model_name, "lengths": lengths, "new": new, "times": out,
            "tokens": n_prompts * new, "equal_tokens": same,
            "bytes_per_token": {"bf16": per_tok * cfg.head_dim * 2,
                                "fp8": per_tok * (cfg.head_dim + 4)}}


def _child(step_args, limit):
    cmd = [sys.executable, str(Path(__file__).resolve()), "--step",
           json.dumps(step_args)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"step {step_args} failed with exit status "
                         f"{r.returncode}; stopping")
    return json.loads(r.stdout.strip().splitlines()[-1])


def run_kernel(args):
    print(f"H={H} Hkv={HKV} D={D}, {args.iters} calls per timing, "
          f"{args.repeats} alternating repeats; us per call, median (min-max)")
    print("| B | lens | splits x rows | bf16 us | fp8 us | bf16 GB/s | "
          "fp8 GB/s | bf16 / fp8 time | max abs diff |")
    print("|---|---|---|---|---|---|---|---|---|")
    cases = [(B, L, [L] * B, str(L)) for B, L in KERNEL_SHAPES]
    cases.append((8, 4096, MIXED, "mixed"))
    for B, smax, lens, label in cases:
        r = _child({"kind": "kernel", "B": B, "smax": smax, "lens": lens,
                    "iters": args.iters, "repeats": args.repeats},
                   args.step_limit)
        t16, t8 = r["times"]["bf16"], r["times"]["fp8"]
        m16, m8 = statistics.median(t16), statistics.median(t8)
        print(f"| {B} | {label} | {r['nsplit']} x {r['split_rows']} | "
              f"{_fmt(t16, 1e6, 1)} | {_fmt(t8, 1e6, 1)} | "
              f"{r['live16'] / m16 / 1e9:.0f} | {r['live8'] / m8 / 1e9:.0f} | "
              f"{m16 / m8:.2f}x | {r['maxdiff']:.2e} |", flush=True)
    print(f"\nmixed = B=8 Smax=4096 lens={MIXED}")


def run_e2e(args):
    r = _child({"kind": "e2e", "model": args.model, "n": args.prompts,
                "new": args.new, "repeats": args.repeats}, args.step_limit)
    print(f"{r['model']}: {len(r['lengths'])} prompts of lengths {r['lengths']}, "
          f"{r['new']} new tokens each, {args.repeats} alternating repeats")
    print("| generate_batch kv_dtype | seconds | new tokens/s | cache bytes/token |")
    print("|---|---|---|---|")
    for name, ts in r["times"].items():
        print(f"| {name} | {_fmt(ts)} | "
              f"{_fmt([r['tokens'] / t for t in ts], 1.0, 0)} | "
              f"{r['bytes_per_token'][name]} |")
    a = statistics.median(r["times"]["bf16"])
    b = statistics.median(r["times"]["fp8"])
    print(f"fp8 is {a / b:.3f}x the bf16 throughput; greedy tokens equal to "
          f"the bf16 run's, per prompt, of {r['new']}: {r['equal_tokens']}")


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
            raise SystemExit("perf_decode_fp8kv needs a GPU")
        s = json.loads(args.step)
        if s["kind"] == "kernel":
            r = step_kernel(s["B"], s["smax"], s["lens"], s["iters"], s["repeats"])
        else:
            r = step_e2e(s["model"], s["n"], s["new"], s["repeats"])
        print(json.dumps(r))
        return
    if args.mode is None:
        ap.error("mode is required: kernel or e2e")
    (run_kernel if args.mode == "kernel" else run_e2e)(args)


if __name__ == "__main__":
    main()
