"""Weight-only fp8 linear: ops.linear_w8 vs F.linear on the bf16 weight at
decode-sized M, and generate_batch end to end with both weight dtypes.

  python tools/perf_linear_w8.py kernel
  python tools/perf_linear_w8.py e2e

Same method as tools/perf_decode_ragged.py (whose helpers this uses): the
parent never touches the GPU, every step is a fresh child process under its
own time limit, the first failing step ends the run; inside a step the
variants are warmed, then alternate `--repeats` times, and the tables give the
median and (min-max). Each variant rotates over its own >= 1 GiB of separate
weights, so the Infinity Cache serves nothing. GB/s is one pass over the
weight: N * K * 2 bytes for bf16, N * (K + 4) for fp8 (bytes plus the scale).
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

from tools.perf_decode_ragged import _fmt, _time_calls  # noqa: E402

# llama_8b: qkv, o, gate/up, down, lm_head
SHAPES = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336),
          (128256, 4096)]
ROWS = [1, 8, 32, 64]


def step_kernel(N, K, iters, repeats):
    import torch
    import torch.nn.functional as F

    from prime_amd import ops

    torch.manual_seed(0)
    dev = "cuda"
    n16 = max(2, -(-(1 << 30) // (N * K * 2)))
    n8 = max(2, -(-(1 << 30) // (N * K)))
    w16 = [(torch.randn(N, K, device=dev) * 0.02).bfloat16() for _ in range(n16)]
    w8 = [ops.quant_weight_fp8(w16[i % n16]) for i in range(n8)]
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    out = {"N": N, "K": K, "ksplit": ops.linear_w8_split(N, K, n_cu), "rows": {}}
    for M in ROWS:
        x = torch.randn(M, K, device=dev).bfloat16()
        fns = {"bf16": lambda i: F.linear(x, w16[i % n16]),
               "fp8": lambda i: ops.linear_w8(x, w8[i % n8])}
        d = (F.linear(x, w16[0]).float() - ops.linear_w8(x, w8[0]).float())
        out["rows"][M] = {"times": _time_calls(fns, iters, repeats),
                          "maxdiff": d.abs().max().item()}
    return out


def step_e2e(model_name, n_prompts, new, repeats):
    import torch

    from prime_amd.models import build_model
    from prime_amd.models.generate import generate_batch

    torch.manual_seed(0)
    with torch.device("cuda"):
        m = build_model(model_name)
    m = m.to(dtype=torch.bfloat16)
    m.reset_rope("cuda")
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, m.cfg.vocab_size, (64 + 32 * i,), generator=g)
               .tolist() for i in range(n_prompts)]
    outs = {}

    def run(dt):
        outs[dt] = generate_batch(m, prompts, new, weight_dtype=dt)

    for dt in ("bf16", "fp8"):  # warm-up: quantisation, graph captures
        run(dt)
    torch.cuda.synchronize()
    times = {"bf16": [], "fp8": []}
    for _ in range(repeats):
        for dt in times:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(dt)
            torch.cuda.synchronize()
            times[dt].append(time.perf_counter() - t0)
    same = [sum(1 for x, y in zip(a, b) if x == y)
            for a, b in zip(outs["bf16"], outs["fp8"])]
    return {"model": model_name, "lengths": [len(p) for p in prompts],
            "new": new, "times": times, "tokens": n_prompts * new,
            "equal_tokens": same}


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
    print(f"{args.iters} calls per timing, {args.repeats} alternating repeats; "
          "us per call, median (min-max)")
    print("| N | K | ksplit | M | bf16 us | fp8 us | bf16 GB/s | fp8 GB/s | "
          "bf16 / fp8 time | max abs diff |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for N, K in SHAPES:
        r = _child({"kind": "kernel", "N": N, "K": K, "iters": args.iters,
                    "repeats": args.repeats}, args.step_limit)
        for M in ROWS:
            row = r["rows"][str(M)]
            t16, t8 = row["times"]["bf16"], row["times"]["fp8"]
            m16, m8 = statistics.median(t16), statistics.median(t8)
            print(f"| {N} | {K} | {r['ksplit']} | {M} | {_fmt(t16, 1e6, 1)} | "
                  f"{_fmt(t8, 1e6, 1)} | {N * K * 2 / m16 / 1e9:.0f} | "
                  f"{N * (K + 4) / m8 / 1e9:.0f} | {m16 / m8:.2f}x | "
                  f"{row['maxdiff']:.2e} |", flush=True)


def run_e2e(args):
    r = _child({"kind": "e2e", "model": args.model, "n": args.prompts,
                "new": args.new, "repeats": args.repeats}, args.step_limit)
    print(f"{r['model']} (random weights): {len(r['lengths'])} prompts of "
          f"lengths {r['lengths']}, {r['new']} new tokens each, "
          f"{args.repeats} alternating repeats")
    print("| generate_batch weight_dtype | seconds | new tokens/s |")
    print("|---|---|---|")
    for name, ts in r["times"].items():
        print(f"| {name} | {_fmt(ts)} | "
              f"{_fmt([r['tokens'] / t for t in ts], 1.0, 0)} |")
    a = statistics.median(r["times"]["bf16"])
    b = statistics.median(r["times"]["fp8"])
    print(f"fp8 is {a / b:.3f}x the bf16 throughput; greedy tokens equal to "
          f"the bf16 run's, per prompt, of {r['new']}: {r['equal_tokens']}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("mode", nargs="?", choices=["kernel", "e2e"])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--model", default="llama_8b")
    ap.add_argument("--prompts", type=int, default=8)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--step-limit", type=float, default=240.0,
                    help="time limit of each GPU step in seconds")
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:  # child: one measurement, one JSON line
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("perf_linear_w8 needs a GPU")
        s = json.loads(args.step)
        if s["kind"] == "kernel":
            r = step_kernel(s["N"], s["K"], s["iters"], s["repeats"])
        else:
            r = step_e2e(s["model"], s["n"], s["new"], s["repeats"])
        print(json.dumps(r))
        return
    if args.mode is None:
        ap.error("mode is required: kernel or e2e")
    (run_kernel if args.mode == "kernel" else run_e2e)(args)


if __name__ == "__main__":
    main()
