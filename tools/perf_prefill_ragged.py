"""Chunked ragged prefill: attn_prefill_ragged against what the GPU path
could do before it.

  python tools/perf_prefill_ragged.py

Empty prefix (B=8, T=2048, lens=1): against the causal flash_attention forward
plus the transpose_bshd(v) it needs. A report, not a bar: the flash kernel
has a pre-transposed operand and 8 tuned waves.
With a prefix (B in {8, 1}, prefix 4096, T in {32, 256}): against ceil(T/8)
calls of attn_decode_ragged_multi, each streaming the whole cache.

The parent process never touches the GPU: every case runs in a fresh child
process under its own time limit, and the first child that fails, faults or
runs out of time ends the run. Inside a child both paths are warmed, then
alternated `--repeats` times, event-timed. The calls rotate over enough
separate KV caches (>= 1 GiB in total) that a timing is not served from the
256 MiB Infinity Cache. H=32, Hkv=8 (G=4), D=128, bf16. TF/s is the
shape-derived count 4*B*H*D*sum_t(keys of token t) over the median time.
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

H, HKV, D = 32, 8, 128
CASES = [(8, 0, 2048), (8, 4096, 32), (8, 4096, 256), (1, 4096, 32),
         (1, 4096, 256)]  # (B, prefix, T)


def step(B, P, T, iters, repeats):
    import torch

    from prime_amd import ops

    torch.manual_seed(0)
    dev = "cuda"
    Smax = P + T
    nbuf = max(2, -(-(1 << 30) // (2 * B * Smax * HKV * D * 2)))
    kcs = [torch.randn(B, Smax, HKV, D, device=dev).bfloat16() for _ in range(nbuf)]
    vcs = [torch.randn(B, Smax, HKV, D, device=dev).bfloat16() for _ in range(nbuf)]
    q = torch.randn(B, T, H, D, device=dev).bfloat16()
    lens = torch.full((B,), P + 1, dtype=torch.int32, device=dev)
    n_new = torch.full((B,), T, dtype=torch.int32, device=dev)

    def new(i):
        return ops.attn_prefill_ragged(q, kcs[i % nbuf], vcs[i % nbuf], lens, n_new)

    if P == 0:
        def old(i):  # flash_attention transposes v itself (transpose_bshd)
            return ops.flash_attention(q, kcs[i % nbuf], vcs[i % nbuf], causal=True)
    else:
        qs = [q[:, t:t + 8].contiguous() for t in range(0, T, 8)]
        ls = [lens + t for t in range(0, T, 8)]
        n8 = torch.full((B,), 8, dtype=torch.int32, device=dev)

        def old(i):
            return torch.cat([ops.attn_decode_ragged_multi(
                qc, kcs[i % nbuf], vcs[i % nbuf], l, n8)
                for qc, l in zip(qs, ls)], 1)

    fns = {"new": new, "old": old}
    diff = (new(0).float() - old(0).float()).abs().max().item()
    for fn in fns.values():
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(iters):
                fn(i)
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / 1e3 / iters)
    return {"times": times, "maxdiff": diff}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-limit", type=float, default=120.0,
                    help="time limit of each child process in seconds")
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:  # child: one case, one JSON line
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("perf_prefill_ragged needs a GPU")
        s = json.loads(args.step)
        print(json.dumps(step(s["B"], s["P"], s["T"], s["iters"], s["repeats"])))
        return
    print(f"H={H} Hkv={HKV} D={D} bf16, {args.iters} calls per timing, "
          f"{args.repeats} alternating repeats; us per repeat")
    print("| B | prefix | T | attn_prefill_ragged | TF/s | before | what "
          "'before' is | slowest new vs fastest before | max abs diff |")
    print("|---|---|---|---|---|---|---|---|---|")
    for B, P, T in CASES:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--step",
               json.dumps({"B": B, "P": P, "T": T, "iters": args.iters,
                           "repeats": args.repeats})]
        r = subprocess.run(cmd, capture_output=True, text=True,
                           timeout=args.step_limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"B={B} prefix={P} T={T} failed with exit status "
                             f"{r.returncode}; stopping")
        v = json.loads(r.stdout.strip().splitlines()[-1])
        new, old = v["times"]["new"], v["times"]["old"]
        flop = 4.0 * B * H * D * sum(P + 1 + t for t in range(T))
        us = lambda xs: " ".join(f"{x * 1e6:.1f}" for x in xs)  # noqa: E731
        what = "flash fwd + transpose_bshd(v)" if P == 0 else \
            f"{-(-T // 8)} attn_decode_ragged_multi calls"
        print(f"| {B} | {P} | {T} | {us(new)} | "
              f"{flop / statistics.median(new) / 1e12:.1f} | {us(old)} | {what} "
              f"| {min(old) / max(new):.2f}x | {v['maxdiff']:.1e} |", flush=True)


if __name__ == "__main__":
    main()
