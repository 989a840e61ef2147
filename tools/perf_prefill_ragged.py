"""Chunked ragged prefill: attn_prefill_ragged against what the GPU path
could do before it.

  python tools/perf_prefill_ragged.py [--fp8]

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
256 MiB Infinity Cache. H=32, Hkv=8 (G=4), D=128 (--head-dim 64 for the
D=64 kernels), bf16. TF/s is the
shape-derived count 4*B*H*D*sum_t(keys of token t) over the median time.

--fp8: attn_prefill_ragged_fp8 over KVCacheFp8 caches (kv_store_fp8 of the
same randn rows). "Before" is ceil(T/8) attn_decode_ragged_multi_fp8 calls
(with a prefix; an empty prefix had no fp8 route). A third path, the bf16
attn_prefill_ragged on the dequantised caches, alternates with them: its
times and the maximum absolute difference to it are reported without a bar.
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


def step(B, P, T, iters, repeats, fp8=False):
    import torch

    from prime_amd import ops

    torch.manual_seed(0)
    dev = "cuda"
    Smax = P + T
    row = (D + 4) if fp8 else 2 * D  # bytes of a cache row and kv head
    nbuf = max(2, -(-(1 << 30) // (2 * B * Smax * HKV * row)))
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
    if fp8:
        cs = [ops.kv_cache_fp8(B, Smax, HKV, D, dev) for _ in range(nbuf)]
        for i, c in enumerate(cs):  # then the bf16 caches hold its values
            ops.kv_store_fp8(c, kcs[i], vcs[i], 0)
            kd, vd = ops.kv_cache_dequant(c)
            kcs[i], vcs[i] = kd.bfloat16(), vd.bfloat16()

        def new8(i):
            return ops.attn_prefill_ragged_fp8(q, cs[i % nbuf], lens, n_new)

        def old8(i):
            return torch.cat([ops.attn_decode_ragged_multi_fp8(
                qc, cs[i % nbuf], l, n8) for qc, l in zip(qs, ls)], 1)

        fns = {"new": new8, "bf16": new}
        if P:
            fns["old"] = old8
        old = new  # the difference reported is that to the bf16 kernel
        new = new8
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


def us(xs):
    return " ".join(f"{x * 1e6:.1f}" for x in xs)


def run_case(args, B, P, T, fp8):
    """One case in a fresh child process; its JSON result."""
    cmd = [sys.executable, str(Path(__file__).resolve()), "--head-dim", str(D),
           "--step",
           json.dumps({"B": B, "P": P, "T": T, "iters": args.iters,
                       "repeats": args.repeats, "fp8": fp8})]
    r = subprocess.run(cmd, capture_output=True, text=True,
                       timeout=args.step_limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"B={B} prefix={P} T={T} failed with exit status "
                         f"{r.returncode}; stopping")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main_fp8(args):
    print(f"H={H} Hkv={HKV} D={D}, fp8 KV cache, {args.iters} calls per "
          f"timing, {args.repeats} alternating repeats; us per repeat")
    print("| B | prefix | T | attn_prefill_ragged_fp8 | TF/s | "
          "ceil(T/8) attn_decode_ragged_multi_fp8 calls | slowest new vs "
          "fastest before | bf16 attn_prefill_ragged | median bf16 / median "
          "fp8 | max abs diff to bf16 |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for B, P, T in CASES:
        v = run_case(args, B, P, T, True)
        t = v["times"]
        flop = 4.0 * B * H * D * sum(P + 1 + k for k in range(T))
        med = statistics.median(t["new"])
        before = f"{us(t['old'])} | {min(t['old']) / max(t['new']):.2f}x" \
            if "old" in t else "none | -"
        print(f"| {B} | {P} | {T} | {us(t['new'])} | {flop / med / 1e12:.1f} | "
              f"{before} | {us(t['bf16'])} | "
              f"{statistics.median(t['bf16']) / med:.2f} | {v['maxdiff']:.1e} |",
              flush=True)


def main():
    global D
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-limit", type=float, default=120.0,
                    help="time limit of each child process in seconds")
    ap.add_argument("--fp8", action="store_true",
                    help="the fp8-cache kernel (see the module docstring)")
    ap.add_argument("--head-dim", type=int, default=D, choices=(64, 128))
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    D = args.head_dim
    if args.step:  # child: one case, one JSON line
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("perf_prefill_ragged needs a GPU")
        s = json.loads(args.step)
        print(json.dumps(step(s["B"], s["P"], s["T"], s["iters"], s["repeats"],
                              s["fp8"])))
        return
    if args.fp8:
        return main_fp8(args)
    print(f"H={H} Hkv={HKV} D={D} bf16, {args.iters} calls per timing, "
          f"{args.repeats} alternating repeats; us per repeat")
    print("| B | prefix | T | attn_prefill_ragged | TF/s | before | what "
          "'before' is | slowest new vs fastest before | max abs diff |")
    print("|---|---|---|---|---|---|---|---|---|")
    for B, P, T in CASES:
        v = run_case(args, B, P, T, False)
        new, old = v["times"]["new"], v["times"]["old"]
        flop = 4.0 * B * H * D * sum(P + 1 + t for t in range(T))
        what = "flash fwd + transpose_bshd(v)" if P == 0 else \
            f"{-(-T // 8)} attn_decode_ragged_multi calls"
        print(f"| {B} | {P} | {T} | {us(new)} | "
              f"{flop / statistics.median(new) / 1e12:.1f} | {us(old)} | {what} "
              f"| {min(old) / max(new):.2f}x | {v['maxdiff']:.1e} |", flush=True)


if __name__ == "__main__":
    main()
