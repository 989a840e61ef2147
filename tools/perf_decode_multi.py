"""Multi-token ragged decode: one T-token attn_decode_ragged_multi call against
T calls of attn_decode_ragged (what verifying T drafted tokens costs without
it), and against one single-token call (the byte-count expectation).

  python tools/perf_decode_multi.py
  python tools/perf_decode_multi.py --fp8

With --fp8 the three paths are one T-token attn_decode_ragged_multi_fp8 call
over an fp8 (e4m3) cache, one bf16 T-token call at the same shape, and T
calls of attn_decode_ragged_fp8.

The parent process never touches the GPU: every (B, L) shape runs in a
fresh child process under its own time limit, `--procs` times over, and the
first child that fails, faults or runs out of time ends the run. Inside a
child the paths are warmed, then alternated `--repeats` times for every T.
The table gives the median and (min-max) over all repeats of all processes.

The calls rotate over enough separate KV caches (>= 1 GiB in total) that a
timing is not served from the 256 MiB Infinity Cache. Shapes are those of
profiles/decode_ragged.md: H=32, Hkv=8 (G=4), D=128, bf16, uniform lengths;
token t of the T attends to L - T + 1 + t rows, the last one to all L.
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
SHAPES = [(1, 4096), (8, 4096), (8, 512)]  # (B, L)
TS = (2, 4, 8)


def _fmt(xs, digits=1):
    xs = [x * 1e6 for x in xs]
    return (f"{statistics.median(xs):.{digits}f} "
            f"({min(xs):.{digits}f}-{max(xs):.{digits}f})")


def step(B, L, iters, repeats, fp8=False):
    import torch

    from prime_amd import ops

    torch.manual_seed(0)
    dev = "cuda"
    # >= 1 GiB of the smaller (fp8) caches too
    nbuf = max(2, -(-(1 << 30) // (2 * B * L * HKV * D * (1 if fp8 else 2))))
    kcs = [torch.randn(B, L, HKV, D, device=dev).bfloat16() for _ in range(nbuf)]
    vcs = [torch.randn(B, L, HKV, D, device=dev).bfloat16() for _ in range(nbuf)]
    c8s = []
    for kc, vc in zip(kcs, vcs) if fp8 else ():
        c8s.append(ops.kv_cache_fp8(B, L, HKV, D, dev))
        ops.kv_store_fp8(c8s[-1], kc, vc, 0)
    out = {}
    for T in TS:
        q = torch.randn(B, T, H, D, device=dev).bfloat16()
        qs = [q[:, t].contiguous() for t in range(T)]
        lens = [torch.full((B,), L - T + 1 + t, dtype=torch.int32, device=dev)
                for t in range(T)]
        n_new = torch.full((B,), T, dtype=torch.int32, device=dev)

        def multi(i):
            return ops.attn_decode_ragged_multi(q, kcs[i % nbuf], vcs[i % nbuf],
                                                lens[0], n_new)

        def singles(i):
            return [ops.attn_decode_ragged(qs[t], kcs[i % nbuf], vcs[i % nbuf],
                                           lens[t]) for t in range(T)]

        def one(i):
            return ops.attn_decode_ragged(qs[-1], kcs[i % nbuf], vcs[i % nbuf],
                                          lens[-1])

        def multi_fp8(i):
            return ops.attn_decode_ragged_multi_fp8(q, c8s[i % nbuf], lens[0],
                                                    n_new)

        def singles_fp8(i):
            return [ops.attn_decode_ragged_fp8(qs[t], c8s[i % nbuf], lens[t])
                    for t in range(T)]

        if fp8:
            fns = {"multi": multi_fp8, "singles": singles_fp8, "one": multi}
        else:
            fns = {"multi": multi, "singles": singles, "one": one}
        diff = (fns["multi"](0).float()
                - torch.stack(fns["singles"](0), 1).float()).abs().max()
        for fn in fns.values():  # warm every path
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
        out[str(T)] = {"times": times, "maxdiff": diff.item()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--procs", type=int, default=3, help="process repeats")
    ap.add_argument("--step-limit", type=float, default=120.0,
                    help="time limit of each child process in seconds")
    ap.add_argument("--fp8", action="store_true",
                    help="time the fp8-cache T-token op against the bf16 "
                    "T-token op and T fp8 single-token calls")
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:  # child: one shape, one JSON line
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("perf_decode_multi needs a GPU")
        s = json.loads(args.step)
        print(json.dumps(step(s["B"], s["L"], s["iters"], s["repeats"],
                              s.get("fp8", False))))
        return
    print(f"H={H} Hkv={HKV} D={D} bf16, {args.iters} calls per timing, "
          f"{args.repeats} alternating repeats x {args.procs} processes; "
          f"us, median (min-max)")
    if args.fp8:
        print("| B | L | T | one fp8 T-token call | T fp8 single-token calls | "
              "one bf16 T-token call | fp8 multi vs T fp8 singles | fp8 multi "
              "/ bf16 multi | max abs diff |")
    else:
        print("| B | L | T | one T-token call | T single-token calls | one "
              "single-token call | multi vs T singles | multi / one single | "
              "max abs diff |")
    print("|---|---|---|---|---|---|---|---|---|")
    for B, L in SHAPES:
        acc = {}
        for _ in range(args.procs):
            cmd = [sys.executable, str(Path(__file__).resolve()), "--step",
                   json.dumps({"B": B, "L": L, "iters": args.iters,
                               "repeats": args.repeats, "fp8": args.fp8})]
            r = subprocess.run(cmd, capture_output=True, text=True,
                               timeout=args.step_limit)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"B={B} L={L} failed with exit status "
                                 f"{r.returncode}; stopping")
            for T, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
                a = acc.setdefault(T, {"multi": [], "singles": [], "one": [],
                                       "maxdiff": 0.0})
                for k, ts in v["times"].items():
                    a[k] += ts
                a["maxdiff"] = max(a["maxdiff"], v["maxdiff"])
        for T, a in acc.items():
            m, s, o = (statistics.median(a[k]) for k in ("multi", "singles", "one"))
            print(f"| {B} | {L} | {T} | {_fmt(a['multi'])} | {_fmt(a['singles'])} "
                  f"| {_fmt(a['one'])} | {s / m:.2f}x | {m / o:.2f} | "
                  f"{a['maxdiff']:.1e} |", flush=True)


if __name__ == "__main__":
    main()
