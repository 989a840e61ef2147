"""Paged KV cache: the block-table readers against their contiguous siblings.

  python tools/perf_kv_paged.py kernel   # timings (needs a GPU)
  python tools/perf_kv_paged.py memory   # cache bytes of a mixed batch (arithmetic)

kernel: for every shape, five variants of one attention call over the SAME
memory: the contiguous kernel, and the paged kernel over that cache viewed as
a pool (no copy) with an identity table and with a shuffled table (a random
permutation of all pages of the pool, so a sequence reads other sequences'
rows: the timing is what is compared, not the values), at P = 64 and 256.
Calls rotate over enough separate caches (>= 1 GiB in total) that nothing is
served from the 256 MiB Infinity Cache. The parent process never touches the
GPU: each measurement runs in a fresh child process under its own time limit,
`--procs` processes per shape, the shapes alternating; inside a process the
variants are warmed, then alternated `--repeats` times. The first step that
fails ends the run. The table lists ALL values, sorted.
"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

H, HKV, D = 32, 8, 128
# (kind, B, rows attended by the first query, T)
SHAPES = [("decode", 1, 512, 1), ("decode", 1, 4096, 1), ("decode", 8, 512, 1),
          ("decode", 8, 4096, 1), ("prefill", 8, 4096, 32),
          ("prefill", 8, 4096, 256)]
VARIANTS = ["contiguous", "identity P=64", "shuffled P=64", "identity P=256",
            "shuffled P=256"]


def step(kind, B, L, T, iters, repeats):
    import torch

    from prime_amd import ops

    torch.manual_seed(0)
    dev = "cuda"
    smax = -(-(L + (T if kind == "prefill" else 0)) // 256) * 256  # whole pages
    nbuf = max(2, -(-(1 << 30) // (2 * B * smax * HKV * D * 2)))
    kcs = torch.randn(nbuf, B, smax, HKV, D, device=dev, dtype=torch.bfloat16)
    vcs = torch.randn(nbuf, B, smax, HKV, D, device=dev, dtype=torch.bfloat16)
    q = torch.randn(B, T, H, D, device=dev, dtype=torch.bfloat16)
    lens = torch.full((B,), L + (kind == "prefill"), dtype=torch.int32, device=dev)
    n_new = torch.full((B,), T, dtype=torch.int32, device=dev)
    tables = {}
    for P in (64, 256):
        n = B * smax // P
        tables["identity", P] = torch.arange(n, dtype=torch.int32, device=dev).view(B, -1)
        tables["shuffled", P] = torch.randperm(n, device=dev).to(torch.int32).view(B, -1)

    def contiguous(i):
        if kind == "decode":
            return ops.attn_decode_ragged(q[:, 0], kcs[i % nbuf], vcs[i % nbuf], lens)
        return ops.attn_prefill_ragged(q, kcs[i % nbuf], vcs[i % nbuf], lens, n_new)

    def paged(order, P):
        def fn(i):
            c = ops.KVCachePaged(kcs[i % nbuf].view(-1, P, HKV, D),
                                 vcs[i % nbuf].view(-1, P, HKV, D),
                                 tables[order, P])
            if kind == "decode":
                return ops.attn_decode_ragged_paged(q[:, 0], c, lens)
            return ops.attn_prefill_ragged_paged(q, c, lens, n_new)
        return fn

    fns = {"contiguous": contiguous}
    for v in VARIANTS[1:]:
        order, p = v.split(" P=")
        fns[v] = paged(order, int(p))
    same = all(torch.equal(fns[v](0), contiguous(0)) for v in VARIANTS[1::2])
    for fn in fns.values():  # warm every variant (code objects, workspace)
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            a.record()
            for i in range(iters):
                fn(i)
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / iters)  # us per call
    return {"times": times, "nbuf": nbuf, "smax": smax,
            "identity_equals_contiguous": same}


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
    res = {s: {v: [] for v in VARIANTS} for s in SHAPES}
    same = True
    for _ in range(args.procs):
        for s in SHAPES:
            r = _child({"shape": list(s), "iters": args.iters,
                        "repeats": args.repeats}, args.step_limit)
            same = same and r["identity_equals_contiguous"]
            print(f"done: {s}", file=sys.stderr, flush=True)
            for v in VARIANTS:
                res[s][v] += r["times"][v]
    print(f"H={H} Hkv={HKV} D={D} bf16; us per call, {args.iters} calls per "
          f"timing, {args.procs} processes x {args.repeats} alternating "
          f"repeats, all values sorted; identity table == contiguous bit for "
          f"bit: {same}")
    print("| kernel | B | L | T | " + " | ".join(VARIANTS) + " |")
    print("|---|---|---|---|" + "---|" * len(VARIANTS))
    for s in SHAPES:
        cells = [" ".join(f"{x:.1f}" for x in sorted(res[s][v])) for v in VARIANTS]
        print(f"| {s[0]} | {s[1]} | {s[2]} | {s[3]} | " + " | ".join(cells) + " |",
              flush=True)


def run_memory(args):
    """Per-layer cache bytes of generate_batch for one 8k prompt and seven
    200-token prompts, by its own sizing rules."""
    prompts, new, P = [8192] + [200] * 7, args.new, 64
    total = max(prompts) + new
    smax = -(-max(total, 1024) // 64) * 64
    row = 2 * HKV * D * 2  # K and V, bf16
    pages = sum(-(-(p + new) // P) for p in prompts)
    print(f"prompts {prompts}, {new} new tokens each, Hkv={HKV} D={D} bf16")
    print(f"contiguous: 8 slots x {smax} rows = {8 * smax * row / 2**20:.1f} MiB per layer")
    print(f"paged P={P}: {pages} pages = {pages * P} rows = "
          f"{pages * P * row / 2**20:.1f} MiB per layer "
          f"({8 * smax / (pages * P):.1f}x less)")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("mode", nargs="?", choices=["kernel", "memory"])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--step-limit", type=float, default=180.0,
                    help="time limit of each GPU step in seconds")
    ap.add_argument("--step", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:  # child: one measurement, one JSON line
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("perf_kv_paged kernel needs a GPU")
        s = json.loads(args.step)
        print(json.dumps(step(*s["shape"], s["iters"], s["repeats"])))
        return
    if args.mode is None:
        ap.error("mode is required: kernel or memory")
    (run_kernel if args.mode == "kernel" else run_memory)(args)


if __name__ == "__main__":
    main()
