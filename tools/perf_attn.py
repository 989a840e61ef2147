"""Standalone flash-attention kernel timing at the bench shape.

Usage (GPU box): python tools/perf_attn.py [iters] [--non-causal]
                     [--seq S] [--batch B] [--doc-len N[,N...]] [--repeats R]
Prints achieved TF/s for fwd / bwd with causal FLOP counting.

--doc-len N times the document-masked kernels with uniform documents of N
tokens per row (N = S: one document, the masked path with nothing masked).
Masked FLOPs count only visible (q, k) pairs. The plain-causal time of the
same run is printed next to it: the variants alternate in one process,
each warmed first, R repeats each.
"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from prime_amd.ops.functional import _FlashAttention


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("iters", nargs="?", type=int, default=20)
    ap.add_argument("--non-causal", action="store_true")
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--doc-len", type=str, default=None)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    iters = args.iters
    causal = not args.non_causal
    B, S, H, Hkv, D = args.batch, args.seq, 32, 8, 128
    torch.manual_seed(0)
    dev = "cuda:0"
    q = torch.randn(B, S, H, D, device=dev).bfloat16().requires_grad_(True)
    k = torch.randn(B, S, Hkv, D, device=dev).bfloat16().requires_grad_(True)
    v = torch.randn(B, S, Hkv, D, device=dev).bfloat16().requires_grad_(True)
    do = torch.randn(B, S, H, D, device=dev).bfloat16()

    def flops(pairs):
        # attention FLOPs (fwd): 2 matmuls * visible (q,k) pairs * D * H * B * 2
        fwd = 2 * 2 * pairs * D * H * B
        return fwd, 2.5 * fwd  # 5 matmuls in bwd vs 2 in fwd

    def timeit(fn, n):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    def measure(doc_start):
        extra = () if doc_start is None else (doc_start,)

        def fwd():
            _FlashAttention.apply(q, k, v, causal, D**-0.5, *extra)

        def fb():
            out = _FlashAttention.apply(q, k, v, causal, D**-0.5, *extra)
            out.backward(do)
            q.grad = k.grad = v.grad = None

        t_fwd = timeit(fwd, iters)  # forward only
        t_fb = timeit(fb, iters)    # fwd+bwd (isolates bwd by subtraction)
        return t_fwd, t_fb - t_fwd

    def report(tag, t_fwd, t_bwd, pairs):
        ff, bf = flops(pairs)
        print(f"{tag}fwd : {t_fwd*1e3:7.3f} ms  {ff/t_fwd/1e12:7.1f} TF/s")
        print(f"{tag}bwd : {t_bwd*1e3:7.3f} ms  {bf/t_bwd/1e12:7.1f} TF/s")
        print(f"{tag}f+b : {(t_fwd+t_bwd)*1e3:7.3f} ms  "
              f"{(ff+bf)/(t_fwd+t_bwd)/1e12:7.1f} TF/s")

    causal_pairs = S * S / (2 if causal else 1)
    if args.doc_len is None:
        report("", *measure(None), causal_pairs)
        return

    if not causal:
        sys.exit("--doc-len needs causal attention")
    variants = [("causal", None, causal_pairs)]
    idx = torch.arange(S, device=dev, dtype=torch.int32)
    for n in (int(x) for x in args.doc_len.split(",")):
        ds = (idx // n * n).expand(B, S).contiguous()
        # visible pairs, counted like the causal S*S/2: n*n/2 per document
        pairs = sum(m * m / 2 for m in [n] * (S // n) + [S % n])
        variants.append((f"doc{n}", ds, pairs))
    for _, ds, _ in variants:  # warm every variant before any timing
        measure(ds)
    times = {name: [] for name, _, _ in variants}
    for _ in range(args.repeats):  # alternate the variants
        for name, ds, _ in variants:
            times[name].append(measure(ds))
    print(f"B={B} S={S} H={H} Hkv={Hkv} D={D} iters={iters} repeats={args.repeats}")
    for name, _, pairs in variants:
        fw = sorted(t[0] for t in times[name])
        bw = sorted(t[1] for t in times[name])
        print(f"{name:>8} fwd ms " + " ".join(f"{t*1e3:.3f}" for t in fw)
              + "   bwd ms " + " ".join(f"{t*1e3:.3f}" for t in bw))
        report(f"{name:>8} median ", fw[len(fw) // 2], bw[len(bw) // 2], pairs)


if __name__ == "__main__":
    main()
