"""Cases, inputs and digests for the serving attention bit-equality test.

One list, used by tools/record_attn_bits.py --suite serving (which records
the SHA-256 of every output on a known-good build into
tests/golden/serving_bits.json) and by tests/test_serving_bits_gpu.py (which
recomputes them on the current build). "Paged equals contiguous"
(tests/test_kv_paged_gpu.py) still holds if both kernels change together;
this pins both to the bits of the build the file was recorded on.

One case per (D, G) instantiation of the four bf16 kernels (ragged decode and
chunked prefill, contiguous and paged), with the shapes of
tests/test_kv_paged_gpu.py::test_decode and ::test_prefill: every length
around a page and a chunk edge, an idle slot, a length beyond Smax, dead
queries, NaN in the dead pages. The page size and the split cycle over the
cases so that each P and one / several splits occur for each kernel.
"""
from __future__ import annotations

import hashlib
import json
from pathlib import Path
from typing import NamedTuple

import torch

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "serving_bits.json"
OUTPUTS = ("decode", "decode_paged", "prefill", "prefill_paged")


class Case(NamedTuple):
    name: str
    D: int
    G: int
    P: int
    decode_split: int   # 256: four splits of one chunk; 512: two of two
    prefill_split: int  # 128: several splits; 384: one (two at P = 256)


def _cases():
    out = []
    for i, (D, G) in enumerate((D, G) for D in (64, 128) for G in (1, 2, 4, 8)):
        P = (64, 128, 256)[i % 3]
        out.append(Case(f"d{D}_g{G}_p{P}", D, G, P, (256, 512)[i % 2],
                        (128, 384)[(i // 2) % 2]))
    return out


CASES = {c.name: c for c in _cases()}


def _paged(ops, kc, vc, P, live, g):
    """test_kv_paged_gpu._paged with the generator's permutation: a pool
    holding the live pages of kc, vc behind a shuffled table; dead pages are
    NaN and their entries invalid."""
    B, Smax, Hkv, D = kc.shape
    mp = Smax // P
    cache = ops.kv_cache_paged(B * mp + 5, P, B, mp, Hkv, D, kc.device)
    cache.k.fill_(float("nan")), cache.v.fill_(float("nan"))
    perm = torch.randperm(B * mp + 5, generator=g)[:B * mp].view(B, mp).tolist()
    for b in range(B):
        for j in range(mp):
            if j * P < live[b]:
                cache.table[b, j] = perm[b][j]
                cache.k[perm[b][j]] = kc[b, j * P:(j + 1) * P]
                cache.v[perm[b][j]] = vc[b, j * P:(j + 1) * P]
            else:
                cache.table[b, j] = (-1, B * mp + 12)[j & 1]
    return cache


def run_here(case: Case, dev="cuda:0") -> dict:
    """The four ops on the GPU -> CPU tensors. Inputs are drawn on the CPU
    from a generator seeded by the case alone."""
    from prime_amd import ops

    D, G, P = case.D, case.G, case.P
    g = torch.Generator().manual_seed(5150 + 7 * D + 3 * G + P)

    def rand(*shape):
        return torch.randn(*shape, generator=g).to(dev, dtype=torch.bfloat16)

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device=dev)

    Hkv = 2 if G == 1 else 1
    H = Hkv * G
    out = {}
    # ---- decode: test_kv_paged_gpu.py::test_decode
    Smax = 1024
    lens = [0, 1, P - 1, P, P + 1, 255, 256, 257, Smax, Smax + 1000]
    B = len(lens)
    q, kc, vc = rand(B, H, D), rand(B, Smax, Hkv, D), rand(B, Smax, Hkv, D)
    cache = _paged(ops, kc, vc, P, [min(x, Smax) for x in lens], g)
    out["decode"] = ops.attn_decode_ragged(q, kc, vc, i32(lens),
                                           split_rows=case.decode_split)
    out["decode_paged"] = ops.attn_decode_ragged_paged(
        q, cache, i32(lens), split_rows=case.decode_split)
    # ---- prefill: test_kv_paged_gpu.py::test_prefill
    T, Smax = 128 // G + 5, -(-320 // P) * P
    lens = [L for L in (1, 63, 64, P, P + 1, Smax - T + 1) for _ in range(4)]
    n_new = [T, T - 1, 1, 0] * 6
    B = len(lens)
    n = [min(x, T, Smax - L + 1) for L, x in zip(lens, n_new)]
    q, kc, vc = rand(B, T, H, D), rand(B, Smax, Hkv, D), rand(B, Smax, Hkv, D)
    cache = _paged(ops, kc, vc, P,
                   [L + x - 1 if x else 0 for L, x in zip(lens, n)], g)
    out["prefill"] = ops.attn_prefill_ragged(
        q, kc, vc, i32(lens), i32(n_new), split_rows=case.prefill_split)
    out["prefill_paged"] = ops.attn_prefill_ragged_paged(
        q, cache, i32(lens), i32(n_new), split_rows=case.prefill_split)
    return {k: v.cpu().contiguous() for k, v in out.items()}


def digests(out: dict) -> dict:
    """SHA-256 of the raw bytes of every output."""
    return {n: hashlib.sha256(out[n].view(torch.uint8).numpy().tobytes()).hexdigest()
            for n in OUTPUTS}


def load_golden() -> dict:
    return json.loads(GOLDEN.read_text())
