"""Cases, inputs and digests for the flash attention bit-equality test.

One list, used by tools/record_attn_bits.py (which records the SHA-256 of
every output on a known-good build into tests/golden/attn_bits.json) and by
tests/test_attn_bits_gpu.py (which recomputes them on the current build and
also compares the same outputs with the fp32 CPU reference).

The shapes are the smallest at which each piece of the kernels can go wrong:

  - 32x32 ("v5") forward and dQ, S % 256 == 0: S = 256 is one q-block, whose
    waves 0-1 compute only their diagonal tile and whose waves 2-7 compute
    one or more unmasked tiles before it; S = 512 adds a second q-block.
    D = 64 and 128, group size H/Hkv = 1 and 4, one grid that is a multiple
    of 8 (XCD remap on) and one that is not (B = 1, H = 3).
  - document mask at S = 512: a document start inside a diagonal tile (37),
    starts on a 64-key edge (128, 448), a single-token document (300), and
    a row that is one document (nothing masked).
  - dK/dV: the shapes and document cases of tests/test_attn_dkv_gpu.py, in
    both launch modes, with the q loop in one and in two slices.
  - the 16x16 forward and dQ at a shape the 32x32 kernels would take,
    PRIME_ATTN_V5=0. The library reads that variable once per process, so
    the case runs in a process of its own.
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path
from typing import NamedTuple, Optional

import torch

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "attn_bits.json"
TOOL = ROOT / "tools" / "record_attn_bits.py"
OUTPUTS = ("o", "lse", "dq", "dk", "dv")


class Case(NamedTuple):
    name: str
    shape: tuple            # (B, S, H, Hkv, D)
    causal: bool
    doc: Optional[tuple]    # document starts per batch row, or None
    env: tuple              # ((variable, value), ...) set around the run
    own_process: bool       # the env is read once per process


# name -> (B, S, H, Hkv, D)
V5_SHAPES = {
    "s256_d128_g4": (2, 256, 4, 1, 128),   # grid 8: XCD remap on
    "s256_d64_g1": (1, 256, 3, 3, 64),     # grid 3: remap off
    "s512_d128_g1": (1, 512, 3, 3, 128),   # grid 6: remap off
    "s512_d64_g4": (2, 512, 4, 1, 64),     # grid 16: remap on
}

# row 0: 37 lies inside the diagonal tile of the wave that owns rows 32-63;
# 128 and 448 sit on 64-key edges; 300 is a single-token document, so rows
# 301.. of the wave that owns 288-319 see none of the keys of tile 128-191;
# row 1 is one document
V5_DOC = ((0, 37, 128, 300, 301, 448), (0,))
V5_DOC_SHAPES = {
    "doc512_d128_g4": (2, 512, 4, 1, 128),
    "doc512_d64_g1": (2, 512, 2, 2, 64),
}

# tests/test_attn_dkv_gpu.py: SHAPES and DOC_CASES
DKV_SHAPES = {
    "s128_d64_g4": (2, 128, 4, 1, 64),
    "s128_d128_g1": (2, 128, 2, 2, 128),
    "s256_d128_g4": (2, 256, 8, 2, 128),
    "s256_d64_g1": (2, 256, 1, 1, 64),
    "s384_d128_g4": (2, 384, 4, 1, 128),
    "s384_d64_g1": (2, 384, 2, 2, 64),
    "s192_d128_g4": (2, 192, 8, 2, 128),
    "s192_d64_g1": (2, 192, 1, 1, 64),
}
DKV_DOCS = {
    "doc256": ("s256_d128_g4", ((0, 1, 37, 128, 203), (0, 100, 171))),
    "doc384": ("s384_d64_g1", ((0, 50, 256, 383), (0, 131, 133, 301))),
}


def _cases():
    out = []
    for name, shape in V5_SHAPES.items():
        for causal in (True, False):
            out.append(Case(f"v5_{name}_{'causal' if causal else 'full'}",
                            shape, causal, None, (), False))
    for name, shape in V5_DOC_SHAPES.items():
        out.append(Case(f"v5_{name}", shape, True, V5_DOC, (), False))
    modes = [(("PRIME_ATTN_DKV_DIRECT", d), ("PRIME_AMD_DKV_SPLITS", s))
             for d in ("1", "0") for s in ("1", "2")]
    for env in modes:
        tag = f"{'direct' if env[0][1] == '1' else 'split'}{env[1][1]}"
        for name, shape in DKV_SHAPES.items():
            for causal in (True, False):
                out.append(Case(f"dkv_{name}_{'causal' if causal else 'full'}_{tag}",
                                shape, causal, None, env, False))
        for name, (shape, doc) in DKV_DOCS.items():
            out.append(Case(f"dkv_{name}_{tag}", DKV_SHAPES[shape], True, doc, env, False))
    out.append(Case("fallback16_s256_d128_g4_causal", V5_SHAPES["s256_d128_g4"], True,
                    None, (("PRIME_ATTN_V5", "0"),), True))
    return out


CASES = {c.name: c for c in _cases()}


def doc_start(case: Case):
    if case.doc is None:
        return None
    S = case.shape[1]
    ds = torch.zeros(len(case.doc), S, dtype=torch.int32)
    for b, row in enumerate(case.doc):
        for s in row:
            ds[b, s:] = s
    return ds


def split_qkv(qkv, H, Hkv, D):
    """q/k/v as strided views of one packed [B,S,(H+2Hkv)*D] buffer."""
    B, S, _ = qkv.shape
    q = qkv[..., : H * D].view(B, S, H, D)
    k = qkv[..., H * D: (H + Hkv) * D].view(B, S, Hkv, D)
    v = qkv[..., (H + Hkv) * D:].view(B, S, Hkv, D)
    return q, k, v


def inputs(case: Case):
    """bf16 inputs built on the CPU; they depend on the shape alone."""
    B, S, H, Hkv, D = case.shape
    g = torch.Generator().manual_seed(20240 + 7 * S + D + 3 * H + Hkv)
    qkv = (0.5 * torch.randn(B, S, (H + 2 * Hkv) * D, generator=g)).bfloat16()
    do = torch.randn(B, S, H, D, generator=g).bfloat16()
    return qkv, do


def run_here(case: Case) -> dict:
    """Forward and backward on the GPU in this process -> CPU tensors."""
    from prime_amd import ops

    _, _, H, Hkv, D = case.shape
    qkv, do = inputs(case)
    ds = doc_start(case)
    saved = {k: os.environ.get(k) for k, _ in case.env}
    os.environ.update(dict(case.env))
    try:
        buf = qkv.to("cuda").requires_grad_(True)
        q, k, v = split_qkv(buf, H, Hkv, D)
        o = ops.flash_attention(q, k, v, causal=case.causal,
                                doc_start=None if ds is None else ds.to("cuda"))
        lse = o.grad_fn.saved_tensors[4]
        o.backward(do.to("cuda"))
        dq, dk, dv = split_qkv(buf.grad, H, Hkv, D)
        got = dict(o=o.detach(), lse=lse, dq=dq, dk=dk, dv=dv)
        return {n: t.cpu().contiguous() for n, t in got.items()}
    finally:
        for k, old in saved.items():
            if old is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = old


def run(case: Case, tmp_dir) -> dict:
    """As run_here; a case whose environment the library reads only once
    per process runs in a fresh one, through the recording tool."""
    if not case.own_process:
        return run_here(case)
    path = Path(tmp_dir) / f"{case.name}.pt"
    subprocess.run([sys.executable, str(TOOL), "--one", case.name, "--dump", str(path)],
                   check=True, cwd=str(ROOT), timeout=300)
    return torch.load(path)


def digests(out: dict) -> dict:
    """SHA-256 of the raw bytes of every output."""
    return {n: hashlib.sha256(out[n].contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
            for n in OUTPUTS}


def reference(case: Case):
    """fp32 CPU reference: o and the gradients of q, k, v."""
    from prime_amd import ops

    _, _, H, Hkv, D = case.shape
    qkv, do = inputs(case)
    ref = qkv.float().requires_grad_(True)
    qr, kr, vr = split_qkv(ref, H, Hkv, D)
    o = ops.reference.attention(qr, kr, vr, causal=case.causal, doc_start=doc_start(case))
    o.backward(do.float())
    dq, dk, dv = (t.contiguous() for t in split_qkv(ref.grad, H, Hkv, D))
    return dict(o=o.detach(), dq=dq, dk=dk, dv=dv)


def load_golden() -> dict:
    return json.loads(GOLDEN.read_text())
