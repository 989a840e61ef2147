"""Record the output bits of flash attention on a known-good build.

Usage (GPU box): python tools/record_attn_bits.py [--out PATH]
                 python tools/record_attn_bits.py --one CASE --dump FILE

Runs every case of tests/attn_bits_cases.py forward and backward on the GPU
and writes the SHA-256 of the raw bytes of o, lse, dq, dk and dv per case to
tests/golden/attn_bits.json. tests/test_attn_bits_gpu.py recomputes the
digests on the current build and compares, so a kernel change that is meant
to keep every bit is checked against the build the file was recorded on:
record on the parent commit's build (PRIME_AMD_LIB_PATH selects a library),
never on the change under test.

--one CASE --dump FILE runs a single case in this process and saves its
output tensors; the test uses it for the case that needs a fresh process.
"""
import argparse
import json
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from tests import attn_bits_cases as ab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=str(ab.GOLDEN))
    ap.add_argument("--one", type=str, default=None)
    ap.add_argument("--dump", type=str, default=None)
    args = ap.parse_args()
    if args.one is not None:
        if args.dump is None:
            sys.exit("--one needs --dump FILE")
        torch.save(ab.run_here(ab.CASES[args.one]), args.dump)
        return
    golden = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, case in ab.CASES.items():
            golden[name] = ab.digests(ab.run(case, tmp))
            print(name, golden[name]["o"][:12], flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(golden, indent=1, sort_keys=True) + "\n")
    print(f"wrote {len(golden)} cases to {args.out}")


if __name__ == "__main__":
    main()
