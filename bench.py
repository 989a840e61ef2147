"""Flagship benchmark: INTELLECT-1 10B DiLoCo H=100 training throughput.

Driver contract: `python bench.py --gpus N --steps K --warmup W` (N>1 via
torch.distributed.run, one rank per GPU over RCCL). Each rank is one DiLoCo
worker (worker_size=1, weak scaling: fixed per-GPU batch); the outer int8
ring all-reduce runs every H=100 inner steps (and once during warmup so the
path is exercised even when K < H). Rank 0 prints ONE JSON line with the
whole-job tokens/sec.

A plain run does only what the headline needs: set up, warm up (including
the one timed outer sync the headline amortizes), time K steps, print the
line. `--dump-outputs DIR` additionally writes what the last timed step
produced as DIR/<name>.npy (same arguments -> same seeds and inputs, so
two builds can be compared output for output). Secondary measurements
belong behind `--full`.

Host-memory sizing at N=8 x 10B: each rank keeps fp32 theta_outer +
momentum on the host (2 x 42 GB), i.e. ~672 GB across the node; the
allocation is pinned only when MemAvailable comfortably covers it
(PRIME_AMD_OUTER_PIN to override) and falls back to pageable otherwise.
"""
from __future__ import annotations

import argparse
import json
import os
import tempfile
import time

import torch


# --dump-outputs: elements sampled from each flat tensor (3 x 16 MiB as fp32)
_DUMP_SAMPLE = 1 << 22


def dump_outputs(trainer, loss, out_dir: str) -> None:
    """Write what the last timed train_step() left its caller: the returned
    loss and the state it updated in place (bf16 weights, fp32 master
    weights, gradients). The flat tensors are too large to store whole, so
    a fixed seeded index sample of each is written, as float32 .npy."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    flat = trainer.flat
    n = flat.flat_w.numel()
    if n > _DUMP_SAMPLE:
        g = torch.Generator()
        g.manual_seed(0)
        idx = torch.randint(0, n, (_DUMP_SAMPLE,), generator=g).sort().values
    else:
        idx = torch.arange(n)
    idx = idx.to(flat.flat_w.device)
    arrays = {
        "loss": torch.zeros(1) if loss is None else loss.reshape(1),
        "weights_sample": flat.flat_w.index_select(0, idx),
        "master_weights_sample": flat.master32.index_select(0, idx),
        "grads_sample": flat.flat_grad.index_select(0, idx),
    }
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"),
                t.detach().float().cpu().numpy())


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="intellect_10b")
    ap.add_argument("--seq-len", type=int, default=2048)
    ap.add_argument("--micro-batch", type=int, default=8)
    ap.add_argument("--h", type=int, default=100, help="DiLoCo inner steps per outer sync")
    ap.add_argument("--no-outer-warmup", action="store_true")
    ap.add_argument("--fp8-dgrad", action="store_true",
                    help="with --fp8: dX GEMMs in e5m2 too")
    ap.add_argument("--fp8-wgrad", action="store_true",
                    help="with --fp8 --fp8-dgrad: dW GEMMs in fp8 too")
    ap.add_argument("--fp8", action="store_true",
                    help="opt-in fp8 forward linears (NOT the headline "
                         "contract dtype; reported as bf16+fp8fwd)")
    ap.add_argument("--ckpt", choices=["on", "off"], default="off",
                    help="activation checkpointing (off: 288 GB HBM fits the "
                         "10B config's activations; recompute costs ~25%%)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed "
                         "step produced (loss, seeded samples of the weights, "
                         "fp32 master weights and gradients) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements (none yet)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", 1))
    n_gpus = world if world > 1 else args.gpus
    if world == 1:
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    rank = int(os.environ.get("RANK", 0))

    from prime_amd.train import Trainer
    from prime_amd.utils.config import (
        DataSection, DilocoConfig, MetricsConfig, ModelConfig, TrainConfig,
    )
    from prime_amd.utils.metrics import mfu as mfu_of

    cfg = TrainConfig(
        run_name="bench",
        steps=args.steps,
        model=ModelConfig(
            name=args.model, seq_len=args.seq_len,
            activation_checkpointing=(args.ckpt == "on"),
            fp8=args.fp8, fp8_dgrad=args.fp8_dgrad, fp8_wgrad=args.fp8_wgrad,
        ),
        data=DataSection(kind="synthetic", micro_batch_size=args.micro_batch),
        diloco=DilocoConfig(H=args.h, quant_int8=True, outer_device="auto"),
        metrics=MetricsConfig(log_interval=10**9),
    )
    # per-user default: a fixed name in a shared temp dir left behind by
    # another account is not writable
    run_dir = os.environ.get("BENCH_RUN_DIR") or os.path.join(
        tempfile.gettempdir(), f"prime_amd_bench_{os.getuid()}")
    trainer = Trainer(cfg, run_dir=run_dir)
    dev = trainer.device

    # ---- warmup (incl. one outer sync so ring/host-offload path is hot).
    # The outer step is TIMED here and folded into the headline as an
    # amortized per-inner-step cost (steps/H outer boundaries per window):
    # the printed value is then defensible for any (steps, H) even when
    # the timed window itself spans no boundary.
    for _ in range(args.warmup):
        trainer.train_step()
    t_outer = 0.0
    if not args.no_outer_warmup:
        trainer.mesh.barrier()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        t1 = time.perf_counter()
        trainer.diloco.outer_step()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        t_outer = time.perf_counter() - t1
    trainer.mesh.barrier()
    if dev.type == "cuda":
        torch.cuda.synchronize()

    # ---- timed region
    outer_before = trainer.diloco.outer_step_count
    loss = None
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = trainer.train_step()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    trainer.mesh.barrier()
    elapsed = time.perf_counter() - t0
    outer_in_window = trainer.diloco.outer_step_count - outer_before

    # max over ranks
    if trainer.mesh.initialized:
        import torch.distributed as dist

        t = torch.tensor([elapsed], device=dev if dev.type == "cuda" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t)

    # max the outer-step time over ranks too
    if trainer.mesh.initialized and t_outer > 0:
        import torch.distributed as dist

        t = torch.tensor([t_outer], device=dev if dev.type == "cuda" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        t_outer = float(t)

    tokens_per_step_per_gpu = args.micro_batch * args.seq_len
    total_tokens = tokens_per_step_per_gpu * args.steps * n_gpus
    tps_inner = total_tokens / elapsed
    # headline includes the amortized DiLoCo outer sync: steps/H
    # boundaries belong to a window of this many inner steps, minus any
    # boundary the window ALREADY contained (K >= H runs would otherwise
    # be charged twice)
    owed = max(0.0, args.steps / max(1, args.h) - outer_in_window)
    elapsed_incl = elapsed + t_outer * owed
    tps = total_tokens / elapsed_incl
    tps_gpu = tps / n_gpus
    mfu = mfu_of(tps_gpu, trainer.flops_per_token)

    if rank == 0 and args.dump_outputs:
        dump_outputs(trainer, loss, args.dump_outputs)

    if rank == 0:
        print(json.dumps({
            "metric": "tokens_per_sec",
            "value": tps,
            "tokens_per_sec_inner": tps_inner,
            "ms_per_outer_step": 1000.0 * t_outer,
            "unit": "tokens/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1000.0 * elapsed_incl / args.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": ("bf16+fp8fwd" + ("+dgrad" if args.fp8_dgrad else "")
                      + ("+wgrad" if args.fp8_wgrad else "")
                      if args.fp8 else "bf16"),
            "data": "synthetic",
            "mfu": mfu,
            # BASELINE.md convention: record the peak used for MFU (DENSE
            # bf16; AMD's 5 PF headline is 2:1-sparse)
            "mfu_peak_flops": 2.5e15,
            "config": {
                "model": args.model,
                "global_batch": args.micro_batch * n_gpus,
                "seq_len": args.seq_len,
                "parallelism": f"diloco{n_gpus}_h{args.h}_int8ring",
            },
        }), flush=True)
    trainer.close()


if __name__ == "__main__":
    main()
