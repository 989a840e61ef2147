"""Sequence parallelism (Ulysses head-scatter) on CPU/gloo: the a2a
round-trip, gradient flow, and a 2-rank SP Trainer matching a 1-rank
full-context run exactly (same seed/data)."""
import torch

from tests.conftest import SCRATCH, run_distributed


def _a2a_worker(rank, world):
    import torch.distributed as dist

    from prime_amd.parallel.seqpar import (_GatherHeads, _ScatterHeads,
                                           ulysses_attention)

    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(7)  # same full tensors on both ranks
    B, S, H, Hkv, D = 2, 16 * world, 2 * world, world, 16
    q_full = torch.randn(B, S, H, D)
    k_full = torch.randn(B, S, Hkv, D)
    v_full = torch.randn(B, S, Hkv, D)
    Sl = S // world
    q = q_full[:, rank * Sl : (rank + 1) * Sl].clone().requires_grad_(True)

    # scatter->gather round-trips
    g = _ScatterHeads.apply(q, None)
    assert g.shape == (B, S, H // world, D)
    back = _GatherHeads.apply(g, None)
    torch.testing.assert_close(back, q)

    # full SP attention vs single-process reference on the full tensors
    from prime_amd import ops

    k = k_full[:, rank * Sl : (rank + 1) * Sl].clone().requires_grad_(True)
    v = v_full[:, rank * Sl : (rank + 1) * Sl].clone().requires_grad_(True)
    o = ulysses_attention(q, k, v, causal=True, group=None)
    ref = ops.reference.attention(q_full.double(), k_full.double(),
                                  v_full.double(), causal=True)
    torch.testing.assert_close(
        o.double(), ref[:, rank * Sl : (rank + 1) * Sl], atol=1e-5, rtol=1e-5)
    # gradient flows through both a2a directions
    o.sum().backward()
    assert q.grad is not None and q.grad.abs().sum() > 0
    assert k.grad is not None and v.grad is not None
    dist.barrier()
    dist.destroy_process_group()
    return True


def test_ulysses_a2a_and_attention():
    assert all(run_distributed(_a2a_worker, 2, timeout=120))


def test_ulysses_a2a_world4():
    # SP degree 4 (the intellect10b_sp4_32k.toml shape, tiny dims)
    assert all(run_distributed(_a2a_worker, 4, timeout=180))


def _sp_trainer(rank, world, sp, steps):
    from prime_amd.train import Trainer
    from prime_amd.utils.config import (
        DilocoConfig, MetricsConfig, ModelConfig, ParallelConfig, TrainConfig,
    )

    # SP run: 2 ranks x seq 32 = one 64-token context.
    # Reference run (sp=False, world=1): seq 64 directly.
    cfg = TrainConfig(
        run_name=f"sp_{sp}",
        steps=steps,
        model=ModelConfig(name="llama_test", seq_len=32 if sp else 64),
        diloco=DilocoConfig(H=10**6),
        parallel=ParallelConfig(worker_size=world if sp else 1,
                                seq_parallel=sp),
        metrics=MetricsConfig(log_interval=100),
    )
    cfg.data.micro_batch_size = 2
    tr = Trainer(cfg, run_dir=f"{SCRATCH}/sp{sp}_r{rank}")
    losses = []
    for _ in range(steps):
        loss = tr.train_step()
        # SP: each rank's loss covers its token slice; average for the
        # full-context loss
        if sp:
            import torch.distributed as dist

            t = loss.detach().clone()
            dist.all_reduce(t)
            losses.append(float(t) / world)
        else:
            losses.append(float(loss))
    w = {n: p.detach().sum().item() for n, p in tr.model.named_parameters()}
    tr.close()
    return {"losses": losses, "w": w}


def test_sp_trainer_matches_full_context():
    sp = run_distributed(_sp_trainer, 2, args=(True, 3), timeout=300)
    ref = run_distributed(_sp_trainer, 1, args=(False, 3), timeout=300)
    for a, b in zip(sp[0]["losses"], ref[0]["losses"]):
        assert abs(a - b) < 1e-3, (sp[0]["losses"], ref[0]["losses"])
    for kk in ref[0]["w"]:
        assert abs(sp[0]["w"][kk] - ref[0]["w"][kk]) < 2e-2, kk
    # both SP ranks hold identical replicated params
    assert sp[0]["w"] == sp[1]["w"]


def _sp_diloco_trainer(rank, world, sp, steps):
    """SP composed with DiLoCo: (sp=True) 2 workers x SP(2) over seq 32
    slices vs (sp=False) 2 full-context workers at seq 64 — same data
    per worker, H=2 outer syncs included; losses and final params must
    match the full-context run."""
    from prime_amd.train import Trainer
    from prime_amd.utils.config import (
        DilocoConfig, MetricsConfig, ModelConfig, ParallelConfig, TrainConfig,
    )

    ws = 2 if sp else 1
    cfg = TrainConfig(
        run_name=f"spdiloco_{sp}",
        steps=steps,
        model=ModelConfig(name="llama_test", seq_len=32 if sp else 64),
        diloco=DilocoConfig(H=2),
        parallel=ParallelConfig(worker_size=ws, seq_parallel=sp),
        metrics=MetricsConfig(log_interval=100),
    )
    cfg.data.micro_batch_size = 2
    tr = Trainer(cfg, run_dir=f"{SCRATCH}/spd{sp}_r{rank}")
    losses = []
    for _ in range(steps):
        loss = tr.train_step()
        if sp:
            import torch.distributed as dist

            t = loss.detach().clone()
            dist.all_reduce(t, group=tr.mesh.local_group)
            losses.append(float(t) / ws)
        else:
            losses.append(float(loss))
    w = {n: p.detach().sum().item() for n, p in tr.model.named_parameters()}
    outer = tr.diloco.outer_step_count
    tr.close()
    return {"losses": losses, "w": w, "outer": outer}


def test_sp_composes_with_diloco():
    sp = run_distributed(_sp_diloco_trainer, 4, args=(True, 4), timeout=300)
    ref = run_distributed(_sp_diloco_trainer, 2, args=(False, 4), timeout=300)
    assert sp[0]["outer"] == ref[0]["outer"] == 2  # H=2, 4 steps
    # worker 0 of the SP run = ranks 0,1; its loss must track ref worker 0
    for a, b in zip(sp[0]["losses"], ref[0]["losses"]):
        assert abs(a - b) < 1e-3, (sp[0]["losses"], ref[0]["losses"])
    for kk in ref[0]["w"]:
        assert abs(sp[0]["w"][kk] - ref[0]["w"][kk]) < 2e-2, kk
    # SP ranks of one worker hold identical replicated params
    assert sp[0]["w"] == sp[1]["w"]
