"""Flat parameter space: the substrate for the fused optimizer, DiLoCo outer
state, int8 ring all-reduce, and checkpointing.

All trainable parameters are re-homed into ONE contiguous buffer per dtype
(param offsets 64-element aligned so every bf16x8 kernel load stays 16 B
aligned). Consequences, all MI355X-deliberate:
  - inner AdamW is ONE kernel launch over the whole model (10B params =
    one 120 GB-traffic pass at HBM speed, no per-tensor launch overhead),
  - the DP gradient all-reduce and the outer pseudo-gradient ring operate
    on single contiguous buffers (bigger, fewer collectives — xGMI-friendly),
  - checkpoint/live-recovery serialize one tensor per state kind.
"""
from __future__ import annotations

import weakref
from typing import Iterator

import torch
import torch.nn as nn

from .. import ops

ALIGN = 64


class FlatParamSpace:
    """Flattens a module's trainable params; owns optimizer + outer state."""

    def __init__(self, module: nn.Module):
        self.module = module
        self.params: list[tuple[str, nn.Parameter]] = [
            (n, p) for n, p in module.named_parameters() if p.requires_grad
        ]
        if not self.params:
            raise ValueError("module has no trainable parameters")
        # tied params (e.g. lm_head.weight is tok_embeddings.weight) must be
        # flattened once
        seen: dict[int, str] = {}
        uniq = []
        for n, p in self.params:
            if id(p) in seen:
                continue
            seen[id(p)] = n
            uniq.append((n, p))
        self.params = uniq

        dev = self.params[0][1].device
        dt = self.params[0][1].dtype
        self.device, self.dtype = dev, dt

        self.offsets: dict[str, tuple[int, int, torch.Size]] = {}
        off = 0
        for n, p in self.params:
            numel = p.numel()
            self.offsets[n] = (off, numel, p.shape)
            off += (numel + ALIGN - 1) // ALIGN * ALIGN
        self.numel_padded = off

        self.flat_w = torch.zeros(off, device=dev, dtype=dt)
        self.flat_grad = torch.zeros(off, device=dev, dtype=dt)
        for n, p in self.params:
            o, k, shp = self.offsets[n]
            self.flat_w[o : o + k].copy_(p.detach().flatten())
            p.data = self.flat_w[o : o + k].view(shp)
            p.grad = self.flat_grad[o : o + k].view(shp)
        self.master32 = self.flat_w.float()
        self._sq = None
        self._register_direct_wgrad()

    # ------------------------------------------------------ direct wgrad
    def _register_direct_wgrad(self) -> None:
        """Untied 2-D PrimeLinear weights get their dW written by the GEMM
        straight into flat_grad (ops.functional, 'Direct wgrad'), so their
        ranges need neither the per-step zero fill nor autograd's
        `grad += dW`. direct_ranges / zero_ranges partition
        [0, numel_padded): zero_grad() fills only the latter."""
        from ..models.llama import PrimeLinear

        uses: dict[int, int] = {}
        for _, p in self.module.named_parameters(remove_duplicate=False):
            uses[id(p)] = uses.get(id(p), 0) + 1
        name_of = {id(p): n for n, p in self.params}
        direct: list[tuple[int, int, str]] = []
        for m in self.module.modules():
            if not isinstance(m, PrimeLinear) or m.bias is not None:
                continue
            p = m.weight
            n = name_of.get(id(p))
            if n is None or p.dim() != 2 or uses[id(p)] != 1:
                continue  # frozen or tied (shared with another module)
            o, k, _ = self.offsets[n]
            direct.append((o, o + k, n))
        direct.sort()
        self.direct_ranges = [(a, b) for a, b, _ in direct]
        self.zero_ranges: list[tuple[int, int]] = []
        cur = 0
        for a, b in self.direct_ranges:
            if a > cur:
                self.zero_ranges.append((cur, a))
            cur = b
        if cur < self.numel_padded:
            self.zero_ranges.append((cur, self.numel_padded))
        self._slots = []
        self._direct_step = False
        if self.device.type != "cuda":
            return  # CPU linears never reach the dW GEMM hook
        self._owner = weakref.ref(self)
        params = dict(self.params)
        for a, b, n in direct:
            p = params[n]
            self._slots.append(ops.functional.register_wgrad_slot(
                p, self.flat_grad[a:b].view(p.shape), self._owner))
        weakref.finalize(self, ops.functional.unregister_wgrad_slots,
                         self._owner)

    def zero_grad(self) -> None:
        """Start a step. With direct wgrad on, registered weight ranges are
        left alone (their first dW of the step overwrites them); call
        finalize_grads() before reading flat_grad."""
        if not (self._slots and ops.direct_wgrad_enabled()):
            for s in self._slots:
                s[1] = s[3] = False
            self._direct_step = False
            self.flat_grad.zero_()
            return
        for a, b in self.zero_ranges:
            self.flat_grad[a:b].zero_()
        for s in self._slots:
            if s[3]:  # a forward already routed this dW through autograd
                s[0].zero_()
                s[1] = s[3] = False
            else:
                s[1] = True
        self._direct_step = True

    def finalize_grads(self) -> None:
        """Before flat_grad is consumed: a registered weight that received
        no gradient this step still holds last step's values — zero it."""
        if not self._direct_step:
            return
        for s in self._slots:
            if s[1]:
                s[0].zero_()
                s[1] = False
        self._direct_step = False

    def grad_views(self) -> Iterator[torch.Tensor]:
        self.finalize_grads()
        for n, _ in self.params:
            o, k, shp = self.offsets[n]
            yield self.flat_grad[o : o + k].view(shp)

    def clip_grad_norm_(self, max_norm: float) -> torch.Tensor:
        """Global-norm clip on the flat grad (single fused pass)."""
        self.finalize_grads()
        norm = self.flat_grad.float().norm(2)
        scale = (max_norm / (norm + 1e-6)).clamp(max=1.0)
        self.flat_grad.mul_(scale.to(self.flat_grad.dtype))
        return norm

    def grad_clip_scale(self, max_norm: float) -> torch.Tensor:
        """Deferred clip (GPU): returns the 1-element scale tensor
        min(1, max_norm/||g||) consumed by the fused AdamW kernel — the
        flat grad is never rewritten (saves a 2x21 GB pass at 10B)."""
        if self._sq is None:
            self._sq = torch.zeros(1, device=self.device, dtype=torch.float32)
        self._sq.zero_()
        self.finalize_grads()
        ops.grad_sqnorm(self.flat_grad, self._sq)
        return (max_norm / (self._sq.sqrt() + 1e-6)).clamp(max=1.0)

    def state_dict(self) -> dict:
        return {"flat_w": self.flat_w, "master32": self.master32}

    def load_flat_(self, master32: torch.Tensor) -> None:
        self.master32.copy_(master32)
        self.flat_w.copy_(self.master32.to(self.dtype))
        ops.invalidate_wt_cache()


class FusedAdamW:
    """AdamW over a FlatParamSpace: fp32 master + m/v, bf16 model params.

    On CUDA: one hand-written HIP kernel pass (prime_adamw). On CPU: the
    fp32 reference math (plumbing config)."""

    def __init__(self, flat: FlatParamSpace, lr=3e-4, betas=(0.9, 0.95),
                 eps=1e-8, weight_decay=0.1):
        self.flat = flat
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.m = torch.zeros_like(flat.master32)
        self.v = torch.zeros_like(flat.master32)
        self.step_count = 0

    def step(self, gscale=None) -> None:
        self.step_count += 1
        ops.invalidate_wt_cache()  # in-place weight update (raw kernel)
        f = self.flat
        if f.device.type == "cuda":
            ops.fused_adamw(
                f.master32, f.flat_w, f.flat_grad, self.m, self.v,
                lr=self.lr, beta1=self.betas[0], beta2=self.betas[1],
                eps=self.eps, wd=self.wd, step=self.step_count,
                gscale=gscale,
            )
        else:
            ops.reference.adamw_step(
                f.master32, f.flat_grad, self.m, self.v, self.lr,
                self.betas[0], self.betas[1], self.eps, self.wd,
                self.step_count,
            )
            f.flat_w.copy_(f.master32.to(f.dtype))

    def zero_grad(self) -> None:
        self.flat.zero_grad()

    def state_dict(self) -> dict:
        return {"m": self.m, "v": self.v, "step": self.step_count,
                "lr": self.lr, "betas": self.betas, "eps": self.eps, "wd": self.wd}

    def load_state_dict(self, sd: dict) -> None:
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])
        self.step_count = int(sd["step"])
