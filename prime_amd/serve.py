"""Local OpenAI-style inference server — the engine-side counterpart of
the reference's hosted inference surface (prime_cli api/inference.py:
list models + chat completion against api.pinference.ai; here the
models run on the local MI355X through the hipGraph decode path).

Endpoints: GET /health, GET /v1/models, POST /v1/completions,
POST /v1/chat/completions. Prompts are either text (requires a local
tokenizer.json) or raw token-id lists. Requests go into a queue; one
worker thread takes the first waiting request, collects more for up to
`batch_window_ms` (or until it holds `max_batch`), and runs them as ONE
ragged generate_batch call, so requests of different lengths share every
decode step. Only that thread touches the model (the decode sessions
cache their hipGraph per (batch, length-bucket); concurrent capture would
race). Admission is per batch: a request that arrives while a batch is
decoding waits for the next one.
"""
from __future__ import annotations

import queue
import threading
import time
import uuid
from concurrent.futures import Future
from typing import Optional, Union

import torch
from pydantic import BaseModel


class CompletionRequest(BaseModel):
    model: Optional[str] = None
    prompt: Union[str, list[int]]
    max_tokens: int = 64
    temperature: float = 0.0
    top_k: int = 0
    seed: Optional[int] = None
    stop_token_ids: Optional[list[int]] = None


class ChatMessage(BaseModel):
    role: str
    content: str


class ChatRequest(BaseModel):
    model: Optional[str] = None
    messages: list[ChatMessage]
    max_tokens: int = 64
    temperature: float = 0.0
    top_k: int = 0
    seed: Optional[int] = None
    stop_token_ids: Optional[list[int]] = None


def create_app(model, model_name: str, tokenizer=None, max_batch: int = 8,
               batch_window_ms: float = 5.0, kv_dtype: str = "bf16"):
    from fastapi import FastAPI, HTTPException

    from .models import generate as gen_mod

    if max_batch < 1:
        raise ValueError("max_batch must be >= 1")
    if kv_dtype not in gen_mod.KV_DTYPES:
        raise ValueError(f"kv_dtype must be one of {gen_mod.KV_DTYPES} (got "
                         f"{kv_dtype!r})")
    app = FastAPI(title="prime-amd inference")
    dev = next(model.parameters()).device
    pending: queue.Queue = queue.Queue()
    worker_lock = threading.Lock()
    worker: list = []  # the one model thread, started by the first request

    def _serve_batch(batch) -> None:
        """Run one generate_batch for `batch` [(ids, req, future)]. Requests
        that stop on different token sets cannot share a call's single stop
        set, so the batch is grouped by it (usually one group)."""
        groups: dict = {}
        for item in batch:
            stop = tuple(sorted(set(item[1].stop_token_ids or ())))
            groups.setdefault(stop, []).append(item)
        for stop, items in groups.items():
            try:
                outs = gen_mod.generate_batch(
                    model, [ids for ids, _, _ in items],
                    [r.max_tokens for _, r, _ in items],
                    temperature=[r.temperature for _, r, _ in items],
                    top_k=[r.top_k for _, r, _ in items],
                    seed=[r.seed for _, r, _ in items],
                    stop_token_ids=list(stop), kv_dtype=kv_dtype)
                for (_, _, fut), new in zip(items, outs):
                    fut.set_result(new)
            except Exception as e:  # noqa: BLE001 - reported to every caller
                for _, _, fut in items:
                    fut.set_exception(e)

    def _worker_loop() -> None:
        while True:
            batch = [pending.get()]
            deadline = time.monotonic() + batch_window_ms / 1e3
            while len(batch) < max_batch:
                left = deadline - time.monotonic()
                if left <= 0:
                    break
                try:
                    batch.append(pending.get(timeout=left))
                except queue.Empty:
                    break
            try:
                _serve_batch(batch)
            except BaseException as e:  # noqa: BLE001 - the worker must live
                for _, _, fut in batch:
                    if not fut.done():
                        fut.set_exception(e)

    def _submit(ids: list[int], req) -> Future:
        with worker_lock:
            if not worker:
                t = threading.Thread(target=_worker_loop, daemon=True,
                                     name="prime-amd-serve")
                t.start()
                worker.append(t)
        fut: Future = Future()
        pending.put((ids, req, fut))
        return fut

    def _encode(prompt: Union[str, list[int]]) -> list[int]:
        if isinstance(prompt, str):
            if tokenizer is None:
                raise HTTPException(
                    400, "text prompts need --tokenizer; send token ids")
            from .utils.tokenizer import encode

            return encode(tokenizer, prompt)
        return [int(t) for t in prompt]

    def _decode(ids: list[int]) -> Union[str, list[int]]:
        if tokenizer is None:
            return ids
        from .utils.tokenizer import decode

        return decode(tokenizer, ids)

    def _run(ids: list[int], req) -> dict:
        if not ids:
            raise HTTPException(400, "empty prompt")
        if not 1 <= req.max_tokens <= 8192:
            raise HTTPException(400, "max_tokens must be in [1, 8192]")
        if not all(0 <= t < model.cfg.vocab_size for t in ids):
            raise HTTPException(400, "token id outside the vocabulary")
        if len(ids) + req.max_tokens > model.cfg.max_seq:
            # checked here so one oversize request cannot fail its batch
            raise HTTPException(
                400, f"prompt + max_tokens exceeds max_seq {model.cfg.max_seq}")
        t0 = time.perf_counter()
        try:
            new = _submit(ids, req).result()
        except Exception as e:  # noqa: BLE001
            raise HTTPException(500, f"generation failed: {e}") from e
        dt = time.perf_counter() - t0
        stopped = bool(new) and new[-1] in set(req.stop_token_ids or ())
        return {
            "text": _decode(new),
            "prompt_tokens": len(ids),
            "completion_tokens": len(new),
            "elapsed_s": dt,
            "finish_reason": "stop" if stopped else "length",
        }

    @app.get("/health")
    def health():
        return {"status": "ok", "model": model_name, "device": str(dev),
                "kv_dtype": kv_dtype}

    @app.get("/v1/models")
    def models():
        from .models import CONFIGS

        return {"object": "list", "data": [
            {"id": model_name, "object": "model", "owned_by": "prime-amd",
             "loaded": True},
            *({"id": n, "object": "model", "owned_by": "prime-amd",
               "loaded": False} for n in CONFIGS if n != model_name),
        ]}

    @app.post("/v1/completions")
    def completions(req: CompletionRequest):
        r = _run(_encode(req.prompt), req)
        return {
            "id": f"cmpl-{uuid.uuid4().hex[:12]}",
            "object": "text_completion",
            "created": int(time.time()),
            "model": model_name,
            "choices": [{"index": 0, "text": r["text"],
                         "finish_reason": r["finish_reason"]}],
            "usage": {"prompt_tokens": r["prompt_tokens"],
                      "completion_tokens": r["completion_tokens"],
                      "total_tokens": r["prompt_tokens"] + r["completion_tokens"]},
        }

    @app.post("/v1/chat/completions")
    def chat(req: ChatRequest):
        if tokenizer is None:
            raise HTTPException(400, "chat needs --tokenizer (text prompts)")
        prompt = "".join(f"<|{m.role}|>\n{m.content}\n" for m in req.messages)
        prompt += "<|assistant|>\n"
        creq = CompletionRequest(prompt=prompt, max_tokens=req.max_tokens,
                                 temperature=req.temperature, top_k=req.top_k,
                                 seed=req.seed,
                                 stop_token_ids=req.stop_token_ids)
        r = _run(_encode(prompt), creq)
        return {
            "id": f"chatcmpl-{uuid.uuid4().hex[:12]}",
            "object": "chat.completion",
            "created": int(time.time()),
            "model": model_name,
            "choices": [{"index": 0, "finish_reason": r["finish_reason"],
                         "message": {"role": "assistant", "content": r["text"]}}],
            "usage": {"prompt_tokens": r["prompt_tokens"],
                      "completion_tokens": r["completion_tokens"],
                      "total_tokens": r["prompt_tokens"] + r["completion_tokens"]},
        }

    return app


def load_model_for_serving(model_name: str, checkpoint: str | None = None,
                           device: str | None = None):
    """Build (and optionally warm-start) a model for the server."""
    from .models import build_model

    dev = device or ("cuda" if torch.cuda.is_available() else "cpu")
    m = build_model(model_name)
    if dev == "cuda":
        m = m.to(dev, dtype=torch.bfloat16)
    m.reset_rope(torch.device(dev))
    if checkpoint:
        from .ckpt import CheckpointManager
        from .parallel.flat import FlatParamSpace

        flat = FlatParamSpace(m)
        payload = CheckpointManager(checkpoint).load(map_location=dev)
        if payload is None:
            raise FileNotFoundError(f"no checkpoint under {checkpoint}")
        flat.load_flat_(payload["tensors"]["master32"].to(dev))
    m.eval()
    return m
