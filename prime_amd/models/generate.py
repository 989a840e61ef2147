"""KV-cache generation (serving path): causal-flash prefill + the
memory-bound decode kernel per new token.

Prompts are right-padded to a multiple of 64 for the prefill kernel
(pad keys sit at positions AFTER every real query, so causal masking
keeps them out of real rows); the caches are then truncated to the true
prompt length before decoding.

generate() decodes a rectangular batch (one position for all sequences);
generate_batch() decodes prompts of different lengths together through
the ragged decode kernels, each sequence at its own position.
"""
from __future__ import annotations

import torch

from .. import ops
from .llama import Llama

KV_DTYPES = ("bf16", "fp8")


def _pad64(n: int) -> int:
    return (n + 63) // 64 * 64


@torch.no_grad()
def generate(
    model: Llama,
    tokens: torch.Tensor,
    max_new_tokens: int,
    temperature: float = 0.0,
    top_k: int = 0,
    seed: int | None = None,
    use_graph: bool = True,
) -> torch.Tensor:
    """tokens [B, L0] -> [B, L0 + max_new_tokens] (greedy when
    temperature == 0). With use_graph on CUDA, the per-token decode pass
    runs as a cached hipGraph replay (capture amortizes across calls of
    the same (batch, length-bucket))."""
    model.eval()
    cfg = model.cfg
    dev = tokens.device
    dtype = next(model.parameters()).dtype
    B, L0 = tokens.shape
    total = L0 + max_new_tokens
    if total > cfg.max_seq:
        raise ValueError(f"{total} tokens exceeds max_seq {cfg.max_seq}")
    graphing = use_graph and tokens.is_cuda and max_new_tokens > 2
    # bucket the cache length so repeat calls reuse the captured graph
    smax = min(_pad64(cfg.max_seq), _pad64(max(total, 1024))) if graphing \
        else _pad64(total)
    sessions = getattr(model, "_decode_sessions", None)
    if sessions is None:
        sessions = model._decode_sessions = {}
    key = (B, smax, dev.index)
    sess = None
    if graphing and key in sessions:
        sess = sessions[key]
        caches = sess["caches"]
    else:
        caches = [
            (
                torch.zeros(B, smax, cfg.n_kv_heads, cfg.head_dim, device=dev, dtype=dtype),
                torch.zeros(B, smax, cfg.n_kv_heads, cfg.head_dim, device=dev, dtype=dtype),
            )
            for _ in range(cfg.n_layers)
        ]
        if graphing:
            # capture BEFORE prefill: the warmup/capture passes write junk
            # rows into the cache, which the prefill then overwrites
            sess = sessions[key] = _build_session(model, caches, B, dev)
    gen = torch.Generator(device="cpu")
    if seed is not None:
        gen.manual_seed(seed)

    # ---- prefill (padded to 64; pad keys are causally invisible)
    Lp = _pad64(L0)
    padded = torch.zeros(B, Lp, dtype=tokens.dtype, device=dev)
    padded[:, :L0] = tokens
    h = model(padded, caches=caches, pos=0)  # caches filled for [0, Lp)
    logits = model.lm_head(h[:, L0 - 1])

    out = [tokens]
    cur = _sample(logits, temperature, top_k, gen)
    out.append(cur)
    pos = L0
    if sess is not None and max_new_tokens > 1:
        rest = _decode_graphed(sess, cur, pos, max_new_tokens - 1,
                               temperature, top_k, gen)
        out.extend(rest)
    else:
        for _ in range(max_new_tokens - 1):
            h = model(cur, caches=caches, pos=pos)
            logits = model.lm_head(h[:, 0])
            cur = _sample(logits, temperature, top_k, gen)
            out.append(cur)
            pos += 1
    return torch.cat(out, dim=1)


def _build_session(model, caches, B, dev):
    """Capture the per-token decode pass (embed -> n_layers x {norms, qkv
    GEMM, rope, cache write, decode attention, o/mlp GEMMs} -> lm_head) as
    ONE replayable hipGraph. Dynamic state (position, cache length) lives
    in device scalars the kernels read at run time; the graph itself
    increments them. Capture cost amortizes across generate() calls."""
    pos_dev = {
        "pos32": torch.zeros((), dtype=torch.int32, device=dev),
        "pos64": torch.zeros(1, dtype=torch.int64, device=dev),
        "len32": torch.ones((), dtype=torch.int32, device=dev),
    }
    static_tok = torch.zeros(B, 1, dtype=torch.int64, device=dev)

    def step():
        h = model(static_tok, caches=caches, pos=0, pos_dev=pos_dev)
        logits = model.lm_head(h[:, 0])
        pos_dev["pos32"].add_(1)
        pos_dev["pos64"].add_(1)
        pos_dev["len32"].add_(1)
        return logits

    # warmup on a side stream (per torch CUDA-graphs contract)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_logits = step()
    return {"caches": caches, "graph": graph, "pos_dev": pos_dev,
            "static_tok": static_tok, "static_logits": static_logits}


def _decode_graphed(sess, first_tok, pos0, n_tokens, temperature, top_k, gen):
    pos_dev = sess["pos_dev"]
    pos_dev["pos32"].fill_(pos0)
    pos_dev["pos64"].fill_(pos0)
    pos_dev["len32"].fill_(pos0 + 1)
    sess["static_tok"].copy_(first_tok)
    graph, static_logits = sess["graph"], sess["static_logits"]
    out = []
    for _ in range(n_tokens):
        graph.replay()
        if temperature <= 0:
            nxt = static_logits.argmax(-1, keepdim=True)  # stays on device
        else:
            nxt = _sample(static_logits, temperature, top_k, gen)
        out.append(nxt)
        sess["static_tok"].copy_(nxt)
    return out


def _per_seq(value, n: int, name: str) -> list:
    """A scalar option broadcast to n sequences, or one value per sequence."""
    if isinstance(value, (list, tuple)):
        if len(value) != n:
            raise ValueError(f"{name}: got {len(value)} values for {n} prompts")
        return list(value)
    return [value] * n


def _bucket(n: int) -> int:
    b = 1
    while b < n:
        b *= 2
    return b


@torch.no_grad()
def generate_batch(
    model: Llama,
    prompts,
    max_new_tokens,
    temperature=0.0,
    top_k=0,
    seed=None,
    stop_token_ids=None,
    use_graph: bool = True,
    kv_dtype: str = "bf16",
) -> list[list[int]]:
    """Ragged batched generation: `prompts` is a list of token-id lists of
    different lengths; returns the NEW tokens of each. max_new_tokens,
    temperature, top_k and seed take a scalar or one value per sequence. A
    sequence ends after its own max_new_tokens or on one of stop_token_ids
    (the stop token is kept); finished sequences become idle slots of the
    decode kernels and cause no further KV traffic. Each sequence samples
    from its own CPU generator, so a seeded request gives the same tokens
    alone or next to others.

    One batched causal-flash prefill (right-padded; rows past a prompt's
    length hold junk that is never read: every decode step writes row
    pos[b] before attending to pos[b] + 1 rows), then one ragged decode pass
    per token. The batch is padded with idle slots to a power of two; with
    use_graph on CUDA the per-token pass is a hipGraph captured once per
    (batch bucket, cache-length bucket, device, kv_dtype) that advances its
    own device-side positions.

    kv_dtype "bf16" keeps the cache in the model's dtype; "fp8" stores it as
    e4m3 bytes with one fp32 scale per (row, kv head) (ops.KVCacheFp8): half
    the memory and traffic. The prefill attends to the unquantised k and v,
    so the first new token is that of the bf16 cache; later tokens see the
    quantised rows."""
    if kv_dtype not in KV_DTYPES:
        raise ValueError(f"kv_dtype must be one of {KV_DTYPES} (got "
                         f"{kv_dtype!r})")
    model.eval()
    cfg = model.cfg
    p0 = next(model.parameters())
    dev, dtype = p0.device, p0.dtype
    n = len(prompts)
    if n == 0:
        return []
    prompts = [[int(t) for t in p] for p in prompts]
    max_new = [int(m) for m in _per_seq(max_new_tokens, n, "max_new_tokens")]
    temps = _per_seq(temperature, n, "temperature")
    topks = _per_seq(top_k, n, "top_k")
    seeds = _per_seq(seed, n, "seed")
    stops = frozenset(int(t) for t in (stop_token_ids or ()))
    L0 = [len(p) for p in prompts]
    for b in range(n):
        if L0[b] == 0:
            raise ValueError(f"prompt {b} is empty")
        if L0[b] + max_new[b] > cfg.max_seq:
            raise ValueError(f"prompt {b}: {L0[b] + max_new[b]} tokens exceeds "
                             f"max_seq {cfg.max_seq}")
    out: list[list[int]] = [[] for _ in range(n)]
    done = [m <= 0 for m in max_new]
    if all(done):
        return out
    total = max(L0[b] + max(max_new[b], 1) for b in range(n))
    Bk = _bucket(n)
    on_gpu = dev.type == "cuda"
    graphing = use_graph and on_gpu and max(max_new) > 2
    # cache-length bucket: shared by the graphed and the eager pass, so both
    # launch the same kernels on the same shapes and agree exactly
    smax = min(_pad64(cfg.max_seq), _pad64(max(total, 1024))) if on_gpu \
        else _pad64(total)
    sessions = getattr(model, "_decode_sessions", None)
    if sessions is None:
        sessions = model._decode_sessions = {}
    key = ("ragged", Bk, smax, dev.index, kv_dtype)
    sess = sessions.get(key) if graphing else None
    if sess is None:
        if kv_dtype == "fp8":
            caches = [ops.kv_cache_fp8(Bk, smax, cfg.n_kv_heads, cfg.head_dim, dev)
                      for _ in range(cfg.n_layers)]
        else:
            caches = [
                (
                    torch.zeros(Bk, smax, cfg.n_kv_heads, cfg.head_dim, device=dev, dtype=dtype),
                    torch.zeros(Bk, smax, cfg.n_kv_heads, cfg.head_dim, device=dev, dtype=dtype),
                )
                for _ in range(cfg.n_layers)
            ]
        sess = _ragged_state(caches, Bk, dev)
        if graphing:
            # capture BEFORE prefill, as _build_session does: the warmup and
            # capture passes write junk rows that the prefill overwrites
            _capture_ragged(model, sess)
            sessions[key] = sess
    caches = sess["caches"]
    gens = []
    for b in range(n):
        g = torch.Generator(device="cpu")
        if seeds[b] is not None:
            g.manual_seed(int(seeds[b]))
        gens.append(g)

    def pick(logits, rows):
        """Next token of every sequence in `rows` (logits row = slot)."""
        greedy = None
        nxt = {}
        for b in rows:
            if temps[b] <= 0:
                if greedy is None:  # one device sync for all greedy rows
                    greedy = logits.argmax(-1).tolist()
                nxt[b] = int(greedy[b])
            else:
                nxt[b] = int(_sample(logits[b:b + 1], temps[b], topks[b], gens[b]))
        return nxt

    def accept(nxt):
        for b, t in nxt.items():
            out[b].append(t)
            if len(out[b]) >= max_new[b] or t in stops:
                done[b] = True

    # ---- prefill the real sequences (views of the first n cache slots)
    Lp = _pad64(max(L0))
    padded = torch.zeros(n, Lp, dtype=torch.int64)
    for b in range(n):
        padded[b, :L0[b]] = torch.tensor(prompts[b], dtype=torch.int64)
    padded = padded.to(dev)
    pre = [ops.KVCacheFp8(*(t[:n] for t in c)) if isinstance(c, ops.KVCacheFp8)
           else (c[0][:n], c[1][:n]) for c in caches]
    h = model(padded, caches=pre, pos=0)
    last = torch.tensor([l - 1 for l in L0], device=dev)
    logits = model.lm_head(h[torch.arange(n, device=dev), last])
    live = [b for b in range(n) if not done[b]]
    accept(pick(logits, live))

    # ---- ragged decode: slot b sits at pos[b]; finished / padding = idle
    def write_state():
        pos = [-1] * Bk
        for b in range(n):
            if not done[b]:
                pos[b] = L0[b] + len(out[b]) - 1
        pos_t = torch.tensor(pos, dtype=torch.int32)
        act_t = (pos_t >= 0).to(torch.int32)
        sess["pos"].copy_(pos_t)
        sess["active"].copy_(act_t)
        sess["lens"].copy_((pos_t + 1) * act_t)

    write_state()
    tok = torch.zeros(Bk, 1, dtype=torch.int64)
    while not all(done):
        live = [b for b in range(n) if not done[b]]
        for b in live:
            tok[b, 0] = out[b][-1]
        sess["tok"].copy_(tok)
        if graphing:
            sess["graph"].replay()
            logits = sess["logits"]
        else:
            logits = _ragged_step(model, sess)
        accept(pick(logits, live))
        if any(done[b] for b in live):
            write_state()  # retire finished sequences to idle slots
    return out


def _ragged_state(caches, Bk, dev):
    """Device-side state of a ragged decode pass (stable pointers for graph
    replay). Initial values are a safe warm-up state: every slot at row 0."""
    return {
        "caches": caches,
        "tok": torch.zeros(Bk, 1, dtype=torch.int64, device=dev),
        "pos": torch.zeros(Bk, dtype=torch.int32, device=dev),
        "lens": torch.ones(Bk, dtype=torch.int32, device=dev),
        "active": torch.ones(Bk, dtype=torch.int32, device=dev),
    }


def _ragged_step(model, sess):
    """One token for every live slot, then advance the device-side state:
    pos += active, lens = (pos + 1) * active (idle slots stay idle)."""
    h = model(sess["tok"], caches=sess["caches"], seq_pos=sess)
    logits = model.lm_head(h[:, 0])
    sess["pos"].add_(sess["active"])
    torch.mul(sess["pos"] + 1, sess["active"], out=sess["lens"])
    return logits


def _capture_ragged(model, sess):
    """Capture _ragged_step as one replayable hipGraph (warm-up on a side
    stream, per the torch CUDA-graphs contract, as _build_session)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            _ragged_step(model, sess)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sess["logits"] = _ragged_step(model, sess)
    sess["graph"] = graph


def _sample(logits: torch.Tensor, temperature: float, top_k: int, gen) -> torch.Tensor:
    if temperature <= 0:
        return logits.argmax(-1, keepdim=True)
    logits = logits.float() / temperature
    if top_k > 0:
        kth = logits.topk(top_k, dim=-1).values[..., -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    probs = logits.softmax(-1)
    idx = torch.multinomial(probs.cpu(), 1, generator=gen).to(logits.device)
    return idx
