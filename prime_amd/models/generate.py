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
KV_LAYOUTS = ("contiguous", "paged")
WEIGHT_DTYPES = ("bf16", "fp8")


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
    lookahead: int = 0,
    prefill_chunk: int = 0,
    kv_layout: str = "contiguous",
    page_size: int = 64,
    kv_pages: int | None = None,
    weight_dtype: str = "bf16",
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
    quantised rows.

    lookahead = K > 0 (at most 7, either cache type) turns on prompt-lookup drafting
    for the greedy sequences: the draft is the K tokens that followed the
    most recent earlier occurrence of the sequence's last two tokens, and one
    multi-token decode step (T = K + 1 rows per sequence) verifies it,
    keeping the longest prefix the model agrees with plus one corrected
    token. Rejected rows are overwritten by the next step. Sampling
    sequences take one token per step in the same batch. The host writes
    the step's tokens, positions and row counts; the graph is captured once
    per (batch bucket, cache-length bucket, device, T, kv_dtype). With an fp8
    cache it needs a model on the GPU.

    prefill_chunk = C > 0 (a multiple of 8) replaces the padded flash
    prefill: the prompts enter the ragged cache in steps of C tokens, each
    sequence at its own position, through the chunked ragged prefill kernels
    (ops.prefill_qkv_append + ops.attn_prefill_ragged, or their _fp8 siblings
    with kv_dtype "fp8", which needs a model on the GPU). A short prompt costs
    its own length, not the longest one's. Runs eagerly. Over an fp8 cache a
    chunk attends to the QUANTISED rows, its own included, so the first new
    token is that of the quantised cache, not that of the bf16 cache as with
    the padded prefill.

    kv_layout "paged" (bf16 cache, no lookahead) stores the cache as a pool of
    kv_pages pages of page_size rows (64, 128 or 256) per layer plus one
    block table shared by the layers (ops.KVCachePaged). kv_pages defaults to
    the contiguous cache's capacity, Bk * smax / page_size. A host-side free
    list hands every sequence ceil((prompt + max_new) / page_size) pages at
    the start of the call and takes them back when it ends; a batch that
    needs more pages than the pool has raises ValueError before any work. A
    short prompt next to a long one then costs its own pages, not a slab of
    the longest length. The prompts always enter through the chunked ragged
    prefill (prefill_chunk, or 256 tokens a step); the decode graph reads the
    table from a stable device buffer, and its session key carries the
    layout, the page size and the pool size.

    weight_dtype "fp8" (a model on the GPU) reads every projection whose shape
    qualifies (Llama.quantize_decode_weights) as e4m3 bytes with one scale per
    output channel in the calls of at most 64 rows, the decode steps above
    all: half the weight traffic through ops.linear_w8. The fp8 copies are
    made once per model and kept on it until a weight changes; the bf16
    weights stay and serve the prefill and every larger call. The dtype is
    part of every session key; "bf16" leaves everything as it was."""
    lookahead = int(lookahead)
    prefill_chunk = int(prefill_chunk)
    if prefill_chunk < 0 or prefill_chunk % 8 != 0:
        raise ValueError(f"prefill_chunk must be 0 or a positive multiple of 8 "
                         f"(got {prefill_chunk})")
    if not 0 <= lookahead <= 7:
        raise ValueError(f"lookahead must be in 0..7 (got {lookahead})")
    if kv_dtype not in KV_DTYPES:
        raise ValueError(f"kv_dtype must be one of {KV_DTYPES} (got "
                         f"{kv_dtype!r})")
    if kv_layout not in KV_LAYOUTS:
        raise ValueError(f"kv_layout must be one of {KV_LAYOUTS} (got "
                         f"{kv_layout!r})")
    if weight_dtype not in WEIGHT_DTYPES:
        raise ValueError(f"weight_dtype must be one of {WEIGHT_DTYPES} (got "
                         f"{weight_dtype!r})")
    paged = kv_layout == "paged"
    if paged:
        if kv_dtype != "bf16" or lookahead:
            raise ValueError("kv_layout='paged' stores a bf16 cache and "
                             "decodes one token per step: it cannot be "
                             "combined with kv_dtype='fp8' or lookahead > 0")
        if page_size not in ops.KV_PAGE_SIZES:
            raise ValueError(f"page_size must be one of {ops.KV_PAGE_SIZES} "
                             f"(got {page_size})")
        if kv_pages is not None and int(kv_pages) < 1:
            raise ValueError(f"kv_pages must be positive (got {kv_pages})")
    model.eval()
    cfg = model.cfg
    p0 = next(model.parameters())
    dev, dtype = p0.device, p0.dtype
    if prefill_chunk and kv_dtype != "bf16" and dev.type != "cuda":
        raise ValueError("prefill_chunk with kv_dtype='fp8' needs a model on "
                         "the GPU: chunked prefill over an fp8 cache has no "
                         "host path")
    if weight_dtype == "fp8" and dev.type != "cuda":
        raise ValueError("weight_dtype='fp8' needs a model on the GPU: the "
                         "fp8 weight copies are read by a HIP kernel only")
    if lookahead and kv_dtype != "bf16" and dev.type != "cuda":
        # the model's guard (Attention.forward), raised before any work
        raise NotImplementedError("lookahead decoding over an fp8 KV cache "
                                  "runs on the GPU only")
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
    if paged:
        P = page_size
        smax = -(-smax // P) * P  # whole pages
        n_pool = int(kv_pages) if kv_pages is not None else Bk * smax // P
        need = [-(-(L0[b] + max(max_new[b], 0)) // P) for b in range(n)]
        if sum(need) > n_pool:
            raise ValueError(f"the batch needs {sum(need)} KV pages of "
                             f"{P} rows, the pool has {n_pool}")
    sessions = getattr(model, "_decode_sessions", None)
    if sessions is None:
        sessions = model._decode_sessions = {}
    key = ("ragged", Bk, smax, dev.index, weight_dtype, kv_dtype) \
        if not lookahead else ("ragged_multi", Bk, smax, dev.index,
                               lookahead + 1, weight_dtype, kv_dtype)
    if paged:
        key = ("ragged_paged", Bk, smax, dev.index, weight_dtype, P, n_pool)
    # with "fp8" the projections carry their fp8 copies for this call only, so
    # that a later "bf16" call finds the model as it was
    before = _attach_decode_weights(model, sessions) \
        if weight_dtype == "fp8" else []
    try:
        sess = sessions.get(key) if graphing else None
        if sess is None:
            if paged:
                # one table for all layers; its pointer is what the graph reads
                table = torch.full((Bk, smax // P), -1, dtype=torch.int32,
                                   device=dev)
                caches = [ops.KVCachePaged(
                    torch.zeros(n_pool, P, cfg.n_kv_heads, cfg.head_dim,
                                device=dev, dtype=dtype),
                    torch.zeros(n_pool, P, cfg.n_kv_heads, cfg.head_dim,
                                device=dev, dtype=dtype), table)
                    for _ in range(cfg.n_layers)]
            elif kv_dtype == "fp8":
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
            sess["weight_dtype"] = weight_dtype
            if paged:
                sess["pages"] = ops.KVPageAllocator(n_pool)
            if lookahead:
                sess["tok"] = torch.zeros(Bk, lookahead + 1, dtype=torch.int64,
                                          device=dev)
                sess["n_new"] = torch.ones(Bk, dtype=torch.int32, device=dev)
            if graphing:
                # capture BEFORE prefill, as _build_session does: the warmup and
                # capture passes write junk rows that the prefill overwrites
                _capture_ragged(model, sess, _multi_step if lookahead
                                else _ragged_step)
                sessions[key] = sess
        caches = sess["caches"]
        if paged:
            # the call's pages; handed back (and the table cleared) when it ends
            held = [sess["pages"].alloc(need[b]) for b in range(n)]
            rows = torch.full(tuple(caches[0].table.shape), -1, dtype=torch.int32)
            for b in range(n):
                rows[b, :need[b]] = torch.tensor(held[b], dtype=torch.int32)
            caches[0].table.copy_(rows)
            try:
                return _generate_ragged(model, sess, prompts, max_new, temps,
                                        topks, seeds, stops, out, done, graphing,
                                        0, prefill_chunk or 256)
            finally:
                for ids in held:
                    sess["pages"].free(ids)
                caches[0].table.fill_(-1)
        return _generate_ragged(model, sess, prompts, max_new, temps, topks, seeds,
                                stops, out, done, graphing, lookahead,
                                prefill_chunk)
    finally:
        for m, lw in before:
            if lw is None:
                m.__dict__.pop("w8", None)
            else:
                m.w8 = lw


def _attach_decode_weights(model, sessions) -> list:
    """Set the fp8 weight copies on the model's projections, quantising only
    when a weight has changed since the cached copies were made (keyed on the
    weights' storage and _version). Returns what the modules carried before,
    [(module, w8 or None)]."""
    mods = model._prime_linears()
    before = [(m, m.__dict__.get("w8")) for m in mods]
    wkey = tuple((m.weight.data_ptr(), m.weight._version) for m in mods)
    cached = getattr(model, "_decode_w8", None)
    if cached is not None and cached[0] == wkey:
        for m, lw in cached[1]:
            m.w8 = lw
        return before
    model.drop_decode_weights()
    model.quantize_decode_weights()
    model._decode_w8 = (wkey, [(m, m.w8) for m in mods if m.w8 is not None])
    # graphs captured over the previous copies would read freed memory
    for k in [k for k, v in sessions.items() if v.get("weight_dtype") == "fp8"]:
        del sessions[k]
    return before


def _generate_ragged(model, sess, prompts, max_new, temps, topks, seeds, stops,
                     out, done, graphing, lookahead, prefill_chunk):
    """Prefill and decode loop of generate_batch over the session's caches
    (any layout); fills `out` and returns it."""
    caches = sess["caches"]
    n, Bk = len(prompts), sess["pos"].shape[0]
    L0 = [len(p) for p in prompts]
    dev = sess["pos"].device
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

    if prefill_chunk:
        logits = model.lm_head(
            prefill_chunked(model, caches, prompts, prefill_chunk))
    else:
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

    if lookahead:
        _decode_lookahead(model, sess, graphing, lookahead, prompts, out, done,
                          max_new, stops, temps, topks, gens)
        return out

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


@torch.no_grad()
def prefill_chunked(model, caches, prompts, chunk: int) -> torch.Tensor:
    """Chunked ragged prefill: write `prompts` (token-id lists of different
    lengths) into the first len(prompts) slots of `caches` [(k, v) or an
    ops.KVCacheFp8 per layer, each k [Bk,Smax,Hkv,D]; or an ops.KVCachePaged
    per layer, whose table rows are the slots] in steps of `chunk`
    tokens and return the hidden state at each prompt's last token,
    [len(prompts), dim]. At every step slot b takes min(chunk, remaining_b)
    tokens at pos = done_b with lens = done_b + 1; finished and padding slots
    are idle (lens = 0, n_new = 0). Over fp8 caches (GPU only) every chunk
    attends to the quantised rows, its own included: the result is that of
    the quantised cache, not of the unquantised k and v as with the padded
    prefill."""
    dev = caches[0][0].device  # k of a (k, v) pair, KVCacheFp8 or KVCachePaged
    # slots: a paged cache's k is the pool, its table has one row per slot
    Bk = caches[0].table.shape[0] if isinstance(caches[0], ops.KVCachePaged) \
        else caches[0][0].shape[0]
    n = len(prompts)
    L = [len(p) for p in prompts]
    last = [None] * n
    for done in range(0, max(L), chunk):
        tok = torch.zeros(Bk, chunk, dtype=torch.int64)
        pos = torch.full((Bk,), -1, dtype=torch.int32)
        nn = torch.zeros(Bk, dtype=torch.int32)
        for b in range(n):
            r = min(chunk, L[b] - done)
            if r > 0:
                tok[b, :r] = torch.tensor(prompts[b][done:done + r],
                                          dtype=torch.int64)
                pos[b], nn[b] = done, r
        seq_pos = {"pos": pos.to(dev), "lens": ((pos + 1) * (nn > 0)).to(dev),
                   "n_new": nn.to(dev)}
        h = model(tok.to(dev), caches=caches, seq_pos=seq_pos)
        for b in range(n):
            if 0 < L[b] - done <= chunk:  # the prompt ends in this chunk
                last[b] = h[b, L[b] - done - 1]
    return torch.stack(last)


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


def _capture_ragged(model, sess, step=_ragged_step):
    """Capture `step` as one replayable hipGraph (warm-up on a side
    stream, per the torch CUDA-graphs contract, as _build_session)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step(model, sess)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sess["logits"] = step(model, sess)
    sess["graph"] = graph


def _multi_step(model, sess):
    """Up to T tokens for every live slot: logits [Bk, T, vocab]. The host
    writes tok / pos / lens / n_new before every step."""
    h = model(sess["tok"], caches=sess["caches"], seq_pos=sess)
    return model.lm_head(h)


def _prompt_lookup(seq, k: int) -> list:
    """The (at most k) tokens that followed the most recent earlier
    occurrence of seq's last two tokens; [] without one."""
    if len(seq) < 3:
        return []
    a, b = seq[-2], seq[-1]
    for i in range(len(seq) - 3, -1, -1):
        if seq[i] == a and seq[i + 1] == b:
            return seq[i + 2:i + 2 + k]
    return []


def _decode_lookahead(model, sess, graphing, K, prompts, out, done, max_new,
                      stops, temps, topks, gens):
    """Decode loop of generate_batch(lookahead=K): each step feeds a live
    sequence its last token plus a prompt-lookup draft (greedy sequences
    only, never longer than the tokens it may still produce) and accepts
    token by token while the model's argmax agrees with the draft."""
    n, Bk, T = len(prompts), sess["tok"].shape[0], K + 1
    while not all(done):
        live = [b for b in range(n) if not done[b]]
        tok = torch.zeros(Bk, T, dtype=torch.int64)
        pos = torch.full((Bk,), -1, dtype=torch.int32)
        nn = torch.zeros(Bk, dtype=torch.int32)
        drafts = {}
        for b in live:
            d = []
            if temps[b] <= 0:
                d = _prompt_lookup(prompts[b] + out[b], K)
                d = d[:max_new[b] - len(out[b]) - 1]
            drafts[b] = d
            row = [out[b][-1]] + d
            tok[b, :len(row)] = torch.tensor(row, dtype=torch.int64)
            pos[b] = len(prompts[b]) + len(out[b]) - 1
            nn[b] = len(row)
        sess["tok"].copy_(tok)
        sess["pos"].copy_(pos)
        sess["lens"].copy_((pos + 1) * (nn > 0))
        sess["n_new"].copy_(nn)
        if graphing:
            sess["graph"].replay()
            logits = sess["logits"]
        else:
            logits = _multi_step(model, sess)
        greedy = None
        for b in live:
            if temps[b] > 0:
                ys = [int(_sample(logits[b, :1], temps[b], topks[b], gens[b]))]
            else:
                if greedy is None:  # one device sync for all greedy rows
                    greedy = logits.argmax(-1).tolist()
                ys = greedy[b][:len(drafts[b]) + 1]
            for t, y in enumerate(ys):
                out[b].append(y)
                if len(out[b]) >= max_new[b] or y in stops:
                    done[b] = True
                    break
                if t >= len(drafts[b]) or drafts[b][t] != y:
                    break


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
