"""Paged KV cache on the GPU: the block-table decode, prefill and append
kernels against (1) ops.reference.attention in fp32 on the CPU over
kv_paged_gather and (2) their contiguous siblings, bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(atol=3e-2, rtol=3e-2)  # the project's decode tolerance


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _rand(*shape):
    return torch.randn(*shape).to(DEV, dtype=torch.bfloat16)


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(97)


def _paged(kc, vc, P, live, fill=float("nan")):
    """A pool holding the contiguous caches kc, vc [B,Smax,Hkv,D] behind a
    shuffled table, with 5 pages more than are used. Only pages of sequence b
    with a row below live[b] are copied and named; every other pool page is
    `fill`, every other table entry is -1 or n_pages + 7."""
    from prime_amd import ops

    B, Smax, Hkv, D = kc.shape
    mp = Smax // P
    cache = ops.kv_cache_paged(B * mp + 5, P, B, mp, Hkv, D, DEV)
    cache.k.fill_(fill), cache.v.fill_(fill)
    perm = torch.randperm(B * mp + 5)[:B * mp].view(B, mp).tolist()
    for b in range(B):
        for j in range(mp):
            if j * P < live[b]:
                cache.table[b, j] = perm[b][j]
                cache.k[perm[b][j]] = kc[b, j * P:(j + 1) * P]
                cache.v[perm[b][j]] = vc[b, j * P:(j + 1) * P]
            else:
                cache.table[b, j] = (-1, B * mp + 12)[j & 1]
    return cache


def _check(got, q, cache, L0, n):
    """got [B,T,H,D] against the fp32 CPU reference over kv_paged_gather:
    query t < n[b] of sequence b attends to rows [0, L0[b] + t), the others
    are exact zeros. One causal call per sequence: query t sits at position
    L0 + t - 1 of a length L0 + n - 1 sequence."""
    from prime_amd import ops

    out, qf = got.float().cpu(), q.float().cpu()
    kf, vf = (x.float().cpu() for x in ops.kv_paged_gather(cache))
    assert torch.isfinite(out).all()
    for b in range(q.shape[0]):
        assert (out[b, n[b]:] == 0).all()
        if n[b]:
            S = L0[b] + n[b] - 1
            qq = torch.zeros(1, S, *qf.shape[2:])
            qq[0, L0[b] - 1:] = qf[b, :n[b]]
            want = ops.reference.attention(qq, kf[b:b + 1, :S], vf[b:b + 1, :S])
            torch.testing.assert_close(out[b, :n[b]], want[0, L0[b] - 1:], **TOL)


@pytest.mark.parametrize("split_rows", [256, 512])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 1)])
@pytest.mark.parametrize("P", [64, 128, 256])
def test_decode(P, H, Hkv, D, split_rows):
    from prime_amd import ops

    Smax = 1024
    lens = [0, 1, P - 1, P, P + 1, 255, 256, 257, Smax, Smax + 1000]
    B, L = len(lens), [min(x, Smax) for x in lens]
    q, kc, vc = _rand(B, H, D), _rand(B, Smax, Hkv, D), _rand(B, Smax, Hkv, D)
    cache = _paged(kc, vc, P, L)  # dead pages NaN, their entries invalid
    got = ops.attn_decode_ragged_paged(q, cache, _i32(lens), split_rows=split_rows)
    assert (got[0] == 0).all()
    _check(got[:, None], q[:, None], cache, L, [int(x > 0) for x in L])
    assert torch.equal(got, ops.attn_decode_ragged(q, kc, vc, _i32(lens),
                                                   split_rows=split_rows))


@pytest.mark.parametrize("split_rows", [128, None])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", [1, 8])
@pytest.mark.parametrize("P", [64, 128, 256])
def test_prefill(P, G, D, split_rows):
    from prime_amd import ops

    T, Smax = 128 // G + 5, -(-320 // P) * P
    Hkv = 2 if G == 1 else 1
    lens = [L for L in (1, 63, 64, P, P + 1, Smax - T + 1) for _ in range(4)]
    n_new = [T, T - 1, 1, 0] * 6
    B = len(lens)
    n = [min(x, T, Smax - L + 1) for L, x in zip(lens, n_new)]
    q = _rand(B, T, Hkv * G, D)
    kc, vc = _rand(B, Smax, Hkv, D), _rand(B, Smax, Hkv, D)
    cache = _paged(kc, vc, P, [L + x - 1 if x else 0 for L, x in zip(lens, n)])
    got = ops.attn_prefill_ragged_paged(q, cache, _i32(lens), _i32(n_new),
                                        split_rows=split_rows)
    _check(got, q, cache, lens, n)
    assert torch.equal(got, ops.attn_prefill_ragged(
        q, kc, vc, _i32(lens), _i32(n_new), split_rows=split_rows))


def test_bad_and_shared_entries():
    """A used entry out of range or negative is clamped (finite output,
    values unspecified); table rows sharing pages give equal outputs."""
    from prime_amd import ops

    B, H, Hkv, D, P, Smax = 2, 8, 2, 128, 64, 512
    q = _rand(1, 20, H, D).expand(B, -1, -1, -1).contiguous()
    kc, vc = _rand(B, Smax, Hkv, D), _rand(B, Smax, Hkv, D)
    cache = _paged(kc, vc, P, [Smax] * B, fill=1.0)
    lens, n_new = _i32([300, 300]), _i32([20, 20])
    cache.table[1] = cache.table[0]  # read-only sharing
    for o in (ops.attn_decode_ragged_paged(q[:, 0], cache, lens),
              ops.attn_prefill_ragged_paged(q, cache, lens, n_new)):
        assert torch.equal(o[0], o[1])
    cache.table[0, 1], cache.table[1, 2] = 10**6, -5
    for o in (ops.attn_decode_ragged_paged(q[:, 0], cache, lens),
              ops.attn_prefill_ragged_paged(q, cache, lens, n_new)):
        assert torch.isfinite(o.float()).all()


@pytest.mark.parametrize("T", [1, 4, 19])
def test_append(T):
    from prime_amd import ops

    B, H, Hkv, D, P, mp, SENT = 5, 8, 2, 64, 64, 4, 3.0
    Smax = mp * P
    cos, sin = ops.reference.rope_tables(D, 512, device=DEV)
    qkv = _rand(B, T, (H + 2 * Hkv) * D)
    sent = torch.full((B, Smax, Hkv, D), SENT, device=DEV, dtype=torch.bfloat16)
    cache = _paged(sent, sent, P, [Smax] * B, fill=SENT)
    # slot 1 idle, 2 crosses Smax, 3 has n_new < T, 4's page 1 entry is -1
    # (its neighbours stay valid)
    pos, n_new = [5, -1, Smax - 2, 60, 70], [T, T, T, T - 2, T]
    cache.table[4, 1] = -1
    kc, vc = sent.clone(), sent.clone()
    pos_c = _i32(pos[:4] + [-1])  # the contiguous kernel sees slot 4 idle
    if T == 1:
        q = ops.decode_qkv_append_paged(qkv[:, 0], cos, sin, cache, _i32(pos), H, Hkv)
        q2 = ops.decode_qkv_append(qkv[:, 0], cos, sin, kc, vc, pos_c, H, Hkv)
    else:
        q = ops.prefill_qkv_append_paged(qkv, cos, sin, cache, _i32(pos),
                                         _i32(n_new), H, Hkv)
        q2 = ops.prefill_qkv_append(qkv, cos, sin, kc, vc, pos_c, _i32(n_new),
                                    H, Hkv)
    assert torch.equal(q, q2)
    # the pool the contiguous result scatters to; everything else keeps SENT
    want_k, want_v = (torch.full_like(cache.k, SENT) for _ in range(2))
    for b in range(B):
        for j, e in enumerate(cache.table[b].tolist()):
            if e >= 0:
                want_k[e], want_v[e] = kc[b, j * P:(j + 1) * P], vc[b, j * P:(j + 1) * P]
    assert torch.equal(cache.k, want_k) and torch.equal(cache.v, want_v)
    assert not torch.equal(kc, sent)  # something was written at all


@pytest.mark.parametrize("op", ["decode", "prefill"])
def test_graph_replay(op):
    """lens, n_new and the table contents change in place between replays
    (two sequences swap their pages); every replay equals an eager call."""
    from prime_amd import ops

    B, T, H, Hkv, D, P, Smax = 3, 40, 8, 2, 128, 64, 512
    q = _rand(B, T, H, D) if op == "prefill" else _rand(B, H, D)
    cache = _paged(_rand(B, Smax, Hkv, D), _rand(B, Smax, Hkv, D), P,
                   [Smax] * B, fill=0.5)
    lens, n_new = _i32([1] * B), _i32([1] * B)

    def run():
        if op == "prefill":
            return ops.attn_prefill_ragged_paged(q, cache, lens, n_new,
                                                 split_rows=128)
        return ops.attn_decode_ragged_paged(q, cache, lens, split_rows=256)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    seen = []
    for L, n in (([200, 1, 281], [40, 2, 40]), ([0, 129, 64], [40, 40, 0]),
                 ([77, 300, 472], [1, 3, 40])):
        lens.copy_(_i32(L)), n_new.copy_(_i32(n))
        cache.table[:2] = cache.table[:2].flip(0)  # swap two sequences' pages
        graph.replay()
        seen.append(out.clone())
        assert torch.equal(seen[-1], run())
    assert not torch.equal(seen[0][2], seen[2][2])


def test_invalid_arguments():
    from prime_amd import ops
    from prime_amd.ops._lib import lib, ptr, stream_of

    q, one = _rand(1, 8, 64), _i32([1])
    bad = ops.KVCachePaged(_rand(4, 32, 2, 64), _rand(4, 32, 2, 64),
                           torch.zeros(1, 4, dtype=torch.int32, device=DEV))
    with pytest.raises(NotImplementedError):
        ops.attn_decode_ragged_paged(q, bad, one)
    ok = ops.kv_cache_paged(4, 64, 1, 4, 2, 64, DEV)
    with pytest.raises(NotImplementedError):  # G = 3
        ops.attn_decode_ragged_paged(_rand(1, 6, 64), ok, one)
    ws = torch.empty(4096, device=DEV)
    for P, table in ((32, ok.table), (64, None)):
        assert lib().prime_attn_decode_ragged_paged(
            stream_of(q), ptr(q), ptr(ok.k), ptr(ok.v), ptr(torch.empty_like(q)),
            ptr(ws), ptr(one), ptr(table), 1, 8, 2, P, 4, 4, 64, 256,
            0.125) == 1  # hipErrorInvalidValue
        assert lib().prime_attn_prefill_ragged_paged(
            stream_of(q), ptr(q), ptr(ok.k), ptr(ok.v), ptr(torch.empty_like(q)),
            ptr(ws), ptr(one), ptr(one), ptr(table), 1, 1, 8, 2, P, 4, 4, 64,
            256, 0.125) == 1


@torch.no_grad()
def test_generate_batch_paged_matches_contiguous():
    from prime_amd.models import Llama
    from prime_amd.models.configs import get_config
    from prime_amd.models.generate import generate_batch

    torch.manual_seed(0)
    cfg = get_config("llama_150m", n_layers=2, n_heads=12, n_kv_heads=6)
    model = Llama(cfg).to(DEV, dtype=torch.bfloat16).eval()
    model.reset_rope(DEV)
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist()
               for n in (5, 70, 133)]
    want = generate_batch(model, prompts, 12, prefill_chunk=64)
    need = sum(-(-(len(p) + 12) // 64) for p in prompts)
    kw = dict(kv_layout="paged", page_size=64, prefill_chunk=64)
    assert generate_batch(model, prompts, 12, **kw) == want
    assert generate_batch(model, prompts, 12, kv_pages=need, **kw) == want
    with pytest.raises(ValueError):
        generate_batch(model, prompts, 12, kv_pages=need - 1, **kw)
    with pytest.raises(ValueError):
        generate_batch(model, prompts, 12, kv_dtype="fp8", **kw)
    with pytest.raises(ValueError):
        generate_batch(model, prompts, 12, lookahead=2, **kw)
