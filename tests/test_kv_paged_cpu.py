"""Paged KV cache without a GPU: the layout's definition, the host paths of
the four paged ops against the contiguous host paths, the page allocator and
generate_batch's argument checks."""
import pytest
import torch

from prime_amd import ops

B, H, HKV, D, P, MP = 3, 4, 2, 64, 64, 3  # Smax = 192


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def _shuffled(kc, vc):
    """kc, vc [B,Smax,Hkv,D] behind a shuffled table, 4 spare pool pages."""
    cache = ops.kv_cache_paged(B * MP + 4, P, B, MP, HKV, D,
                               dtype=torch.float32)
    perm = torch.randperm(B * MP + 4)[:B * MP].view(B, MP)
    cache.table.copy_(perm)
    cache.k[perm.flatten()] = kc.reshape(B * MP, P, HKV, D)
    cache.v[perm.flatten()] = vc.reshape(B * MP, P, HKV, D)
    return cache


def test_gather_is_the_layout():
    torch.manual_seed(0)
    cache = _shuffled(torch.randn(B, MP * P, HKV, D), torch.randn(B, MP * P, HKV, D))
    cache.table[1, 2], cache.table[2, 0] = -1, B * MP + 4  # outside the pool
    k, v = ops.kv_paged_gather(cache)
    assert k.shape == v.shape == (B, MP * P, HKV, D)
    for b in range(B):
        for r in (0, 1, P - 1, P, 2 * P + 5, MP * P - 1):
            e = int(cache.table[b, r // P])
            if 0 <= e < B * MP + 4:
                row = e * P + r % P  # the format, written out
                assert torch.equal(k[b, r], cache.k.view(-1, HKV, D)[row])
                assert torch.equal(v[b, r], cache.v.view(-1, HKV, D)[row])
            else:
                assert (k[b, r] == 0).all() and (v[b, r] == 0).all()


@pytest.mark.parametrize("op", ["decode", "prefill", "append1", "appendT"])
def test_host_paths_match_contiguous(op):
    torch.manual_seed(1)
    Smax, T = MP * P, 7
    kc, vc = torch.randn(B, Smax, HKV, D), torch.randn(B, Smax, HKV, D)
    cache = _shuffled(kc, vc)
    lens, n_new = _i32([70, 0, Smax + 9]), _i32([T, 3, 2])
    if op == "decode":
        q = torch.randn(B, H, D)
        assert torch.equal(ops.attn_decode_ragged_paged(q, cache, lens),
                           ops.attn_decode_ragged(q, kc, vc, lens))
        return
    if op == "prefill":
        q = torch.randn(B, T, H, D)
        assert torch.equal(ops.attn_prefill_ragged_paged(q, cache, lens, n_new),
                           ops.attn_prefill_ragged(q, kc, vc, lens, n_new))
        return
    cos, sin = ops.reference.rope_tables(D, 256)
    qkv = torch.randn(B, T, (H + 2 * HKV) * D)
    pos = _i32([60, -1, Smax - 2])  # crosses a page; idle; crosses Smax
    if op == "append1":
        q = ops.decode_qkv_append_paged(qkv[:, 0], cos, sin, cache, pos, H, HKV)
        q2 = ops.decode_qkv_append(qkv[:, 0], cos, sin, kc, vc, pos, H, HKV)
    else:
        q = ops.prefill_qkv_append_paged(qkv, cos, sin, cache, pos, n_new, H, HKV)
        q2 = ops.prefill_qkv_append(qkv, cos, sin, kc, vc, pos, n_new, H, HKV)
    k, v = ops.kv_paged_gather(cache)
    assert torch.equal(q, q2) and torch.equal(k, kc) and torch.equal(v, vc)
    cache.table[0, 0] = -1  # an invalid entry kills the token, writes nothing
    before = cache.k.clone()
    q = ops.decode_qkv_append_paged(qkv[:, 0], cos, sin, cache, pos, H, HKV)
    assert (q[0] == 0).all() and torch.equal(cache.k, before)


def test_page_allocator():
    pages = ops.KVPageAllocator(6)
    a, b = pages.alloc(2), pages.alloc(3)
    assert len(set(a + b)) == 5 and all(0 <= p < 6 for p in a + b)
    with pytest.raises(ValueError):
        pages.alloc(2)
    assert pages.n_free == 1  # a failed request takes nothing
    pages.free(a)
    c = pages.alloc(3)
    assert pages.n_free == 0 and not set(c) & set(b)


@torch.no_grad()
def test_generate_batch_arguments():
    from prime_amd.models import Llama
    from prime_amd.models.configs import get_config
    from prime_amd.models.generate import generate_batch

    torch.manual_seed(0)
    model = Llama(get_config("llama_test")).eval()
    prompts = [[1, 2, 3, 4, 5], list(range(1, 71))]
    need = -(-(5 + 3) // 64) + -(-(70 + 3) // 64)
    kw = dict(kv_layout="paged", page_size=64)
    want = generate_batch(model, prompts, 3, prefill_chunk=64)
    assert generate_batch(model, prompts, 3, kv_pages=need, **kw) == want
    for bad in (dict(kv_pages=need - 1), dict(kv_dtype="fp8"),
                dict(lookahead=2), dict(page_size=96)):
        with pytest.raises(ValueError):
            generate_batch(model, prompts, 3, **{**kw, **bad})
    with pytest.raises(ValueError):
        generate_batch(model, prompts, 3, kv_layout="blocked")
