"""Multi-token ragged decode on the CPU: the fallbacks of the two ops, the
model guards and generate_batch(lookahead=...) on an fp32 model."""
import pytest
import torch


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def test_attn_fallback_matches_plain_softmax():
    from prime_amd import ops

    torch.manual_seed(0)
    B, T, H, Hkv, D, Smax = 3, 3, 4, 2, 8, 10
    q = torch.randn(B, T, H, D)
    kc, vc = torch.randn(B, Smax, Hkv, D), torch.randn(B, Smax, Hkv, D)
    lens, n_new = [4, 0, 9], [3, 3, 7]  # slot 2: n clamps to Smax - 9 + 1 = 2
    got = ops.attn_decode_ragged_multi(q, kc, vc, _i32(lens), _i32(n_new))
    want = torch.zeros_like(q)
    for b, t, rows in ((0, 0, 4), (0, 1, 5), (0, 2, 6), (2, 0, 9), (2, 1, 10)):
        for h in range(H):
            k, v = kc[b, :rows, h // 2], vc[b, :rows, h // 2]
            p = torch.softmax(k @ q[b, t, h] * D ** -0.5, 0)
            want[b, t, h] = p @ v
    torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-5)
    assert (got[1] == 0).all() and (got[2, 2] == 0).all()


def test_append_fallback_matches_apply_rope():
    from prime_amd import ops

    torch.manual_seed(1)
    B, T, H, Hkv, D, Smax = 3, 3, 2, 1, 8, 6
    cos, sin = ops.reference.rope_tables(D, 16)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D)
    kc, vc = torch.full((B, Smax, Hkv, D), 7.0), torch.full((B, Smax, Hkv, D), 7.0)
    pos, n_new = [1, -1, 4], [2, 3, 3]  # slot 2: token 2 would be row 6 = Smax
    q = ops.decode_qkv_append_multi(qkv, cos, sin, kc, vc, _i32(pos),
                                    _i32(n_new), H, Hkv)
    x = qkv.view(B, T, H + 2 * Hkv, D)
    live = {(0, 0): 1, (0, 1): 2, (2, 0): 4, (2, 1): 5}
    keep = torch.ones(B, Smax, dtype=torch.bool)
    for b in range(B):
        for t in range(T):
            if (b, t) not in live:
                assert (q[b, t] == 0).all()
                continue
            p = live[b, t]
            keep[b, p] = False
            xt = x[b:b + 1, t:t + 1]
            assert torch.equal(q[b, t], ops.reference.apply_rope(
                xt[:, :, :H], cos, sin, p)[0, 0])
            assert torch.equal(kc[b, p], ops.reference.apply_rope(
                xt[:, :, H:H + Hkv], cos, sin, p)[0, 0])
            assert torch.equal(vc[b, p], x[b, t, H + Hkv:])
    assert (kc[keep] == 7).all() and (vc[keep] == 7).all()


@pytest.fixture(scope="module")
def model():
    from prime_amd.models import Llama
    from prime_amd.models.configs import get_config

    torch.manual_seed(0)
    cfg = get_config("llama_150m", n_layers=2, dim=64, n_heads=4, n_kv_heads=2,
                     intermediate=128, vocab_size=24, max_seq=256)
    return Llama(cfg).eval()


@torch.no_grad()
def test_model_guards(model):
    from prime_amd import ops

    cfg = model.cfg
    caches = [tuple(torch.zeros(1, 64, cfg.n_kv_heads, cfg.head_dim)
                    for _ in range(2)) for _ in range(cfg.n_layers)]
    sp = {"pos": _i32([3]), "lens": _i32([4])}
    toks = torch.zeros(1, 2, dtype=torch.int64)
    with pytest.raises(ValueError):  # T > 1 needs "n_new"
        model(toks, caches=caches, seq_pos=sp)
    sp["n_new"] = _i32([2])
    assert model(toks, caches=caches, seq_pos=sp).shape == (1, 2, cfg.dim)
    fp8 = [ops.kv_cache_fp8(1, 64, cfg.n_kv_heads, cfg.head_dim, "cpu")
           for _ in range(cfg.n_layers)]
    with pytest.raises(NotImplementedError):
        model(toks, caches=fp8, seq_pos=sp)


def test_generate_batch_lookahead_equals_plain_decoding(model):
    from prime_amd.models.generate import generate_batch

    prompts = [[1, 2, 3] * 6, [5, 6] * 9 + [5], list(range(4, 21))]
    new = [40, 40, 12]
    calls = []
    hook = model.register_forward_hook(lambda *a: calls.append(1))
    base = generate_batch(model, prompts, new)
    n_base, calls[:] = len(calls), []
    look = generate_batch(model, prompts, new, lookahead=3)
    n_look = len(calls)
    hook.remove()
    assert look == base and [len(o) for o in look] == new
    print(f"model passes: plain {n_base}, lookahead {n_look}")
    assert n_look < n_base  # drafts were accepted

    # a stop token inside an accepted run ends the sequence there: the
    # plain path fixes where each sequence must stop
    stop = base[0][len(base[0]) // 2]
    want = generate_batch(model, prompts, new, stop_token_ids=[stop])
    got = generate_batch(model, prompts, new, stop_token_ids=[stop], lookahead=3)
    assert got == want and any(len(o) < m for o, m in zip(got, new))
