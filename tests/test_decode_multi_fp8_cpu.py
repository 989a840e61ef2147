"""Multi-token ragged decode over the fp8 KV cache on the CPU: the fallbacks
of the two ops and the generate_batch guard for a model that is not on a GPU."""
import pytest
import torch

from tests.test_decode_multi_cpu import _i32, model  # noqa: F401


def test_attn_fallback_matches_plain_softmax():
    from prime_amd import ops

    torch.manual_seed(0)
    B, T, H, Hkv, D, Smax = 3, 3, 4, 2, 8, 10
    q = torch.randn(B, T, H, D)
    c = ops.kv_cache_fp8(B, Smax, Hkv, D)
    ops.kv_store_fp8(c, torch.randn(B, Smax, Hkv, D) * 3,
                     torch.randn(B, Smax, Hkv, D) / 5, 0)
    kc, vc = ops.kv_cache_dequant(c)
    lens, n_new = [4, 0, 9], [3, 3, 7]  # slot 2: n clamps to Smax - 9 + 1 = 2
    got = ops.attn_decode_ragged_multi_fp8(q, c, _i32(lens), _i32(n_new))
    want = torch.zeros_like(q)
    for b, t, rows in ((0, 0, 4), (0, 1, 5), (0, 2, 6), (2, 0, 9), (2, 1, 10)):
        for h in range(H):
            k, v = kc[b, :rows, h // 2], vc[b, :rows, h // 2]
            p = torch.softmax(k @ q[b, t, h] * D ** -0.5, 0)
            want[b, t, h] = p @ v
    torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-5)
    assert (got[1] == 0).all() and (got[2, 2] == 0).all()


def test_append_fallback_matches_quantised_apply_rope():
    from prime_amd import ops
    from prime_amd.ops.functional import _kv_quant

    torch.manual_seed(1)
    B, T, H, Hkv, D, Smax = 3, 3, 2, 1, 8, 6
    cos, sin = ops.reference.rope_tables(D, 16)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D)
    c = ops.kv_cache_fp8(B, Smax, Hkv, D)
    for t in c:
        t.view(torch.uint8).fill_(0x55)
    pos, n_new = [1, -1, 4], [2, 3, 3]  # slot 2: token 2 would be row 6 = Smax
    q = ops.decode_qkv_append_multi_fp8(qkv, cos, sin, c, _i32(pos),
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
            for by, sc, w in (
                    (c.k, c.k_scale, ops.reference.apply_rope(
                        xt[:, :, H:H + Hkv], cos, sin, p)[0, 0]),
                    (c.v, c.v_scale, x[b, t, H + Hkv:])):
                wq, ws = _kv_quant(w)
                assert torch.equal(by[b, p].view(torch.uint8), wq.view(torch.uint8))
                assert torch.equal(sc[b, p], ws)
    for t in c:
        assert (t[keep].view(torch.uint8) == 0x55).all()


def test_generate_batch_lookahead_fp8_needs_a_gpu_model(model):
    from prime_amd.models.generate import generate_batch

    with pytest.raises(NotImplementedError):
        generate_batch(model, [[1, 2, 3]], 4, lookahead=2, kv_dtype="fp8")
