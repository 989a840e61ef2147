"""Ragged batched decoding on the CPU (llama_test, fp32 reference fallbacks):
generate_batch against solo generate, per-sequence seeds, stop tokens,
limits, the model's seq_pos guards and the two op fallbacks."""
import pytest
import torch

from prime_amd import ops
from prime_amd.models import build_model
from prime_amd.models.generate import generate, generate_batch

LENGTHS = (3, 10, 40)
MAX_NEW = [6, 2, 9]


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    m = build_model("llama_test")
    m.eval()
    return m


@pytest.fixture(scope="module")
def prompts(model):
    g = torch.Generator().manual_seed(1)
    return [torch.randint(0, model.cfg.vocab_size, (n,), generator=g).tolist()
            for n in LENGTHS]


@pytest.fixture(scope="module")
def greedy(model, prompts):
    return generate_batch(model, prompts, MAX_NEW)


def test_ragged_greedy_equals_solo_greedy(model, prompts, greedy):
    assert [len(o) for o in greedy] == MAX_NEW
    for p, n, got in zip(prompts, MAX_NEW, greedy):
        solo = generate(model, torch.tensor([p]), n)[0, len(p):].tolist()
        assert got == solo


def test_seed_independent_of_batch(model, prompts):
    alone = generate_batch(model, [prompts[1]], 8, temperature=0.8, top_k=10,
                           seed=7)
    batch = generate_batch(model, prompts, 8, temperature=[0.0, 0.8, 0.0],
                           top_k=[0, 10, 0], seed=[None, 7, None])
    assert len(alone[0]) == 8 and batch[1] == alone[0]
    # and equal to the existing single-sequence sampler
    solo = generate(model, torch.tensor([prompts[1]]), 8, temperature=0.8,
                    top_k=10, seed=7)[0, len(prompts[1]):].tolist()
    assert alone[0] == solo


def test_stop_tokens(model, prompts, greedy):
    t = greedy[2][1]  # second greedy token of the longest sequence
    assert t not in greedy[0] and t not in greedy[1] and t != greedy[2][0]
    out = generate_batch(model, prompts, MAX_NEW, stop_token_ids=[t])
    assert out[2] == greedy[2][:2] and out[2][-1] == t
    assert out[0] == greedy[0] and out[1] == greedy[1]


def test_limits(model, prompts):
    with pytest.raises(ValueError):
        generate_batch(model, [prompts[0], []], 4)
    with pytest.raises(ValueError):
        generate_batch(model, prompts, [4, 4, model.cfg.max_seq - 39])
    with pytest.raises(ValueError):
        generate_batch(model, prompts, [4, 4])  # one value per sequence
    assert generate_batch(model, [], 4) == []


def test_model_seq_pos_guards(model):
    cfg = model.cfg
    B = 2

    def caches():
        return [(torch.zeros(B, 64, cfg.n_kv_heads, cfg.head_dim),
                 torch.zeros(B, 64, cfg.n_kv_heads, cfg.head_dim))
                for _ in range(cfg.n_layers)]

    sp = {"pos": torch.tensor([3, 5], dtype=torch.int32),
          "lens": torch.tensor([4, 6], dtype=torch.int32)}
    one = torch.zeros(B, 1, dtype=torch.int64)
    with torch.no_grad():
        assert model(one, caches=caches(), seq_pos=sp).shape == (B, 1, cfg.dim)
        with pytest.raises(ValueError):  # S != 1
            model(torch.zeros(B, 2, dtype=torch.int64), caches=caches(), seq_pos=sp)
        with pytest.raises(ValueError):  # no caches
            model(one, seq_pos=sp)
        with pytest.raises(ValueError):  # document mask
            model(one, caches=caches(), seq_pos=sp,
                  doc_start=torch.zeros(B, 1, dtype=torch.int32))
        with pytest.raises(ValueError):  # scalar graph position
            model(one, caches=caches(), seq_pos=sp,
                  pos_dev={"pos32": torch.zeros((), dtype=torch.int32)})
        attn = model.layers[0].attn
        x = torch.zeros(B, 1, cfg.dim)
        with pytest.raises(ValueError):  # layer level: no cache
            attn(x, model.rope_cos, model.rope_sin, seq_pos=sp)
        with pytest.raises(ValueError):  # layer level: doc_start
            attn(x, model.rope_cos, model.rope_sin, cache=caches()[0],
                 seq_pos=sp, doc_start=torch.zeros(B, 1, dtype=torch.int32))


def _softmax_attn(q, k, v):
    """q [H,D], k/v [L,Hkv,D] -> [H,D], written out by hand."""
    H, D = q.shape
    G = H // k.shape[1]
    out = torch.zeros(H, D)
    for h in range(H):
        kh, vh = k[:, h // G], v[:, h // G]
        s = (kh @ q[h]) / D ** 0.5
        p = torch.exp(s - s.max())
        out[h] = (p / p.sum()) @ vh
    return out


def test_attn_decode_ragged_fallback():
    torch.manual_seed(2)
    B, H, Hkv, D, Smax = 4, 6, 2, 16, 12  # G = 3: the fallback takes any group
    q = torch.randn(B, H, D)
    kc = torch.randn(B, Smax, Hkv, D)
    vc = torch.randn(B, Smax, Hkv, D)
    lens = torch.tensor([5, 0, Smax, Smax + 7], dtype=torch.int32)
    kc[1] = float("nan")  # idle slot: never read
    vc[1] = float("nan")
    kc[0, 5:] = float("nan")  # rows past the length: never read
    vc[0, 5:] = float("nan")
    o = ops.attn_decode_ragged(q, kc, vc, lens)
    assert o.shape == (B, H, D) and torch.isfinite(o).all()
    assert (o[1] == 0).all()
    for b, n in ((0, 5), (2, Smax), (3, Smax)):  # the last one is clamped
        torch.testing.assert_close(o[b], _softmax_attn(q[b], kc[b, :n], vc[b, :n]),
                                   atol=1e-5, rtol=1e-5)
    o4 = ops.attn_decode_ragged(q.unsqueeze(1), kc, vc, lens)
    assert torch.equal(o4, o)
    with pytest.raises(ValueError):
        ops.attn_decode_ragged(q, kc, vc, lens.long())


def test_decode_qkv_append_fallback():
    torch.manual_seed(3)
    B, H, Hkv, D, Smax, T = 4, 4, 2, 16, 8, 32
    cos, sin = ops.reference.rope_tables(D, T)
    qkv = torch.randn(B, (H + 2 * Hkv) * D)
    pos = torch.tensor([5, Smax, 0, -1], dtype=torch.int32)
    kc = torch.full((B, Smax, Hkv, D), 7.0)
    vc = torch.full((B, Smax, Hkv, D), 7.0)
    q = ops.decode_qkv_append(qkv, cos, sin, kc, vc, pos, H, Hkv)
    x = qkv.view(B, H + 2 * Hkv, D)
    half = D // 2

    def rot(v, p):  # NeoX half-split rotation of [heads, D] at position p
        c, s = cos[p], sin[p]
        return torch.cat([v[:, :half] * c - v[:, half:] * s,
                          v[:, half:] * c + v[:, :half] * s], -1)

    for b, p in ((0, 5), (2, 0)):
        torch.testing.assert_close(q[b], rot(x[b, :H], p))
        torch.testing.assert_close(kc[b, p], rot(x[b, H:H + Hkv], p))
        assert torch.equal(vc[b, p], x[b, H + Hkv:])
        keep = torch.ones(Smax, dtype=torch.bool)
        keep[p] = False
        assert (kc[b, keep] == 7).all() and (vc[b, keep] == 7).all()
    for b in (1, 3):  # out of range / idle: nothing written, q zero
        assert (q[b] == 0).all()
        assert (kc[b] == 7).all() and (vc[b] == 7).all()


def test_split_helper_and_chunk_constant():
    C = ops.DECODE_RAGGED_CHUNK
    assert C == 256
    for B, Hkv, Smax in ((1, 8, 4096), (8, 8, 4096), (3, 2, 512), (64, 8, 300),
                         (1, 1, 100000)):
        rows = ops.decode_ragged_split(B, Hkv, Smax)
        assert rows >= C and rows % C == 0
        nsplit = -(-Smax // rows)
        assert nsplit >= 1 and (nsplit - 1) * rows < Smax
    # enough work already: one split per (b, kv head)
    assert ops.decode_ragged_split(128, 8, 1024) == 1024
    # a lone sequence is split to fill the machine
    assert ops.decode_ragged_split(1, 8, 4096) == C
