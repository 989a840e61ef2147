"""Chunked ragged prefill over the fp8 KV cache on the GPU. The reference is
ops.reference.attention in fp32 on the CPU over the dequantised cache rows: it
sees exactly the stored values, so the decode tolerance covers kernel error
only. Rows carry their own scale factors (the multi-token fp8 test's inputs),
so a scale taken from the wrong row is far outside the tolerance."""
import pytest
import torch

from tests.test_decode_fp8kv_gpu import _sentinel_cache, _u8, _untouched
from tests.test_decode_multi_fp8_gpu import _inputs
from tests.test_decode_multi_gpu import DEV, TOL, _i32, _live, _seed, model  # noqa: F401

pytestmark = pytest.mark.gpu


def _raw(t):  # bytes of an e4m3 tensor, scales as they are
    return _u8(t) if t.dtype == torch.float8_e4m3fn else t


def _run(q, c, lens, n_new, poison=False, **kw):
    """The op against the reference per (b, t) on rows [0, L0 + t); dead rows
    exactly zero. poison: NaN bytes and scales wherever the kernel may not
    load."""
    from prime_amd import ops

    T, Smax = q.shape[1], c.k.shape[1]
    if poison:
        for b, (L, n) in enumerate(zip(lens, n_new)):
            L0, n = _live(L, n, T, Smax)
            dead = slice(L0 + n - 1 if n else 0, None)
            _u8(c.k)[b, dead] = 0x7F  # e4m3 NaN
            _u8(c.v)[b, dead] = 0x7F
            c.k_scale[b, dead] = float("nan")
            c.v_scale[b, dead] = float("nan")
    got = ops.attn_prefill_ragged_fp8(q, c, _i32(lens), _i32(n_new), **kw)
    assert got.shape == q.shape and got.dtype == torch.bfloat16
    out, qf = got.float().cpu(), q.float().cpu()
    assert torch.isfinite(out).all()
    cpu = ops.KVCacheFp8(*(t.cpu() for t in c))
    for b, (L, n) in enumerate(zip(lens, n_new)):
        L0, n = _live(L, n, T, Smax)
        assert (out[b, n:] == 0).all()
        for t in range(n):
            kd, vd = ops.kv_cache_dequant(
                ops.KVCacheFp8(*(x[b:b + 1, :L0 + t] for x in cpu)))
            want = ops.reference.attention(qf[b:b + 1, t:t + 1], kd, vd,
                                           causal=False)[0, 0]
            torch.testing.assert_close(out[b, t], want, **TOL)
    return got


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2), (8, 1)])
def test_row_tiling(H, Hkv, D):
    from prime_amd import ops

    KT = ops.PREFILL_KEY_TILE
    T = ops.PREFILL_Q_ROWS // (H // Hkv) + 5  # a partial second q-tile
    Smax = 4 * KT + 64
    _run(*_inputs(4, T, H, Hkv, D, Smax), [1, KT - 1, KT, Smax - T + 1],
         [T, T, T - 1, T])


@pytest.mark.parametrize("split_rows", [None, 2])
def test_key_tile_and_split_boundaries(split_rows):
    from prime_amd import ops

    KT, T, Smax = ops.PREFILL_KEY_TILE, 24, 4 * ops.PREFILL_KEY_TILE + 64
    n_cu = torch.cuda.get_device_properties(DEV).multi_processor_count
    kw = {} if split_rows is None else {"split_rows": split_rows * KT}
    rows = kw.get("split_rows") or ops.prefill_ragged_split(13, 1, T, 8, Smax, n_cu)
    lens = sorted({e + d for e in (KT, 2 * KT, rows) for d in (-T, -1, 0, 1)}
                  | {Smax - T + 1})
    _run(*_inputs(len(lens), T, 8, 1, 64, Smax), lens, [T] * len(lens), **kw)


def test_dead_rows_and_scales_are_not_read():
    # NaN bytes and scales at and beyond L0 + n - 1; slot 1 idle, slot 2
    # n_new = 0 (whole cache NaN), slot 3 one live token of T
    T = 40
    _run(*_inputs(4, T, 8, 2, 128, 320), [200, 0, 257, 130], [T, T, 0, 1],
         poison=True)


def test_every_e4m3_code_through_both_staging_paths():
    """Rows 0..3 of K and of V hold the bytes 0..255 (NaN codes zeroed)."""
    from prime_amd import ops

    D, Smax = 64, 256
    codes = torch.arange(256, dtype=torch.uint8)
    codes[codes & 0x7F == 0x7F] = 0
    c = ops.kv_cache_fp8(1, Smax, 1, D, DEV)
    _u8(c.k)[0, :4, 0] = codes.view(4, D).to(DEV)
    _u8(c.v)[0, :4, 0] = codes.view(4, D).to(DEV)
    c.k_scale.fill_(2.0 ** -9)
    c.v_scale.fill_(2.0 ** -4)
    _run(torch.randn(1, 2, 1, D).to(DEV, dtype=torch.bfloat16), c, [4], [1])


def test_clamp_agreement_and_reproducibility():
    from prime_amd import ops

    T, Smax = 40, 320
    q, c = _inputs(3, T, 8, 2, 128, Smax)
    a = ops.attn_prefill_ragged_fp8(q, c, _i32([Smax + 1000, 200, -5]),
                                    _i32([T, T + 5, T]))
    b = _run(q, c, [Smax, 200, 0], [1, T, 0])
    assert torch.equal(a, b)
    assert torch.equal(b, ops.attn_prefill_ragged_fp8(
        q, c, _i32([Smax, 200, 0]), _i32([1, T, 0])))
    # T = 4: the multi-token fp8 decode kernel
    q, c = _inputs(3, 4, 8, 2, 128, Smax)
    lens, n_new = [300, 1, 77], [4, 4, 3]
    new = _run(q, c, lens, n_new)
    old = ops.attn_decode_ragged_multi_fp8(q, c, _i32(lens), _i32(n_new))
    torch.testing.assert_close(new.float(), old.float(), **TOL)


def test_graph_replay_with_changing_lengths():
    from prime_amd import ops

    KT = ops.PREFILL_KEY_TILE
    q, c = _inputs(3, 40, 8, 2, 128, 320)
    lens, n_new = _i32([1, 1, 1]), _i32([1, 1, 1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ops.attn_prefill_ragged_fp8(q, c, lens, n_new, split_rows=2 * KT)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attn_prefill_ragged_fp8(q, c, lens, n_new, split_rows=2 * KT)
    for L, n in (([200, 1, 281], [40, 2, 40]), ([0, 129, 64], [40, 40, 0]),
                 ([77, 0, 320], [1, 3, 40])):
        lens.copy_(_i32(L))
        n_new.copy_(_i32(n))
        graph.replay()
        assert torch.equal(out.clone(), _run(q, c, L, n, split_rows=2 * KT))


@pytest.mark.parametrize("T", [4, 19])
def test_prefill_qkv_append_fp8(T):
    from prime_amd import ops

    B, H, Hkv, D, Smax = 4, 8, 2, 64, 64
    cos, sin = ops.reference.rope_tables(D, 256, device=DEV)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D).to(DEV, dtype=torch.bfloat16)
    # slot 1 idle, slot 2 crosses Smax at t = 2, slot 3 has n_new < T
    pos, n_new = [5, -1, Smax - 2, 0], [T, T, T, T - 2]
    c, one = (_sentinel_cache(B, Smax, Hkv, D) for _ in range(2))  # 0x55, 7.0
    q = ops.prefill_qkv_append_fp8(qkv, cos, sin, c, _i32(pos), _i32(n_new),
                                   H, Hkv)
    kc = torch.zeros(B, Smax, Hkv, D, device=DEV, dtype=torch.bfloat16)
    assert torch.equal(q, ops.prefill_qkv_append(
        qkv, cos, sin, kc, torch.zeros_like(kc), _i32(pos), _i32(n_new), H, Hkv))
    keep = torch.ones(B, Smax, dtype=torch.bool, device=DEV)
    for t in range(T):  # the same rows through the single-token kernel
        live = [p >= 0 and t < n and p + t < Smax for p, n in zip(pos, n_new)]
        ops.decode_qkv_append_fp8(
            qkv[:, t].contiguous(), cos, sin, one,
            _i32([p + t if ok else -1 for p, ok in zip(pos, live)]), H, Hkv)
        for b in range(B):
            if live[b]:
                keep[b, pos[b] + t] = False
    assert not keep.all()
    for ta, tb in zip(c, one):  # live rows equal, the others the sentinel
        assert torch.equal(_raw(ta), _raw(tb))
    _untouched(c, keep)


@pytest.mark.parametrize("H,Hkv,D", [(6, 2, 64), (8, 2, 96)])  # G = 3; D = 96
def test_unsupported_shapes_raise(H, Hkv, D):
    from prime_amd import ops
    from prime_amd.ops._lib import lib, ptr, stream_of

    q = torch.randn(1, 16, H, D).to(DEV, dtype=torch.bfloat16)
    c = ops.kv_cache_fp8(1, 256, Hkv, D, DEV)
    one = _i32([1])
    with pytest.raises(NotImplementedError):
        ops.attn_prefill_ragged_fp8(q, c, _i32([5]), one)
    assert lib().prime_attn_prefill_ragged_fp8(
        stream_of(q), ptr(q), ptr(c.k), ptr(c.v), ptr(c.k_scale),
        ptr(c.v_scale), ptr(torch.empty_like(q)), ptr(None), ptr(one),
        ptr(one), 1, 16, H, Hkv, 256, D, 256, 0.125) == 1  # hipErrorInvalidValue


@torch.no_grad()
def test_model_chunked_prefill_matches_eight_token_steps(model):
    from prime_amd import ops
    from prime_amd.models import Llama
    from prime_amd.models.generate import prefill_chunked

    cfg, L = model.cfg, (5, 70, 133)
    g = torch.Generator().manual_seed(5)
    toks = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in L]
    m32 = Llama(cfg)  # fp32 CPU model with the same (bf16-valued) weights
    m32.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    ref = [m32.eval()(t[None])[0, -1] for t in toks]

    def caches():  # one padding slot
        return [ops.kv_cache_fp8(4, 256, cfg.n_kv_heads, cfg.head_dim, DEV)
                for _ in range(cfg.n_layers)]

    prompts = [t.tolist() for t in toks]
    c_old, c_new = caches(), caches()
    old = prefill_chunked(model, c_old, prompts, 8)  # the multi-token fp8 path
    new = prefill_chunked(model, c_new, prompts, 64)
    for b, n in enumerate(L):
        e_old = (old[b].float().cpu() - ref[b]).abs().max().item()
        e_new = (new[b].float().cpu() - ref[b]).abs().max().item()
        print(f"L={n}: max abs err vs fp32 CPU model: 8-token fp8 steps "
              f"{e_old:.4e}, chunked fp8 prefill {e_new:.4e}")
        assert e_new <= 2 * e_old + 1e-3
        for t_new, t_old in zip(c_new[0], c_old[0]):  # layer-0 bytes, scales
            assert torch.equal(_raw(t_new)[b, :n], _raw(t_old)[b, :n])
    assert all((_raw(t)[3] == 0).all() for t in c_new[0])  # the idle slot


def test_generate_batch_chunked_fp8_graphed_matches_eager(model):
    from prime_amd.models.generate import generate_batch

    g = torch.Generator().manual_seed(6)
    ps = [torch.randint(0, model.cfg.vocab_size, (n,), generator=g).tolist()
          for n in (5, 70, 133)]
    new = [12, 3, 8]
    eager = generate_batch(model, ps, new, use_graph=False, prefill_chunk=64,
                           kv_dtype="fp8")
    graphed = generate_batch(model, ps, new, use_graph=True, prefill_chunk=64,
                             kv_dtype="fp8")
    assert graphed == eager and [len(o) for o in eager] == new
