"""Chunked ragged prefill on the GPU: attn_prefill_ragged and
prefill_qkv_append against fp32 CPU references, then the model path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(atol=3e-2, rtol=3e-2)  # the decode tolerance of test_decode_multi_gpu


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(4321)


def _inputs(B, T, H, Hkv, D, Smax):
    return [torch.randn(s).to(DEV, dtype=torch.bfloat16)
            for s in ((B, T, H, D), (B, Smax, Hkv, D), (B, Smax, Hkv, D))]


def _live(L, n, T, Smax):
    L0 = min(max(L, 0), Smax)
    return (L0, min(max(n, 0), T, Smax - L0 + 1)) if L0 else (0, 0)


def _run(q, kc, vc, lens, n_new, poison=False, **kw):
    """The op against ops.reference.attention in fp32 on the CPU, per (b, t)
    on rows [0, L0 + t); dead rows must be exactly zero. poison: every row
    the kernel may not load is NaN."""
    from prime_amd import ops

    T, Smax = q.shape[1], kc.shape[1]
    if poison:
        for b, (L, n) in enumerate(zip(lens, n_new)):
            L0, n = _live(L, n, T, Smax)
            kc[b, L0 + n - 1 if n else 0:] = float("nan")
            vc[b, L0 + n - 1 if n else 0:] = float("nan")
    got = ops.attn_prefill_ragged(q, kc, vc, _i32(lens), _i32(n_new), **kw)
    assert got.shape == q.shape and got.dtype == torch.bfloat16
    out, qf, kf, vf = (x.float().cpu() for x in (got, q, kc, vc))
    assert torch.isfinite(out).all()
    for b, (L, n) in enumerate(zip(lens, n_new)):
        L0, n = _live(L, n, T, Smax)
        assert (out[b, n:] == 0).all()
        for t in range(n):
            want = ops.reference.attention(
                qf[b:b + 1, t:t + 1], kf[b:b + 1, :L0 + t], vf[b:b + 1, :L0 + t],
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
    assert rows % KT == 0
    assert kw or rows == ops.prefill_ragged_split(len(lens), 1, T, 8, Smax, n_cu)
    _run(*_inputs(len(lens), T, 8, 1, 64, Smax), lens, [T] * len(lens), **kw)


def test_dead_rows_are_not_read():
    # NaN at and beyond L0 + n - 1; slot 1 idle, slot 2 n_new = 0 (whole
    # caches NaN), slot 3 one live token of T
    T = 40
    _run(*_inputs(4, T, 8, 2, 128, 320), [200, 0, 257, 130], [T, T, 0, 1],
         poison=True)


def test_clamp_agreement_and_reproducibility():
    from prime_amd import ops
    from prime_amd.ops._lib import lib

    assert lib().prime_prefill_q_rows() == ops.PREFILL_Q_ROWS
    assert lib().prime_prefill_key_tile() == ops.PREFILL_KEY_TILE
    T, Smax = 40, 320
    q, kc, vc = _inputs(3, T, 8, 2, 128, Smax)
    a = ops.attn_prefill_ragged(q, kc, vc, _i32([Smax + 1000, 200, -5]),
                                _i32([T, T + 5, T]))
    b = _run(q, kc, vc, [Smax, 200, 0], [1, T, 0])
    assert torch.equal(a, b)
    assert torch.equal(b, ops.attn_prefill_ragged(
        q, kc, vc, _i32([Smax, 200, 0]), _i32([1, T, 0])))
    # T = 4: the multi-token decode kernel
    q, kc, vc = _inputs(3, 4, 8, 2, 128, Smax)
    lens, n_new = [300, 1, 77], [4, 4, 3]
    new = _run(q, kc, vc, lens, n_new)
    old = ops.attn_decode_ragged_multi(q, kc, vc, _i32(lens), _i32(n_new))
    torch.testing.assert_close(new.float(), old.float(), **TOL)
    # empty prefix: the causal flash forward on the same rows
    q, kc, vc = _inputs(2, 128, 8, 2, 128, 192)
    new = _run(q, kc, vc, [1, 1], [128, 128])
    old = ops.flash_attention(q, kc[:, :128].contiguous(),
                              vc[:, :128].contiguous(), causal=True)
    torch.testing.assert_close(new.float(), old.float(), **TOL)


def test_graph_replay_with_changing_lengths():
    from prime_amd import ops

    KT = ops.PREFILL_KEY_TILE
    q, kc, vc = _inputs(3, 40, 8, 2, 128, 320)
    lens, n_new = _i32([1, 1, 1]), _i32([1, 1, 1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ops.attn_prefill_ragged(q, kc, vc, lens, n_new, split_rows=2 * KT)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attn_prefill_ragged(q, kc, vc, lens, n_new, split_rows=2 * KT)
    for L, n in (([200, 1, 281], [40, 2, 40]), ([0, 129, 64], [40, 40, 0]),
                 ([77, 0, 320], [1, 3, 40])):
        lens.copy_(_i32(L))
        n_new.copy_(_i32(n))
        graph.replay()
        assert torch.equal(out.clone(), _run(q, kc, vc, L, n, split_rows=2 * KT))


def test_transposing_read_probe():
    from prime_amd import ops

    src = torch.randn(64, 64).to(DEV, dtype=torch.bfloat16)  # asymmetric
    assert torch.equal(ops.tr16_probe(src), src.t().contiguous())


@pytest.mark.parametrize("T", [4, 19])
def test_prefill_qkv_append(T):
    from prime_amd import ops

    B, H, Hkv, D, Smax, SENT = 4, 8, 2, 64, 64, 3.0
    cos, sin = ops.reference.rope_tables(D, 256, device=DEV)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D).to(DEV, dtype=torch.bfloat16)
    x = qkv.view(B, T, H + 2 * Hkv, D)
    kc = torch.full((B, Smax, Hkv, D), SENT, device=DEV, dtype=torch.bfloat16)
    vc = torch.full_like(kc, SENT)
    # slot 1 idle, slot 2 crosses Smax at t = 2, slot 3 has n_new < T
    pos, n_new = [5, -1, Smax - 2, 0], [T, T, T, T - 2]
    q = ops.prefill_qkv_append(qkv, cos, sin, kc, vc, _i32(pos), _i32(n_new),
                               H, Hkv)
    if T <= 8:
        kc2, vc2 = torch.full_like(kc, SENT), torch.full_like(kc, SENT)
        q2 = ops.decode_qkv_append_multi(qkv, cos, sin, kc2, vc2, _i32(pos),
                                         _i32(n_new), H, Hkv)
        assert torch.equal(q, q2) and torch.equal(kc, kc2) and torch.equal(vc, vc2)
        return
    keep = torch.ones(B, Smax, dtype=torch.bool, device=DEV)
    for b in range(B):
        for t in range(T):
            p = pos[b] + t
            if pos[b] < 0 or t >= n_new[b] or p >= Smax:
                assert (q[b, t] == 0).all()
                continue
            keep[b, p] = False
            xt = x[b:b + 1, t:t + 1]
            assert torch.equal(q[b, t], ops.apply_rope(
                xt[:, :, :H].contiguous(), cos, sin, pos_offset=p)[0, 0])
            assert torch.equal(kc[b, p], ops.apply_rope(
                xt[:, :, H:H + Hkv].contiguous(), cos, sin, pos_offset=p)[0, 0])
            assert torch.equal(vc[b, p], x[b, t, H + Hkv:])
    assert (kc[keep] == SENT).all() and (vc[keep] == SENT).all()


@pytest.mark.parametrize("H,Hkv,D", [(6, 2, 64), (8, 2, 96)])  # G = 3; D = 96
def test_unsupported_shapes_raise(H, Hkv, D):
    from prime_amd import ops
    from prime_amd.ops._lib import lib, ptr, stream_of

    q, kc, vc = _inputs(1, 16, H, Hkv, D, 256)
    one = _i32([1])
    with pytest.raises(NotImplementedError):
        ops.attn_prefill_ragged(q, kc, vc, _i32([5]), one)
    assert lib().prime_attn_prefill_ragged(
        stream_of(q), ptr(q), ptr(kc), ptr(vc), ptr(torch.empty_like(q)),
        ptr(None), ptr(one), ptr(one), 1, 16, H, Hkv, 256, D, 256,
        0.125) == 1  # hipErrorInvalidValue


def test_fp8_cache_raises():
    from prime_amd import ops

    q, kc, vc = _inputs(1, 16, 8, 2, 64, 256)
    cache = ops.kv_cache_fp8(1, 256, 2, 64, DEV)
    with pytest.raises(NotImplementedError):
        ops.attn_prefill_ragged(q, cache, cache, _i32([5]), _i32([1]))
    cos, sin = ops.reference.rope_tables(64, 256, device=DEV)
    with pytest.raises(NotImplementedError):
        ops.prefill_qkv_append(torch.zeros(1, 16, 12 * 64, device=DEV,
                                           dtype=torch.bfloat16), cos, sin,
                               cache, cache, _i32([0]), _i32([16]), 8, 2)


@torch.no_grad()
def test_model_chunked_prefill_matches_padded_prefill():
    from prime_amd.models import Llama
    from prime_amd.models.configs import get_config
    from prime_amd.models.generate import prefill_chunked

    torch.manual_seed(0)
    cfg = get_config("llama_150m", n_layers=2, n_heads=12, n_kv_heads=6)
    model = Llama(cfg).to(DEV, dtype=torch.bfloat16).eval()
    model.reset_rope(DEV)
    L = (5, 70, 133)
    g = torch.Generator().manual_seed(5)
    toks = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in L]
    m32 = Llama(cfg)  # fp32 CPU model with the same (bf16-valued) weights
    m32.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    ref = [m32.eval()(t[None])[0, -1] for t in toks]

    def caches(B):
        return [tuple(torch.zeros(B, 256, cfg.n_kv_heads, cfg.head_dim,
                                  device=DEV, dtype=torch.bfloat16)
                      for _ in range(2)) for _ in range(cfg.n_layers)]

    pad = torch.zeros(3, 192, dtype=torch.int64, device=DEV)
    for b, t in enumerate(toks):
        pad[b, :len(t)] = t.to(DEV)
    c_old, c_new = caches(3), caches(4)  # one padding slot
    old = model(pad, caches=c_old, pos=0)
    new = prefill_chunked(model, c_new, [t.tolist() for t in toks], 64)
    for b, n in enumerate(L):
        e_old = (old[b, n - 1].float().cpu() - ref[b]).abs().max().item()
        e_new = (new[b].float().cpu() - ref[b]).abs().max().item()
        print(f"L={n}: max abs err vs fp32 CPU model: padded flash prefill "
              f"{e_old:.4e}, chunked ragged prefill {e_new:.4e}")
        assert e_new <= 2 * e_old + 1e-3
        for i in range(2):  # layer-0 K and V rows
            assert torch.equal(c_new[0][i][b, :n], c_old[0][i][b, :n])
    assert (c_new[0][0][3] == 0).all()  # the idle slot wrote nothing
