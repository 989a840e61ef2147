"""Multi-token ragged decode on the GPU: attn_decode_ragged_multi and
decode_qkv_append_multi against fp32 CPU references, then the model and
generate_batch(lookahead=...) paths."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(atol=3e-2, rtol=3e-2)  # the decode tolerance of test_decode_ragged_gpu


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(1234)


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
    got = ops.attn_decode_ragged_multi(q, kc, vc, _i32(lens), _i32(n_new), **kw)
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
@pytest.mark.parametrize("T,H,Hkv", [(4, 4, 4), (3, 8, 2), (2, 8, 1), (5, 8, 1),
                                     (8, 8, 1)])  # M = 4, 12, 16, 40, 64
def test_row_tiling(T, H, Hkv, D):
    from prime_amd import ops

    C = ops.DECODE_MULTI_CHUNK
    Smax = 2 * C + 64
    _run(*_inputs(4, T, H, Hkv, D, Smax), [1, C - 1, C, Smax - T + 1],
         [T, T, T - 1, T])


@pytest.mark.parametrize("split_rows", [None, 2])
def test_chunk_and_split_boundaries(split_rows):
    from prime_amd import ops

    C, T, Smax = ops.DECODE_MULTI_CHUNK, 4, 4 * ops.DECODE_MULTI_CHUNK + 64
    n_cu = torch.cuda.get_device_properties(DEV).multi_processor_count
    kw = {} if split_rows is None else {"split_rows": split_rows * C}
    rows = kw.get("split_rows") or ops.decode_ragged_split(17, 1, Smax, n_cu)
    lens = sorted({e + d for e in (C, 2 * C, rows) for d in (-T, -1, 0, 1)}
                  | {Smax - T + 1})
    assert kw or rows == ops.decode_ragged_split(len(lens), 1, Smax, n_cu)
    assert -(-Smax // rows) >= 2
    _run(*_inputs(len(lens), T, 8, 1, 64, Smax), lens, [T] * len(lens), **kw)


def test_dead_rows_are_not_read():
    # NaN at and beyond L0 + n - 1; slot 1 idle, slot 2 n_new = 0 (whole
    # caches NaN), slot 3 one live row of four
    _run(*_inputs(4, 4, 8, 2, 128, 512), [300, 0, 257, 130], [4, 4, 0, 1],
         poison=True)


def test_clamp_agreement_and_reproducibility():
    from prime_amd import ops
    from prime_amd.ops._lib import lib

    assert lib().prime_decode_multi_chunk() == ops.DECODE_MULTI_CHUNK
    T, Smax = 4, 512
    q, kc, vc = _inputs(3, T, 8, 2, 128, Smax)
    a = ops.attn_decode_ragged_multi(q, kc, vc, _i32([Smax + 1000, 300, -5]),
                                     _i32([T, T + 5, T]))
    b = _run(q, kc, vc, [Smax, 300, 0], [1, T, 0])
    assert torch.equal(a, b)
    assert torch.equal(b, ops.attn_decode_ragged_multi(
        q, kc, vc, _i32([Smax, 300, 0]), _i32([1, T, 0])))
    for D, lens in ((128, [300, 0, 512]), (64, [129, 1, 77])):  # T = 1
        q, kc, vc = _inputs(3, 1, 8, 2, D, Smax)
        one = _run(q, kc, vc, lens, [int(n > 0) for n in lens])
        old = ops.attn_decode_ragged(q[:, 0], kc, vc, _i32(lens))
        torch.testing.assert_close(one[:, 0].float(), old.float(), **TOL)


def test_graph_replay_with_changing_lengths():
    from prime_amd import ops

    q, kc, vc = _inputs(3, 4, 8, 2, 128, 1024)
    lens, n_new = _i32([1, 1, 1]), _i32([1, 1, 1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ops.attn_decode_ragged_multi(q, kc, vc, lens, n_new)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attn_decode_ragged_multi(q, kc, vc, lens, n_new)
    for L, n in (([300, 1, 1021], [4, 2, 4]), ([0, 513, 256], [4, 4, 0]),
                 ([77, 0, 1024], [1, 3, 4])):
        lens.copy_(_i32(L))
        n_new.copy_(_i32(n))
        graph.replay()
        assert torch.equal(out.clone(), _run(q, kc, vc, L, n))


@pytest.mark.parametrize("T,H,Hkv", [(2, 6, 2), (9, 8, 1)])  # G = 3; T*G > 64
def test_unsupported_shapes_raise(T, H, Hkv):
    from prime_amd import ops
    from prime_amd.ops._lib import lib, ptr, stream_of

    q, kc, vc = _inputs(1, T, H, Hkv, 64, 256)
    one = _i32([1])
    with pytest.raises(NotImplementedError):
        ops.attn_decode_ragged_multi(q, kc, vc, _i32([5]), one)
    ws = torch.empty(2 * Hkv * T * H * 66, device=DEV)
    assert lib().prime_attn_decode_ragged_multi(
        stream_of(q), ptr(q), ptr(kc), ptr(vc), ptr(torch.empty_like(q)),
        ptr(ws), ptr(one), ptr(one), 1, T, H, Hkv, 256, 64, 128, 0.125) != 0


@pytest.mark.parametrize("D", [128, 64])
def test_decode_qkv_append_multi(D):
    from prime_amd import ops

    B, T, H, Hkv, Smax, SENT = 4, 3, 8, 2, 64, 3.0
    cos, sin = ops.reference.rope_tables(D, 256, device=DEV)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D).to(DEV, dtype=torch.bfloat16)
    x = qkv.view(B, T, H + 2 * Hkv, D)
    kc = torch.full((B, Smax, Hkv, D), SENT, device=DEV, dtype=torch.bfloat16)
    vc = torch.full_like(kc, SENT)
    # slot 1 idle, slot 2 crosses Smax at t = 2 (not the last slot), slot 3
    # has n_new < T
    pos, n_new = [5, -1, Smax - 2, 0], [3, 3, 3, 2]
    q = ops.decode_qkv_append_multi(qkv, cos, sin, kc, vc, _i32(pos),
                                    _i32(n_new), H, Hkv)
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


# ------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def model():
    from prime_amd.models import Llama
    from prime_amd.models.configs import get_config

    torch.manual_seed(0)
    cfg = get_config("llama_150m", n_layers=2, n_heads=12, n_kv_heads=6)
    m = Llama(cfg).to(DEV, dtype=torch.bfloat16)
    m.reset_rope(DEV)
    return m.eval()


@torch.no_grad()
def test_multi_step_matches_token_by_token_path(model):
    from prime_amd.models import Llama

    cfg, T, L0, n_new = model.cfg, 4, [5, 33, 60], [4, 2, 4]
    g = torch.Generator().manual_seed(5)
    toks = [torch.randint(0, cfg.vocab_size, (n + T,), generator=g) for n in L0]
    m32 = Llama(cfg)  # fp32 CPU model with the same (bf16-valued) weights
    m32.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    ref = [m32.eval()(t[None])[0, n:] for t, n in zip(toks, L0)]

    def prefilled():
        c = [tuple(torch.zeros(3, 128, cfg.n_kv_heads, cfg.head_dim, device=DEV,
                               dtype=torch.bfloat16) for _ in range(2))
             for _ in range(cfg.n_layers)]
        pad = torch.zeros(3, 64, dtype=torch.int64, device=DEV)
        for b, (t, n) in enumerate(zip(toks, L0)):
            pad[b, :n] = t[:n].to(DEV)
        model(pad, caches=c, pos=0)
        return c

    cur = torch.stack([t[n:] for t, n in zip(toks, L0)]).to(DEV)  # [3, T]
    c = prefilled()
    old = [model(cur[:, t:t + 1], caches=c, seq_pos={
        "pos": _i32([n + t for n in L0]),
        "lens": _i32([n + t + 1 for n in L0])})[:, 0] for t in range(T)]
    new = model(cur, caches=prefilled(), seq_pos={
        "pos": _i32(L0), "lens": _i32([n + 1 for n in L0]), "n_new": _i32(n_new)})
    for b in range(3):
        for t in range(n_new[b]):
            e_old = (old[t][b].float().cpu() - ref[b][t]).abs().max().item()
            e_new = (new[b, t].float().cpu() - ref[b][t]).abs().max().item()
            print(f"L0={L0[b]} t={t}: max abs err vs fp32 CPU model: single-"
                  f"token path {e_old:.4e}, multi-token path {e_new:.4e}")
            assert e_new <= 2 * e_old + 1e-3


def test_generate_batch_lookahead_graphed_matches_eager(model):
    from prime_amd.models.generate import generate_batch

    ps = [[7, 8, 9] * 5, [3, 4] * 8 + [3], list(range(20, 37))]
    new = [16, 9, 12]
    eager = generate_batch(model, ps, new, use_graph=False, lookahead=3)
    graphed = generate_batch(model, ps, new, use_graph=True, lookahead=3)
    assert graphed == eager and [len(o) for o in eager] == new
    plain = generate_batch(model, ps, new, use_graph=False)
    same = sum(a == b for o, p in zip(eager, plain) for a, b in zip(o, p))
    print(f"lookahead=3 vs lookahead=0: {same}/{sum(new)} tokens agree")
