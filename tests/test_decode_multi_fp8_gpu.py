"""Multi-token ragged decode over the fp8 KV cache on the GPU. The reference is
ops.reference.attention in fp32 on the CPU over the dequantised cache: it sees
exactly the stored values, so the decode tolerance covers kernel error only."""
import pytest
import torch

from tests import kernel_oracles as ko
from tests.test_decode_fp8kv_gpu import _assert_rows, _sentinel_cache, _u8, _untouched
from tests.test_decode_multi_gpu import DEV, TOL, _i32, _live, _seed, model  # noqa: F401

pytestmark = pytest.mark.gpu


def _inputs(B, T, H, Hkv, D, Smax):
    """q and an fp8 cache of randn rows, each (b, row, kv head) vector times
    its own factor (K 2^-2..2^1, V 2^-3..2^3): scales differ by row and head."""
    from prime_amd import ops

    def rows(lo, hi):
        f = 2.0 ** (lo + (hi - lo) * torch.rand(B, Smax, Hkv, 1))
        return (torch.randn(B, Smax, Hkv, D) * f).to(DEV, dtype=torch.bfloat16)

    c = ops.kv_cache_fp8(B, Smax, Hkv, D, DEV)
    ops.kv_store_fp8(c, rows(-2, 1), rows(-3, 3), 0)
    return torch.randn(B, T, H, D).to(DEV, dtype=torch.bfloat16), c


def _outside(a, want):
    return ((a - want).abs() > TOL["atol"] + TOL["rtol"] * want.abs()).any()


def _run(q, c, lens, n_new, poison=False, bites=False, **kw):
    """The op against the reference per (b, t) on rows [0, L0 + t); dead rows
    exactly zero. poison: NaN bytes and scales wherever the kernel may not
    load. bites: the reference with k_scale / v_scale rolled by one row is
    itself outside the tolerance for some checked query."""
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
    got = ops.attn_decode_ragged_multi_fp8(q, c, _i32(lens), _i32(n_new), **kw)
    assert got.shape == q.shape and got.dtype == torch.bfloat16
    out, qf = got.float().cpu(), q.float().cpu()
    assert torch.isfinite(out).all()
    cpu = ops.KVCacheFp8(*(t.cpu() for t in c))
    rolled = [cpu._replace(k_scale=cpu.k_scale.roll(1, 1)),
              cpu._replace(v_scale=cpu.v_scale.roll(1, 1))]
    moved = [False, False]

    def ref(cache, b, t, rows):
        kd, vd = ops.kv_cache_dequant(
            ops.KVCacheFp8(*(x[b:b + 1, :rows] for x in cache)))
        return ops.reference.attention(qf[b:b + 1, t:t + 1], kd, vd,
                                       causal=False)[0, 0]

    for b, (L, n) in enumerate(zip(lens, n_new)):
        L0, n = _live(L, n, T, Smax)
        assert (out[b, n:] == 0).all()
        for t in range(n):
            want = ref(cpu, b, t, L0 + t)
            torch.testing.assert_close(out[b, t], want, **TOL)
            if bites:
                moved = [m or bool(_outside(ref(r, b, t, L0 + t), want))
                         for m, r in zip(moved, rolled)]
    assert not bites or all(moved)  # the test bites: a scale of the wrong row fails
    return got


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T,H,Hkv", [(4, 4, 4), (3, 8, 2), (2, 8, 1), (5, 8, 1),
                                     (8, 8, 1)])  # M = 4, 12, 16, 40, 64
def test_row_tiling(T, H, Hkv, D):
    from prime_amd import ops

    C = ops.DECODE_MULTI_CHUNK
    Smax = 2 * C + 64
    _run(*_inputs(4, T, H, Hkv, D, Smax), [1, C - 1, C, Smax - T + 1],
         [T, T, T - 1, T], bites=True)


def test_every_e4m3_code_through_both_byte_paths():
    """Rows 0..3 of K (register path) and V (LDS path) hold the bytes 0..255."""
    from prime_amd import ops

    D, Smax = 64, 256
    codes = torch.arange(256, dtype=torch.uint8)
    codes[codes & 0x7F == 0x7F] = 0
    c = ops.kv_cache_fp8(1, Smax, 1, D, DEV)
    _u8(c.k)[0, :4, 0] = codes.view(4, D).to(DEV)
    _u8(c.v)[0, :4, 0] = codes.view(4, D).to(DEV)
    c.k_scale.fill_(2.0 ** -9)
    c.v_scale.fill_(2.0 ** -4)
    q = torch.randn(1, 2, 1, D).to(DEV, dtype=torch.bfloat16)
    _run(q, c, [4], [1])
    kd, vd = ops.kv_cache_dequant(ops.KVCacheFp8(*(t.cpu()[:, :4] for t in c)))
    assert vd.abs().max() == 448 * 2.0 ** -4  # the OCP range on the CPU side
    want = ops.reference.attention(q.float().cpu()[:, :1], kd, vd, causal=False)
    # the test bites: half the V scale alone is already outside TOL
    assert _outside(0.5 * want, want)


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


def test_dead_rows_and_scales_are_not_read():
    # NaN bytes and scales at and beyond L0 + n - 1; slot 1 idle, slot 2
    # n_new = 0 (whole cache NaN), slot 3 one live row of four
    _run(*_inputs(4, 4, 8, 2, 128, 512), [300, 0, 257, 130], [4, 4, 0, 1],
         poison=True)


def test_clamp_agreement_and_reproducibility():
    from prime_amd import ops
    from prime_amd.ops._lib import lib

    assert lib().prime_decode_multi_chunk() == ops.DECODE_MULTI_CHUNK
    T, Smax = 4, 512
    q, c = _inputs(3, T, 8, 2, 128, Smax)
    a = ops.attn_decode_ragged_multi_fp8(q, c, _i32([Smax + 1000, 300, -5]),
                                         _i32([T, T + 5, T]))
    b = _run(q, c, [Smax, 300, 0], [1, T, 0])
    assert torch.equal(a, b)
    assert torch.equal(b, ops.attn_decode_ragged_multi_fp8(
        q, c, _i32([Smax, 300, 0]), _i32([1, T, 0])))
    for D, lens in ((128, [300, 0, 512]), (64, [129, 1, 77])):  # T = 1
        q, c = _inputs(3, 1, 8, 2, D, Smax)
        one = _run(q, c, lens, [int(n > 0) for n in lens])
        old = ops.attn_decode_ragged_fp8(q[:, 0], c, _i32(lens))
        torch.testing.assert_close(one[:, 0].float(), old.float(), **TOL)


def test_graph_replay_with_changing_lengths():
    from prime_amd import ops

    q, c = _inputs(3, 4, 8, 2, 128, 1024)
    lens, n_new = _i32([1, 1, 1]), _i32([1, 1, 1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ops.attn_decode_ragged_multi_fp8(q, c, lens, n_new)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attn_decode_ragged_multi_fp8(q, c, lens, n_new)
    for L, n in (([300, 1, 1021], [4, 2, 4]), ([0, 513, 256], [4, 4, 0]),
                 ([77, 0, 1024], [1, 3, 4])):
        lens.copy_(_i32(L))
        n_new.copy_(_i32(n))
        graph.replay()
        assert torch.equal(out.clone(), _run(q, c, L, n))


@pytest.mark.parametrize("T,H,Hkv", [(2, 6, 2), (9, 8, 1)])  # G = 3; T*G > 64
def test_unsupported_shapes_raise(T, H, Hkv):
    from prime_amd import ops
    from prime_amd.ops._lib import lib, ptr, stream_of

    q, c = _inputs(1, T, H, Hkv, 64, 256)
    one = _i32([1])
    with pytest.raises(NotImplementedError):
        ops.attn_decode_ragged_multi_fp8(q, c, _i32([5]), one)
    ws = torch.empty(2 * Hkv * T * H * 66, device=DEV)
    assert lib().prime_attn_decode_ragged_multi_fp8(
        stream_of(q), ptr(q), ptr(c.k), ptr(c.v), ptr(c.k_scale),
        ptr(c.v_scale), ptr(torch.empty_like(q)), ptr(ws), ptr(one), ptr(one),
        1, T, H, Hkv, 256, 64, 128, 0.125) != 0


@pytest.mark.parametrize("D", [128, 64])
def test_decode_qkv_append_multi_fp8(D):
    from prime_amd import ops

    B, T, H, Hkv, Smax = 4, 3, 8, 2, 64
    NH = H + 2 * Hkv
    cos, sin = ops.reference.rope_tables(D, 256, device=DEV)
    qkv = ko.fp8_values((B, T, NH * D), 41).to(DEV)
    x = qkv.view(B, T, NH, D)
    x[0, 1, H + Hkv] = 0  # an all-zero v head row

    # slot 1 idle, slot 2 crosses Smax at t = 2 (not the last slot), slot 3
    # has n_new < T
    pos, n_new = [5, -1, Smax - 2, 0], [3, 3, 3, 2]
    c, one = (_sentinel_cache(B, Smax, Hkv, D) for _ in range(2))  # 0x55, 7.0
    q = ops.decode_qkv_append_multi_fp8(qkv, cos, sin, c, _i32(pos),
                                        _i32(n_new), H, Hkv)
    kc = torch.zeros(B, Smax, Hkv, D, device=DEV, dtype=torch.bfloat16)
    assert torch.equal(q, ops.decode_qkv_append_multi(
        qkv, cos, sin, kc, torch.zeros_like(kc), _i32(pos), _i32(n_new), H, Hkv))
    keep = torch.ones(B, Smax, dtype=torch.bool, device=DEV)
    for t in range(T):  # the same rows through the single-token kernel
        live = [p >= 0 and t < n and p + t < Smax for p, n in zip(pos, n_new)]
        ops.decode_qkv_append_fp8(
            qkv[:, t].contiguous(), cos, sin, one,
            _i32([p + t if ok else -1 for p, ok in zip(pos, live)]), H, Hkv)
        for b in range(B):
            if not live[b]:
                assert (q[b, t] == 0).all()
                continue
            p = pos[b] + t
            keep[b, p] = False
            wk = ops.apply_rope(x[b:b + 1, t:t + 1, H:H + Hkv].contiguous(),
                                cos, sin, pos_offset=p)[0, 0]
            _assert_rows(_u8(c.k)[b, p], c.k_scale[b, p], wk, f"k[{b},{t}]")
            _assert_rows(_u8(c.v)[b, p], c.v_scale[b, p], x[b, t, H + Hkv:],
                         f"v[{b},{t}]")
    for ta, tb in zip(c, one):
        assert torch.equal(_u8(ta), _u8(tb))
    _untouched(c, keep)


@torch.no_grad()
def test_multi_step_matches_token_by_token_path(model):
    """The bf16 test of the same name and its rule, fp8 caches on both sides."""
    from prime_amd import ops
    from prime_amd.models import Llama

    cfg, T, L0, n_new = model.cfg, 4, [5, 33, 60], [4, 2, 4]
    g = torch.Generator().manual_seed(5)
    toks = [torch.randint(0, cfg.vocab_size, (n + T,), generator=g) for n in L0]
    m32 = Llama(cfg)  # fp32 CPU model with the same (bf16-valued) weights
    m32.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    ref = [m32.eval()(t[None])[0, n:] for t, n in zip(toks, L0)]

    def prefilled():
        c = [ops.kv_cache_fp8(3, 128, cfg.n_kv_heads, cfg.head_dim, DEV)
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
                  f"token fp8 path {e_old:.4e}, multi-token fp8 path {e_new:.4e}")
            assert e_new <= 2 * e_old + 1e-3


def test_generate_batch_lookahead_fp8_graphed_matches_eager(model):
    from prime_amd.models.generate import generate_batch

    ps = [[7, 8, 9] * 5, [3, 4] * 8 + [3], list(range(20, 37))]
    new = [16, 9, 12]
    # a graphed bf16 session of the same shape first: fp8 must not pick it up
    generate_batch(model, ps, new, use_graph=True, lookahead=3)
    eager = generate_batch(model, ps, new, use_graph=False, lookahead=3,
                           kv_dtype="fp8")
    graphed = generate_batch(model, ps, new, use_graph=True, lookahead=3,
                             kv_dtype="fp8")
    assert graphed == eager and [len(o) for o in eager] == new
