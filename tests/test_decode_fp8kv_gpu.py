"""fp8 (e4m3) KV cache on the GPU: the append and store kernels bit-exact
against the row-wise fp8 oracle, the fp8 ragged decode attention against the
fp32 CPU reference on the dequantised cache (which sees exactly the stored
values, so the decode tolerance covers kernel error only), and the model /
generate_batch paths."""
import pytest
import torch

from tests import fp8kv_common as common
from tests import kernel_oracles as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(atol=3e-2, rtol=3e-2)  # the project's decode tolerance
SENT_BYTE = 0x55
SENT_SCALE = 7.0


def _bf(x):
    return x.to(DEV, dtype=torch.bfloat16)


def _lens(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _u8(t):
    return t.view(torch.uint8)


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(4321)


def _sentinel_cache(B, Smax, Hkv, D):
    from prime_amd import ops

    c = ops.kv_cache_fp8(B, Smax, Hkv, D, DEV)
    _u8(c.k).fill_(SENT_BYTE)
    _u8(c.v).fill_(SENT_BYTE)
    c.k_scale.fill_(SENT_SCALE)
    c.v_scale.fill_(SENT_SCALE)
    return c


def _assert_rows(bytes_, scale, x, what):
    """Stored bytes [.., D] / scales [..] of the bf16 vectors x [.., D]
    against the row-wise oracle: equal."""
    D = x.shape[-1]
    o = ko.oracle_fp8_rowwise(x.detach().cpu().reshape(-1, D), "e4m3")
    ko.assert_fp8(o, "e4m3", bytes_.reshape(-1, D),
                  sinv=scale.cpu().reshape(-1, 1), what=what)


def _untouched(cache, keep):
    """keep: bool [B, Smax] of rows that must still hold the sentinel."""
    for t in (cache.k, cache.v):
        assert (_u8(t)[keep] == SENT_BYTE).all()
    for t in (cache.k_scale, cache.v_scale):
        assert (t[keep] == SENT_SCALE).all()


# ------------------------------------------------------- quantising kernels
@pytest.mark.parametrize("D", [128, 64])
def test_decode_qkv_append_fp8(D):
    from prime_amd import ops

    B, H, Hkv, Smax, T = 3, 8, 2, 64, 256
    NH = H + 2 * Hkv
    cos, sin = ops.reference.rope_tables(D, T, device=DEV)
    qkv = ko.fp8_values((B, NH * D), 21).to(DEV)
    x = qkv.view(B, 1, NH, D)
    x[1, 0, H + Hkv] = 0  # an all-zero v head row

    def check(pos):
        c = _sentinel_cache(B, Smax, Hkv, D)
        q = ops.decode_qkv_append_fp8(qkv, cos, sin, c, _lens(pos), H, Hkv)
        kc = torch.zeros(B, Smax, Hkv, D, device=DEV, dtype=torch.bfloat16)
        q_bf = ops.decode_qkv_append(qkv, cos, sin, kc, torch.zeros_like(kc),
                                     _lens(pos), H, Hkv)
        torch.cuda.synchronize()
        assert torch.equal(q, q_bf)
        keep = torch.ones(B, Smax, dtype=torch.bool, device=DEV)
        for b, p in enumerate(pos):
            if not 0 <= p < Smax:
                assert (q[b] == 0).all()
                continue
            keep[b, p] = False
            wk = ops.apply_rope(x[b:b + 1, :, H:H + Hkv].contiguous(), cos, sin,
                                pos_offset=p)[0, 0]
            _assert_rows(_u8(c.k)[b, p], c.k_scale[b, p], wk, f"append k[{b}]")
            _assert_rows(_u8(c.v)[b, p], c.v_scale[b, p], x[b, 0, H + Hkv:],
                         f"append v[{b}]")
            # append and store agree: the same rows through the prefill store
            s = _sentinel_cache(1, Smax, Hkv, D)
            ops.kv_store_fp8(s, wk[None, None], x[b:b + 1, :, H + Hkv:], p)
            for ta, ts in zip(c, s):
                assert torch.equal(_u8(ta[b, p]), _u8(ts[0, p]))
        _untouched(c, keep)

    check([5, 0, 63])
    # idle and out-of-range slots; the out-of-range one is NOT the last slot,
    # so a missing guard would land in the next sequence's (checked) rows
    check([-1, Smax, 7])


@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("S,pos", [(1, 0), (1, 3), (64, 0), (64, 3), (70, 0), (70, 3)])
def test_kv_store_fp8(D, S, pos):
    from prime_amd import ops

    B, Bc, Hkv, Smax = 2, 4, 2, 128
    k = ko.fp8_values((B, S, Hkv, D), 31).to(DEV)
    v = ko.fp8_values((B, S, Hkv, D), 32).to(DEV)
    k[1, S // 2, 1] = 0  # an all-zero head row
    c = _sentinel_cache(Bc, Smax, Hkv, D)
    ops.kv_store_fp8(c, k, v, pos)
    torch.cuda.synchronize()
    _assert_rows(_u8(c.k)[:B, pos:pos + S], c.k_scale[:B, pos:pos + S], k, "store k")
    _assert_rows(_u8(c.v)[:B, pos:pos + S], c.v_scale[:B, pos:pos + S], v, "store v")
    keep = torch.ones(Bc, Smax, dtype=torch.bool, device=DEV)
    keep[:B, pos:pos + S] = False
    _untouched(c, keep)
    # a strided v (the model's view of the packed projection) and a view of
    # the leading cache slots give the same result
    c2 = _sentinel_cache(Bc, Smax, Hkv, D)
    kv = torch.cat([k, v], dim=2)
    ops.kv_store_fp8(ops.KVCacheFp8(*(t[:B] for t in c2)), kv[:, :, :Hkv],
                     kv[:, :, Hkv:], pos)
    for ta, tb in zip(c, c2):
        assert torch.equal(_u8(ta), _u8(tb))


def test_kv_store_fp8_rejects_bad_ranges():
    from prime_amd import ops
    from prime_amd.ops._lib import lib, ptr, stream_of

    B, S, Hkv, D, Smax = 2, 8, 2, 64, 16
    k = _bf(torch.randn(B, S, Hkv, D))
    c = _sentinel_cache(B, Smax, Hkv, D)

    def raw(S_, D_, pos):
        return lib().prime_kv_store_fp8(
            stream_of(k), ptr(k), ptr(k), ptr(c.k), ptr(c.v), ptr(c.k_scale),
            ptr(c.v_scale), B, S_, Hkv, D_, Smax, pos)

    assert raw(S, D, -1) != 0
    assert raw(S, D, Smax - S + 1) != 0
    assert raw(Smax + 1, D, 0) != 0
    assert raw(S, 32, 0) != 0
    for pos in (-1, Smax - S + 1):
        with pytest.raises(ValueError):
            ops.kv_store_fp8(c, k, k, pos)
    torch.cuda.synchronize()
    _untouched(c, torch.ones(B, Smax, dtype=torch.bool, device=DEV))


# ------------------------------------------------------- decode attention
def _inputs(B, H, Hkv, D, Smax):
    """q and an fp8 cache built by the store kernel from randn bf16."""
    from prime_amd import ops

    c = ops.kv_cache_fp8(B, Smax, Hkv, D, DEV)
    ops.kv_store_fp8(c, _bf(torch.randn(B, Smax, Hkv, D)),
                     _bf(torch.randn(B, Smax, Hkv, D)), 0)
    return _bf(torch.randn(B, H, D)), c


def _check_rows(got, q, cache, lens):
    """Every sequence against its own fp32 CPU reference on the dequantised
    rows [0, lens[b]); idle slots must be exactly zero."""
    from prime_amd import ops

    got = got.float().cpu()
    assert torch.isfinite(got).all()
    cpu = ops.KVCacheFp8(*(t.cpu() for t in cache))
    Smax = cpu.k.shape[1]
    for b, n in enumerate(lens):
        n = min(max(n, 0), Smax)
        if n == 0:
            assert (got[b] == 0).all()
            continue
        kd, vd = ops.kv_cache_dequant(ops.KVCacheFp8(*(t[b:b + 1, :n] for t in cpu)))
        want = ops.reference.attention(q[b:b + 1].float().cpu().unsqueeze(1),
                                       kd, vd, causal=False)[0, 0]
        torch.testing.assert_close(got[b], want, **TOL)


def test_every_e4m3_code_decodes_as_ocp():
    """Rows 0..3 of K and of V hold the bytes 0..255 (the two NaN codes
    replaced by 0). An fnuz decode reads every value at half its size and
    fails the tolerance."""
    from prime_amd import ops

    D, Smax = 64, 256
    codes = torch.arange(256, dtype=torch.uint8)
    codes[codes & 0x7F == 0x7F] = 0
    c = ops.kv_cache_fp8(1, Smax, 1, D, DEV)
    _u8(c.k)[0, :4, 0] = codes.view(4, D).to(DEV)
    _u8(c.v)[0, :4, 0] = codes.view(4, D).to(DEV)
    c.k_scale.fill_(2.0 ** -9)
    c.v_scale.fill_(2.0 ** -4)
    q = _bf(torch.randn(1, 1, D))
    got = ops.attn_decode_ragged_fp8(q, c, _lens([4]))
    kd, vd = ops.kv_cache_dequant(ops.KVCacheFp8(*(t.cpu()[:, :4] for t in c)))
    assert vd.abs().max() == 448 * 2.0 ** -4  # the OCP range on the CPU side
    want = ops.reference.attention(q.float().cpu().unsqueeze(1), kd, vd,
                                   causal=False)[0, 0]
    # the test bites: half the V scale alone (no change of the weights) is
    # already outside TOL
    assert (0.5 * want.abs() > TOL["atol"] + TOL["rtol"] * want.abs()).any()
    torch.testing.assert_close(got.float().cpu()[0], want, **TOL)


def test_mixed_lengths():
    from prime_amd import ops

    lens = [300, 1, 257]
    q, c = _inputs(3, 8, 2, 128, 512)
    got = ops.attn_decode_ragged_fp8(q, c, _lens(lens))
    assert got.shape == q.shape and got.dtype == torch.bfloat16
    _check_rows(got, q, c, lens)


@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 1)])  # D=64: G=1 and G=8
@pytest.mark.parametrize("split_chunks", [None, 2])
def test_internal_boundaries(H, Hkv, split_chunks):
    """One below / at / one above the softmax chunk and the rows-per-split
    boundary (and their multiples below Smax), plus lens = Smax, with the
    default split and with a split of two chunks."""
    from prime_amd import ops

    C = ops.DECODE_RAGGED_CHUNK
    D, Smax = 64, 4 * C + 64
    n_cu = torch.cuda.get_device_properties(DEV).multi_processor_count
    edges = {e + d for e in (C, 2 * C, 4 * C) for d in (-1, 0, 1)} | {Smax}
    kw = {} if split_chunks is None else {"split_rows": split_chunks * C}
    for _ in range(2):  # the default split depends on B = len(edges)
        rows = kw.get("split_rows") or ops.decode_ragged_split(
            len(edges), Hkv, Smax, n_cu)
        edges |= {rows + d for d in (-1, 0, 1)}
    edges = sorted(edges)
    B = len(edges)
    assert rows == (kw.get("split_rows")
                    or ops.decode_ragged_split(B, Hkv, Smax, n_cu))
    assert -(-Smax // rows) >= 2  # at least two live splits at lens = Smax
    assert max(edges) == Smax
    q, c = _inputs(B, H, Hkv, D, Smax)
    got = ops.attn_decode_ragged_fp8(q, c, _lens(edges), **kw)
    _check_rows(got, q, c, edges)


@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 128), (16, 4, 64)])  # G=2, G=4
def test_other_group_sizes(H, Hkv, D):
    from prime_amd import ops

    lens = [511, 0, 256, 3]
    q, c = _inputs(4, H, Hkv, D, 512)
    _check_rows(ops.attn_decode_ragged_fp8(q, c, _lens(lens)), q, c, lens)


def test_rows_beyond_length_are_not_read():
    from prime_amd import ops

    lens = [300, 0, 257, 1]
    q, c = _inputs(4, 8, 2, 128, 512)
    for b, n in enumerate(lens):
        _u8(c.k)[b, n:] = 0x7F  # e4m3 NaN
        _u8(c.v)[b, n:] = 0x7F
        c.k_scale[b, n:] = float("nan")
        c.v_scale[b, n:] = float("nan")
    got = ops.attn_decode_ragged_fp8(q, c, _lens(lens))
    assert (got[1] == 0).all()  # idle slot, whole cache NaN
    _check_rows(got, q, c, lens)


def test_length_is_clamped_and_result_reproducible():
    from prime_amd import ops

    Smax = 512
    q, c = _inputs(3, 8, 2, 128, Smax)
    a = ops.attn_decode_ragged_fp8(q, c, _lens([300, Smax + 1000, -5]))
    b = ops.attn_decode_ragged_fp8(q, c, _lens([300, Smax, 0]))
    assert torch.equal(a, b)
    _check_rows(a, q, c, [300, Smax, 0])


def test_unsupported_shapes_raise():
    from prime_amd import ops
    from prime_amd.ops._lib import lib, ptr, stream_of

    q, c = _inputs(1, 6, 2, 64, 256)  # G = 3
    with pytest.raises(NotImplementedError):
        ops.attn_decode_ragged_fp8(q, c, _lens([5]))
    ws = torch.empty(2 * 3 * 66, device=DEV)
    o = torch.empty_like(q)
    rc = lib().prime_attn_decode_ragged_fp8(
        stream_of(q), ptr(q), ptr(c.k), ptr(c.v), ptr(c.k_scale),
        ptr(c.v_scale), ptr(o), ptr(ws), ptr(_lens([5])), 1, 6, 2, 256, 64,
        256, 0.125)
    assert rc != 0  # hipErrorInvalidValue, nothing launched


def test_graph_replay_with_changing_lengths():
    from prime_amd import ops

    q, c = _inputs(3, 8, 2, 128, 1024)
    lens = _lens([1, 1, 1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ops.attn_decode_ragged_fp8(q, c, lens)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attn_decode_ragged_fp8(q, c, lens)
    for case in ([300, 1, 1024], [0, 513, 256], [77, 0, 0]):
        lens.copy_(_lens(case))
        graph.replay()
        got = out.clone()
        eager = ops.attn_decode_ragged_fp8(q, c, _lens(case))
        assert torch.equal(got, eager)
        _check_rows(got, q, c, case)


# ------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def models():
    """(bf16 GPU model, fp32 CPU model) holding the same bf16-valued weights."""
    from prime_amd.models import Llama

    m32 = common.build_cpu_model()
    m = Llama(m32.cfg)
    m.load_state_dict(m32.state_dict())
    m = m.to(DEV, dtype=torch.bfloat16)
    m.reset_rope(DEV)
    m.eval()
    return m, m32


@torch.no_grad()
def test_fp8_step_error_is_bounded_by_the_quantisation_effect(models):
    """Error of the new token's hidden state against the fp32 CPU model:
    e_fp8 (fp8 cache) <= 2 e_bf16 (bf16 ragged path) + 2 e_q + 1e-3, with e_q
    the pure quantisation effect measured on the CPU (common.E_Q_MEASURED).
    The factor on e_bf16 is the existing ragged model test's; the factor on
    e_q allows for bf16 inputs moving a value into the next e4m3 bin."""
    model, m32 = models
    cfg = model.cfg
    L0 = common.L0
    toks = common.step_tokens(cfg)
    ref = [m32(t[None])[0, -1] for t in toks]

    c = [tuple(torch.zeros(3, common.SMAX, cfg.n_kv_heads, cfg.head_dim,
                           device=DEV, dtype=torch.bfloat16) for _ in range(2))
         for _ in range(cfg.n_layers)]
    pad = torch.zeros(3, 64, dtype=torch.int64, device=DEV)
    for b, (t, n) in enumerate(zip(toks, L0)):
        pad[b, :n] = t[:n].to(DEV)
    model(pad, caches=c, pos=0)
    cur = torch.stack([t[-1:] for t in toks]).to(DEV)
    sp = {"pos": _lens(L0), "lens": _lens([n + 1 for n in L0])}
    bf = model(cur, caches=c, seq_pos=sp)[:, 0]
    f8 = common.fp8_step(model, toks, DEV)

    fails = []
    for b in range(3):
        e_bf16 = (bf[b].float().cpu() - ref[b]).abs().max().item()
        e_fp8 = (f8[b].float().cpu() - ref[b]).abs().max().item()
        e_q = common.E_Q_MEASURED[b]
        bound = 2 * e_bf16 + 2 * e_q + 1e-3
        print(f"L0={L0[b]}: max abs err vs fp32 CPU model: e_bf16 {e_bf16:.4e}, "
              f"e_fp8 {e_fp8:.4e}, e_q {e_q:.4e}, bound {bound:.4e}")
        if not e_fp8 <= bound:
            fails.append(b)
    assert not fails


def _prompts(cfg, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist()
            for n in lengths]


def test_generate_batch_fp8(models):
    from prime_amd.models.generate import generate_batch

    model, _ = models
    cfg = model.cfg
    ps = _prompts(cfg, (5, 17, 33), 6)
    new = [12, 3, 8]
    eager = generate_batch(model, ps, new, use_graph=False, kv_dtype="fp8")
    graphed = generate_batch(model, ps, new, use_graph=True, kv_dtype="fp8")
    assert [len(o) for o in eager] == new
    assert graphed == eager
    bf = generate_batch(model, ps, new, use_graph=True)
    assert [o[0] for o in bf] == [o[0] for o in eager]
    ragged = {k: v for k, v in model._decode_sessions.items() if k[0] == "ragged"}
    assert sorted(k[-1] for k in ragged) == ["bf16", "fp8"]  # both survive
    key8, = (k for k in ragged if k[-1] == "fp8")
    key16, = (k for k in ragged if k[-1] == "bf16")
    assert key8[:-1] == key16[:-1] and key8[1] == 4
    from prime_amd import ops

    assert all(isinstance(c, ops.KVCacheFp8) for c in ragged[key8]["caches"])
    assert not any(isinstance(c, ops.KVCacheFp8) for c in ragged[key16]["caches"])
    graph = ragged[key8]["graph"]

    # another set of prompts in the same bucket: same captured graph
    ps2 = _prompts(cfg, (40, 2, 9), 7)
    new2 = [5, 9, 4]
    eager2 = generate_batch(model, ps2, new2, use_graph=False, kv_dtype="fp8")
    graphed2 = generate_batch(model, ps2, new2, use_graph=True, kv_dtype="fp8")
    assert graphed2 == eager2 and [len(o) for o in eager2] == new2
    assert model._decode_sessions[key8]["graph"] is graph
    assert set(k for k in model._decode_sessions if k[0] == "ragged") == {key8, key16}
