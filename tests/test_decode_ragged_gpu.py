"""Ragged batched decoding on the GPU: the attn_decode_ragged and
decode_qkv_append kernels against the fp32 CPU reference, and the model /
generate_batch paths against the existing single-position decode."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(atol=3e-2, rtol=3e-2)  # as test_attn_decode_vs_reference


def _bf(x):
    return x.to(DEV, dtype=torch.bfloat16)


def _lens(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(4321)


def _inputs(B, H, Hkv, D, Smax):
    return (_bf(torch.randn(B, H, D)), _bf(torch.randn(B, Smax, Hkv, D)),
            _bf(torch.randn(B, Smax, Hkv, D)))


def _check_rows(got, q, kc, vc, lens):
    """Every sequence against its own fp32 CPU reference on kc[b, :lens[b]];
    idle slots must be exactly zero."""
    from prime_amd import ops

    got = got.float().cpu()
    assert torch.isfinite(got).all()
    Smax = kc.shape[1]
    for b, n in enumerate(lens):
        n = min(max(n, 0), Smax)
        if n == 0:
            assert (got[b] == 0).all()
            continue
        want = ops.reference.attention(
            q[b:b + 1].float().cpu().unsqueeze(1), kc[b:b + 1, :n].float().cpu(),
            vc[b:b + 1, :n].float().cpu(), causal=False)[0, 0]
        torch.testing.assert_close(got[b], want, **TOL)


def test_mixed_lengths():
    from prime_amd import ops

    lens = [300, 1, 257]
    q, kc, vc = _inputs(3, 8, 2, 128, 512)
    got = ops.attn_decode_ragged(q, kc, vc, _lens(lens))
    assert got.shape == q.shape and got.dtype == torch.bfloat16
    _check_rows(got, q, kc, vc, lens)


@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 1)])  # D=64: G=1 and G=8
@pytest.mark.parametrize("split_chunks", [None, 2])
def test_internal_boundaries(H, Hkv, split_chunks):
    """One below / at / one above the softmax chunk and the rows-per-split
    boundary (and their multiples below Smax), plus lens = Smax, with the
    default split and with a split of two chunks so the two boundaries
    differ."""
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
    q, kc, vc = _inputs(B, H, Hkv, D, Smax)
    got = ops.attn_decode_ragged(q, kc, vc, _lens(edges), **kw)
    _check_rows(got, q, kc, vc, edges)


def test_chunk_constant_matches_kernel():
    from prime_amd import ops
    from prime_amd.ops._lib import lib

    assert lib().prime_decode_ragged_chunk() == ops.DECODE_RAGGED_CHUNK


def test_rows_beyond_length_are_not_read():
    from prime_amd import ops

    lens = [300, 0, 257, 1]
    q, kc, vc = _inputs(4, 8, 2, 128, 512)
    for b, n in enumerate(lens):
        kc[b, n:] = float("nan")
        vc[b, n:] = float("nan")
    got = ops.attn_decode_ragged(q, kc, vc, _lens(lens))
    assert (got[1] == 0).all()  # idle slot, whole cache NaN
    _check_rows(got, q, kc, vc, lens)


def test_length_is_clamped():
    from prime_amd import ops

    Smax = 512
    q, kc, vc = _inputs(3, 8, 2, 128, Smax)
    a = ops.attn_decode_ragged(q, kc, vc, _lens([300, Smax + 1000, -5]))
    b = ops.attn_decode_ragged(q, kc, vc, _lens([300, Smax, 0]))
    assert torch.equal(a, b)
    _check_rows(a, q, kc, vc, [300, Smax, 0])


def test_agrees_with_attn_decode_and_is_reproducible():
    from prime_amd import ops

    for (B, H, Hkv, D, Smax, L) in ((2, 8, 2, 128, 512, 300),
                                    (1, 4, 2, 64, 768, 700)):
        q, kc, vc = _inputs(B, H, Hkv, D, Smax)
        lens = _lens([L] * B)
        a = ops.attn_decode_ragged(q, kc, vc, lens)
        old = ops.attn_decode(q, kc, vc, length=L)
        torch.testing.assert_close(a.float(), old.float(), **TOL)
        assert torch.equal(a, ops.attn_decode_ragged(q, kc, vc, lens))


def test_unsupported_shapes_raise():
    from prime_amd import ops
    from prime_amd.ops._lib import lib, ptr, stream_of

    q, kc, vc = _inputs(1, 6, 2, 64, 256)  # G = 3
    with pytest.raises(NotImplementedError):
        ops.attn_decode_ragged(q, kc, vc, _lens([5]))
    ws = torch.empty(2 * 3 * 66, device=DEV)
    o = torch.empty_like(q)
    rc = lib().prime_attn_decode_ragged(
        stream_of(q), ptr(q), ptr(kc), ptr(vc), ptr(o), ptr(ws), ptr(_lens([5])),
        1, 6, 2, 256, 64, 256, 0.125)
    assert rc != 0  # hipErrorInvalidValue, nothing launched


def test_graph_replay_with_changing_lengths():
    from prime_amd import ops

    q, kc, vc = _inputs(3, 8, 2, 128, 1024)
    lens = _lens([1, 1, 1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ops.attn_decode_ragged(q, kc, vc, lens)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attn_decode_ragged(q, kc, vc, lens)
    for case in ([300, 1, 1024], [0, 513, 256], [77, 0, 0]):
        lens.copy_(_lens(case))
        graph.replay()
        got = out.clone()
        eager = ops.attn_decode_ragged(q, kc, vc, _lens(case))
        assert torch.equal(got, eager)
        _check_rows(got, q, kc, vc, case)


@pytest.mark.parametrize("D", [128, 64])
def test_decode_qkv_append(D):
    from prime_amd import ops

    B, H, Hkv, Smax, T = 3, 8, 2, 64, 256
    NH = H + 2 * Hkv
    cos, sin = ops.reference.rope_tables(D, T, device=DEV)
    qkv = _bf(torch.randn(B, NH * D))
    x = qkv.view(B, 1, NH, D)
    SENT = 3.0

    def run(pos):
        kc = torch.full((B, Smax, Hkv, D), SENT, device=DEV, dtype=torch.bfloat16)
        vc = torch.full_like(kc, SENT)
        q = ops.decode_qkv_append(qkv, cos, sin, kc, vc, _lens(pos), H, Hkv)
        torch.cuda.synchronize()
        return q, kc, vc

    def check(pos, q, kc, vc):
        for b, p in enumerate(pos):
            keep = torch.ones(Smax, dtype=torch.bool, device=DEV)
            if 0 <= p < Smax:
                keep[p] = False
                wq = ops.apply_rope(x[b:b + 1, :, :H].contiguous(), cos, sin,
                                    pos_offset=p)[0, 0]
                wk = ops.apply_rope(x[b:b + 1, :, H:H + Hkv].contiguous(), cos,
                                    sin, pos_offset=p)[0, 0]
                assert torch.equal(q[b], wq)
                assert torch.equal(kc[b, p], wk)
                assert torch.equal(vc[b, p], x[b, 0, H + Hkv:])
            else:
                assert (q[b] == 0).all()
            assert (kc[b, keep] == SENT).all() and (vc[b, keep] == SENT).all()

    pos = [5, 0, 63]
    check(pos, *run(pos))
    # idle and out-of-range slots; the out-of-range one is NOT the last slot,
    # so a missing guard would land in the next sequence's (checked) rows
    pos = [-1, Smax, 7]
    check(pos, *run(pos))


# ------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def model():
    from prime_amd.models import Llama
    from prime_amd.models.configs import get_config

    torch.manual_seed(0)
    cfg = get_config("llama_150m", n_layers=2, n_heads=12, n_kv_heads=6)
    m = Llama(cfg).to(DEV, dtype=torch.bfloat16)
    m.reset_rope(DEV)
    m.eval()
    return m


def _caches(cfg, B, smax):
    return [tuple(torch.zeros(B, smax, cfg.n_kv_heads, cfg.head_dim, device=DEV,
                              dtype=torch.bfloat16) for _ in range(2))
            for _ in range(cfg.n_layers)]


@torch.no_grad()
def test_ragged_step_matches_single_position_path(model):
    from prime_amd.models import Llama

    cfg = model.cfg
    L0 = [5, 33, 64]
    g = torch.Generator().manual_seed(5)
    toks = [torch.randint(0, cfg.vocab_size, (n + 1,), generator=g) for n in L0]
    m32 = Llama(cfg)  # fp32 CPU model with the same (bf16-valued) weights
    m32.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    m32.eval()
    ref = [m32(t[None])[0, -1] for t in toks]  # hidden state of the new token

    smax = 128
    old = []
    for t, n in zip(toks, L0):
        c = _caches(cfg, 1, smax)
        pad = torch.zeros(1, 64, dtype=torch.int64, device=DEV)
        pad[0, :n] = t[:n].to(DEV)
        model(pad, caches=c, pos=0)
        old.append(model(t[n:].view(1, 1).to(DEV), caches=c, pos=n)[0, 0])

    c = _caches(cfg, 3, smax)
    pad = torch.zeros(3, 64, dtype=torch.int64, device=DEV)
    for b, (t, n) in enumerate(zip(toks, L0)):
        pad[b, :n] = t[:n].to(DEV)
    model(pad, caches=c, pos=0)
    cur = torch.stack([t[-1:] for t in toks]).to(DEV)
    sp = {"pos": _lens(L0), "lens": _lens([n + 1 for n in L0])}
    new = model(cur, caches=c, seq_pos=sp)[:, 0]

    for b in range(3):
        e_old = (old[b].float().cpu() - ref[b]).abs().max().item()
        e_new = (new[b].float().cpu() - ref[b]).abs().max().item()
        print(f"L0={L0[b]}: max abs err vs fp32 CPU model: existing path "
              f"{e_old:.4e}, ragged path {e_new:.4e}")
        assert e_new <= 2 * e_old + 1e-3


def _prompts(cfg, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist()
            for n in lengths]


def test_generate_batch_graphed_matches_eager_and_reuses_graph(model):
    from prime_amd.models.generate import generate_batch

    cfg = model.cfg
    ps = _prompts(cfg, (5, 17, 33), 6)
    new = [12, 3, 8]
    eager = generate_batch(model, ps, new, use_graph=False)
    graphed = generate_batch(model, ps, new, use_graph=True)
    assert [len(o) for o in eager] == new
    assert graphed == eager
    ragged = {k: v for k, v in model._decode_sessions.items() if k[0] == "ragged"}
    assert len(ragged) == 1
    (key, sess), = ragged.items()
    assert key[1] == 4  # three prompts: bucket of four, one idle slot
    graph = sess["graph"]

    # another set of prompts in the same bucket: same captured graph
    ps2 = _prompts(cfg, (40, 2, 9), 7)
    new2 = [5, 9, 4]
    eager2 = generate_batch(model, ps2, new2, use_graph=False)
    graphed2 = generate_batch(model, ps2, new2, use_graph=True)
    assert graphed2 == eager2 and [len(o) for o in eager2] == new2
    ragged = {k: v for k, v in model._decode_sessions.items() if k[0] == "ragged"}
    assert list(ragged) == [key] and ragged[key]["graph"] is graph
