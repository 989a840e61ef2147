"""Document-masked attention for packed sequences — CPU layers: the
doc_starts helper, the fp32 reference, the model plumbing (incl. activation
checkpointing), config / Trainer wiring and prepare-data --eos-id."""
import numpy as np
import pytest
import torch

from prime_amd import ops
from prime_amd.models import build_model

EOS = 7


def _loop_doc_starts(rows, eos):
    out = []
    for row in rows:
        cur, r = 0, []
        for i, _ in enumerate(row):
            if i > 0 and row[i - 1] == eos:
                cur = i
            r.append(cur)
        out.append(r)
    return out


# ------------------------------------------------------------ 1. doc_starts
def test_doc_starts_hand_written_rows():
    rows = [
        [1, 2, 3, 4, 5, 6, 1, 2],            # no EOS
        [EOS, 1, 2, 3, 4, 5, 6, 1],          # EOS at index 0
        [1, 2, 3, 4, 5, 6, 1, EOS],          # EOS as last token
        [1, 2, EOS, EOS, 3, 4, 5, 6],        # adjacent EOS: one-token document
        [1, EOS, 2, 3, EOS, 4, EOS, 5],      # several documents
    ]
    want = [
        [0, 0, 0, 0, 0, 0, 0, 0],
        [0, 1, 1, 1, 1, 1, 1, 1],
        [0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 3, 4, 4, 4, 4],
        [0, 0, 2, 2, 2, 5, 5, 7],
    ]
    assert _loop_doc_starts(rows, EOS) == want  # the loop is the spec
    tokens = torch.tensor(rows)  # different rows in one batch
    ds = ops.doc_starts(tokens, EOS)
    assert ds.dtype == torch.int32 and ds.shape == tokens.shape
    assert ds.tolist() == want
    idx = torch.arange(tokens.shape[1])
    assert bool((ds >= 0).all()) and bool((ds <= idx).all())   # 0 <= ds[i] <= i
    assert bool((ds[:, 1:] >= ds[:, :-1]).all())               # non-decreasing
    # int32 tokens (the dtype a uint16 token file is widened to) work too
    assert ops.doc_starts(tokens.int(), EOS).tolist() == want


def test_doc_ends_is_the_mirror():
    from prime_amd.ops.functional import _doc_ends

    tokens = torch.tensor([[1, EOS, 2, 3, EOS, 4, EOS, 5], [1, 2, 3, 4, 5, 6, 1, 2]])
    de = _doc_ends(ops.doc_starts(tokens, EOS))
    assert de.dtype == torch.int32
    assert de.tolist() == [[2, 2, 5, 5, 5, 7, 7, 8], [8] * 8]


# ------------------------------------------------- 2. reference.attention
def _starts_to_doc_start(starts, S):
    ds = torch.zeros(S, dtype=torch.int32)
    for s in starts:
        ds[s:] = s
    return ds


def test_reference_doc_mask_is_block_diagonal():
    torch.manual_seed(0)
    B, S, H, Hkv, D = 2, 48, 4, 2, 16
    q, k, v = torch.randn(B, S, H, D), torch.randn(B, S, Hkv, D), torch.randn(B, S, Hkv, D)
    starts = [[0, 1, 17, 40], [0, 30]]
    ds = torch.stack([_starts_to_doc_start(s, S) for s in starts])
    got = ops.reference.attention(q, k, v, causal=True, doc_start=ds)
    for b, st in enumerate(starts):
        for lo, hi in zip(st, st[1:] + [S]):
            want = ops.reference.attention(q[b:b + 1, lo:hi], k[b:b + 1, lo:hi],
                                           v[b:b + 1, lo:hi], causal=True)
            torch.testing.assert_close(got[b:b + 1, lo:hi], want, atol=1e-5, rtol=1e-5)
    # all-zero doc_start == no mask, exactly
    zero = torch.zeros(B, S, dtype=torch.int32)
    assert torch.equal(ops.reference.attention(q, k, v, causal=True, doc_start=zero),
                       ops.reference.attention(q, k, v, causal=True))
    # the CPU path of the public op is this reference
    assert torch.equal(ops.flash_attention(q, k, v, causal=True, doc_start=ds), got)


def test_flash_attention_doc_start_validation():
    q = torch.randn(1, 8, 2, 16)
    ds = torch.zeros(1, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match="causal"):
        ops.flash_attention(q, q, q, causal=False, doc_start=ds)
    with pytest.raises(TypeError, match="int32"):
        ops.flash_attention(q, q, q, causal=True, doc_start=ds.long())
    with pytest.raises(ValueError, match="shape"):
        ops.flash_attention(q, q, q, causal=True, doc_start=ds[:, :4])
    with pytest.raises(ValueError, match="is on"):
        ops.flash_attention(q, q, q, causal=True, doc_start=ds.to("meta"))


# ---------------------------------------------------- 3. model invariance
def test_model_packed_documents_match_running_alone():
    torch.manual_seed(0)
    m = build_model("llama_test").eval()
    S, cut = 64, 23
    tokens = torch.randint(0, 256, (1, S))
    ds = _starts_to_doc_start([0, cut], S).unsqueeze(0)
    with torch.no_grad():
        packed = m(tokens, doc_start=ds)
        plain = m(tokens)
        first = m(tokens[:, :cut])
        # RoPE is relative: the second document alone, at position 0, gives
        # the hidden states it has at offset `cut` inside the packed row
        second = m(tokens[:, cut:])
    torch.testing.assert_close(packed[:, :cut], first, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(packed[:, cut:], second, atol=1e-5, rtol=1e-5)
    # not vacuous: without the mask the second document sees the first
    assert float((plain[:, cut:] - second).abs().max()) > 0.1


def test_model_decode_paths_reject_doc_start():
    m = build_model("llama_test").eval()
    cfg = m.cfg
    tokens = torch.randint(0, 256, (1, 8))
    ds = torch.zeros(1, 8, dtype=torch.int32)
    caches = [(torch.zeros(1, 16, cfg.n_kv_heads, cfg.head_dim),
               torch.zeros(1, 16, cfg.n_kv_heads, cfg.head_dim))
              for _ in range(cfg.n_layers)]
    with pytest.raises(ValueError, match="doc_start"):
        m(tokens, caches=caches, doc_start=ds)
    with pytest.raises(ValueError, match="doc_start"):
        m.layers[0].attn(torch.zeros(1, 8, cfg.dim), m.rope_cos, m.rope_sin,
                         cache=caches[0], doc_start=ds)


# ------------------------------------------- 4. activation checkpointing
def test_activation_checkpointing_same_loss_with_doc_mask():
    torch.manual_seed(0)
    m1 = build_model("llama_test")
    torch.manual_seed(0)
    m2 = build_model("llama_test", activation_checkpointing=True)
    m2.train()
    x = torch.randint(0, 256, (2, 64))
    y = torch.randint(0, 256, (2, 64))
    ds = torch.stack([_starts_to_doc_start([0, 23], 64),
                      _starts_to_doc_start([0, 5, 40], 64)])
    l1 = m1.loss(x, y, doc_start=ds)
    l2 = m2.loss(x, y, doc_start=ds)
    torch.testing.assert_close(l1, l2, atol=1e-5, rtol=1e-4)
    l1.backward()
    l2.backward()
    g1 = m1.layers[0].attn.wqkv.weight.grad
    g2 = m2.layers[0].attn.wqkv.weight.grad
    torch.testing.assert_close(g1, g2, atol=1e-5, rtol=1e-4)
    # both really ran masked
    with torch.no_grad():
        assert abs(float(m1.loss(x, y)) - float(l1)) > 1e-4
        assert abs(float(m2.loss(x, y)) - float(l2)) > 1e-4


# ------------------------------------------------- 5. config and Trainer
def test_config_key_parses_and_validates(tmp_path):
    from prime_amd.utils.config import (ConfigError, TrainConfig,
                                        default_config_toml, load_config)

    assert TrainConfig().data.doc_mask_eos_id is None
    p = tmp_path / "c.toml"
    p.write_text("[data]\ndoc_mask_eos_id = 2\n")
    assert load_config(p).data.doc_mask_eos_id == 2
    p.write_text("[data]\ndoc_mask_eos_id = -1\n")
    with pytest.raises(ConfigError, match="doc_mask_eos_id"):
        load_config(p)
    assert "doc_mask_eos_id" in default_config_toml()
    p.write_text(default_config_toml())
    assert load_config(p).data.doc_mask_eos_id is None


def _train_cfg(path, eos, **parallel):
    from prime_amd.utils.config import (DataSection, DilocoConfig, MetricsConfig,
                                        ModelConfig, ParallelConfig, TrainConfig)

    return TrainConfig(
        run_name="docmask_cpu", steps=2, device="cpu",
        model=ModelConfig(name="llama_test", seq_len=64),
        data=DataSection(kind="token_file", path=str(path), micro_batch_size=2,
                         shuffle=False, doc_mask_eos_id=eos),
        diloco=DilocoConfig(H=100),
        parallel=ParallelConfig(**parallel),
        metrics=MetricsConfig(log_interval=100),
    )


def test_trainer_rejects_seq_parallel_with_doc_mask(tmp_path):
    from prime_amd.train import Trainer

    with pytest.raises(ValueError, match="seq_parallel"):
        Trainer(_train_cfg(tmp_path / "unused.bin", EOS, seq_parallel=True),
                run_dir=tmp_path)


@pytest.mark.parametrize("eos", [EOS, None])
def test_trainer_hands_doc_start_to_flash_attention(tmp_path, monkeypatch, eos):
    from prime_amd.train import Trainer

    rng = np.random.default_rng(0)
    toks = rng.integers(8, 256, size=2000).astype(np.uint16)
    toks[rng.choice(2000, size=60, replace=False)] = EOS
    path = tmp_path / "toks.bin"
    toks.tofile(path)

    seen = []
    real = ops.flash_attention

    def spy(q, k, v, causal=True, doc_start=None):
        seen.append(doc_start)
        return real(q, k, v, causal=causal, doc_start=doc_start)

    monkeypatch.setattr(ops, "flash_attention", spy)
    tr = Trainer(_train_cfg(path, eos), run_dir=tmp_path / "run")
    try:
        losses = [float(tr.train_step()) for _ in range(2)]
    finally:
        tr.close()
    assert all(np.isfinite(losses))
    assert len(seen) == 2 * 2  # two layers, two steps
    if eos is None:
        assert all(d is None for d in seen)
        return
    # shuffle=False, one shard: step 0 reads windows 0 and 1 of the file
    x0 = torch.from_numpy(np.stack([toks[0:64], toks[64:128]]).astype(np.int64))
    want = torch.tensor(_loop_doc_starts(x0.tolist(), EOS), dtype=torch.int32)
    assert int(want.max()) > 0, "fixture must contain a document boundary"
    assert seen[0].dtype == torch.int32 and torch.equal(seen[0], want)
    assert seen[1] is seen[0]  # built once per micro-batch, shared by layers


# ------------------------------------------------ 6. prepare-data --eos-id
def test_prepare_data_eos_id(tmp_path):
    tokenizers = __import__("tokenizers")
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import Whitespace
    from tokenizers.trainers import WordLevelTrainer
    from typer.testing import CliRunner

    from prime_amd.cli.main import app

    a = "alpha beta gamma\n<|doc|>\ndelta epsilon\nzeta\n  <|doc|>  \neta\n"
    b = "theta alpha\n"
    fa, fb = tmp_path / "a.txt", tmp_path / "b.txt"
    fa.write_text(a)
    fb.write_text(b)
    tok = tokenizers.Tokenizer(WordLevel(unk_token="<unk>"))
    tok.pre_tokenizer = Whitespace()
    words = "alpha beta gamma delta epsilon zeta eta theta"
    tok.train_from_iterator([words], WordLevelTrainer(special_tokens=["<unk>", "<eos>"]))
    tok_path = tmp_path / "tok.json"
    tok.save(str(tok_path))
    eos = tok.token_to_id("<eos>")
    ids = lambda s: tok.encode(s).ids  # noqa: E731

    base = ["prepare-data", str(fa), str(fb), "--tokenizer", str(tok_path)]
    out = tmp_path / "eos.bin"
    r = CliRunner().invoke(app, base + ["--out", str(out), "--eos-id", str(eos),
                                        "--doc-separator", "<|doc|>"])
    assert r.exit_code == 0, r.output
    want = (ids("alpha beta gamma") + [eos] + ids("delta epsilon zeta") + [eos]
            + ids("eta") + [eos] + ids("theta alpha") + [eos])
    assert np.fromfile(out, dtype=np.uint16).tolist() == want

    # --eos-id alone: file ends only; the separator line is ordinary text
    out2 = tmp_path / "eos_files.bin"
    r = CliRunner().invoke(app, base + ["--out", str(out2), "--eos-id", str(eos)])
    assert r.exit_code == 0, r.output
    assert np.fromfile(out2, dtype=np.uint16).tolist() == ids(a) + [eos] + ids(b) + [eos]

    # without the flag: the bytes the tool has always written
    out3 = tmp_path / "plain.bin"
    r = CliRunner().invoke(app, base + ["--out", str(out3)])
    assert r.exit_code == 0, r.output
    assert out3.read_bytes() == np.asarray(ids(a) + ids(b), dtype=np.uint16).tobytes()
