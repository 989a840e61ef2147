"""Streaming / sharded corpus tokenization for `prime-amd prepare-data`.

The round-1 path read the whole text into memory and produced a single
.bin — fine for samples, unusable for a multi-GB corpus. This module
streams inputs in bounded blocks, tokenizes blocks in parallel worker
processes (order-preserving), and writes fixed-size output shards that
TokenFileDataset consumes directly (a directory of part_*.bin, or one
flat .bin when the corpus fits a single shard).
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Iterator

import numpy as np

_BLOCK_BYTES = 8 << 20  # 8 MiB of UTF-8 per tokenization block


def iter_blocks(paths: list[Path], block_bytes: int = _BLOCK_BYTES) -> Iterator[str]:
    """Stream text files in ~block_bytes chunks, splitting only at line
    boundaries so tokens never straddle a block cut mid-word."""
    for p in paths:
        with open(p, encoding="utf-8", errors="replace") as fh:
            buf: list[str] = []
            size = 0
            for line in fh:
                buf.append(line)
                size += len(line)
                if size >= block_bytes:
                    yield "".join(buf)
                    buf, size = [], 0
            if buf:
                yield "".join(buf)


def iter_segments(paths: list[Path], separator: str | None,
                  block_bytes: int = _BLOCK_BYTES) -> Iterator[str | None]:
    """iter_blocks with document boundaries: yields text blocks, and None
    where an EOS token belongs — at the end of every file and, with a
    separator, in place of every line whose stripped text equals it."""
    for p in paths:
        with open(p, encoding="utf-8", errors="replace") as fh:
            buf: list[str] = []
            size = 0
            for line in fh:
                if separator is not None and line.strip() == separator:
                    if buf:
                        yield "".join(buf)
                        buf, size = [], 0
                    yield None
                    continue
                buf.append(line)
                size += len(line)
                if size >= block_bytes:
                    yield "".join(buf)
                    buf, size = [], 0
            if buf:
                yield "".join(buf)
        yield None


_TOK = None


def _worker_init(tokenizer_path: str) -> None:
    global _TOK
    from ..utils.tokenizer import load_tokenizer

    _TOK = load_tokenizer(tokenizer_path)


def _encode_block(text: str | None, eos_id: int | None = None) -> np.ndarray:
    if text is None:  # document boundary (iter_segments)
        return np.asarray([eos_id], dtype=np.int64)
    return np.asarray(_TOK.encode(text).ids, dtype=np.int64)


class ShardWriter:
    """Append token arrays, rolling to a new part_NNNN.bin every
    `shard_tokens`; a single-shard corpus is renamed to the flat `out`
    path so small cases keep the simple one-file layout."""

    def __init__(self, out: Path, dtype: np.dtype, shard_tokens: int):
        self.out = Path(out)
        self.dtype = dtype
        self.shard_tokens = shard_tokens
        self.dir = self.out if self.out.suffix == "" else self.out.parent
        self.stem = "part" if self.out.suffix == "" else self.out.stem
        self.dir.mkdir(parents=True, exist_ok=True)
        self.total = 0
        self._shard_idx = -1
        self._in_shard = 0
        self._fh = None
        self.paths: list[Path] = []

    def _roll(self) -> None:
        if self._fh:
            self._fh.close()
        self._shard_idx += 1
        p = self.dir / f"{self.stem}_{self._shard_idx:04d}.bin"
        self.paths.append(p)
        self._fh = open(p, "wb")
        self._in_shard = 0

    def write(self, ids: np.ndarray) -> None:
        off = 0
        while off < len(ids):
            if self._fh is None or self._in_shard >= self.shard_tokens:
                self._roll()
            take = min(len(ids) - off, self.shard_tokens - self._in_shard)
            ids[off : off + take].astype(self.dtype).tofile(self._fh)
            self._in_shard += take
            self.total += take
            off += take

    def close(self) -> list[Path]:
        if self._fh:
            self._fh.close()
        # single shard + flat out path requested: keep the simple layout
        if self.out.suffix and len(self.paths) == 1:
            os.replace(self.paths[0], self.out)
            self.paths = [self.out]
        return self.paths


def prepare_corpus(
    inputs: list[str | Path],
    out: str | Path,
    tokenizer_path: str,
    vocab_threshold: int = 65535,
    shard_tokens: int = 512 * 1024 * 1024,
    workers: int = 0,
    eos_id: int | None = None,
    doc_separator: str | None = None,
) -> dict:
    """Tokenize text files into token shards. Returns a summary dict.

    eos_id: append this token id at the end of every input file and, with
    doc_separator, at every line whose stripped text equals it (that line
    is dropped) — the boundaries `data.doc_mask_eos_id` acts on. Without
    eos_id the output is unchanged."""
    import functools

    from ..utils.tokenizer import load_tokenizer

    if doc_separator is not None and eos_id is None:
        raise ValueError("doc_separator needs eos_id")
    if eos_id is not None and eos_id < 0:
        raise ValueError("eos_id must be >= 0")

    paths = [Path(p) for p in inputs]
    for p in paths:
        if not p.exists():
            raise FileNotFoundError(p)
    vocab = load_tokenizer(tokenizer_path).get_vocab_size()
    dtype = np.uint16 if vocab <= vocab_threshold else np.uint32
    if eos_id is not None and eos_id > np.iinfo(dtype).max:
        raise ValueError(f"eos_id {eos_id} does not fit {np.dtype(dtype).name}")
    writer = ShardWriter(Path(out), dtype, shard_tokens)
    if eos_id is None:
        items, encode = iter_blocks(paths), _encode_block
    else:
        items = iter_segments(paths, doc_separator)
        encode = functools.partial(_encode_block, eos_id=eos_id)

    if workers and workers > 1:
        import multiprocessing as mp

        ctx = mp.get_context("spawn")
        with ctx.Pool(workers, initializer=_worker_init,
                      initargs=(tokenizer_path,)) as pool:
            for ids in pool.imap(encode, items, chunksize=1):
                writer.write(ids)
    else:
        _worker_init(tokenizer_path)
        for block in items:
            writer.write(encode(block))
    shards = writer.close()
    return {
        "tokens": writer.total,
        "vocab": vocab,
        "dtype": np.dtype(dtype).name,
        "shards": [str(s) for s in shards],
    }
