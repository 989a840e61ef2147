"""Guards the driver contract: bench.py single- and multi-rank invocations
must emit exactly one well-formed JSON line from rank 0."""
import json
import os
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def _check_payload(out: str, n_gpus: int):
    lines = [l for l in out.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in d, key
    assert d["n_gpus"] == n_gpus
    assert d["scaling"] == "weak" and d["dtype"] == "bf16"
    assert d["config"]["model"] and d["config"]["seq_len"]
    assert d["value"] > 0
    return d


def test_bench_single_rank_cpu():
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
         "--model", "llama_test", "--seq-len", "64", "--micro-batch", "2",
         "--h", "2"],
        cwd=REPO, capture_output=True, text=True, timeout=300,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    _check_payload(out.stdout, 1)


def test_bench_dump_outputs_cpu(tmp_path):
    """--dump-outputs writes the last timed step's arrays as float .npy,
    identically for identical arguments; --full still ends in one line."""
    import numpy as np

    dumps = []
    for tag, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / tag
        out = subprocess.run(
            [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
             "--model", "llama_test", "--seq-len", "64", "--micro-batch", "2",
             "--h", "2", "--dump-outputs", str(d), *extra],
            cwd=REPO, capture_output=True, text=True, timeout=300,
            env={**os.environ, "BENCH_RUN_DIR": str(tmp_path / "run")},
        )
        assert out.returncode == 0, out.stderr[-2000:]
        assert _check_payload(out.stdout, 1)["steps"] == 2
        dumps.append({f.stem: np.load(f) for f in sorted(d.glob("*.npy"))})
    a, b = dumps
    assert set(a) == set(b) >= {"loss", "weights_sample", "grads_sample"}
    assert sum(v.nbytes for v in a.values()) <= 64 * 2**20
    for name, v in a.items():
        assert v.dtype in (np.float32, np.float64), name
        assert v.size > 0 and np.isfinite(v).all(), name
        assert np.array_equal(v, b[name]), name
    assert np.abs(a["grads_sample"]).max() > 0


def test_bench_two_ranks_cpu():
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29411", "bench.py", "--gpus", "2", "--steps", "2",
         "--warmup", "1", "--model", "llama_test", "--seq-len", "64",
         "--micro-batch", "2", "--h", "2"],
        cwd=REPO, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    d = _check_payload(out.stdout, 2)
    assert "diloco2" in d["config"]["parallelism"]
