"""Flash attention forward and backward keep the bits of the build that
tests/golden/attn_bits.json was recorded on (tools/record_attn_bits.py), and
the same outputs agree with the fp32 CPU reference, so that a wrong golden
file cannot hide a wrong kernel. The cases and why they are the smallest that
matter: tests/attn_bits_cases.py.

Each case runs on the GPU once; both tests share its outputs."""
import functools

import pytest
import torch

from tests import attn_bits_cases as ab

pytestmark = pytest.mark.gpu

TOL_O = 3e-2     # atol = rtol on o, as test_flash_attention_fwd_bwd
TOL_GRAD = 5e-2  # atol = rtol on gradients, as tests/test_attn_dkv_gpu.py


@pytest.fixture(scope="module")
def own_process_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("attn_bits")


@functools.lru_cache(maxsize=None)
def _outputs(name, tmp_dir):
    return ab.run(ab.CASES[name], tmp_dir)


@functools.lru_cache(maxsize=None)
def _reference(shape, causal, doc):
    """Shared by every launch mode of one shape; never modified."""
    return ab.reference(ab.Case("ref", shape, causal, doc, (), False))


def test_golden_file_lists_exactly_the_cases():
    assert sorted(ab.load_golden()) == sorted(ab.CASES)


@pytest.mark.parametrize("name", list(ab.CASES))
def test_same_bits_as_recorded(name, own_process_dir):
    got = ab.digests(_outputs(name, own_process_dir))
    want = ab.load_golden()[name]
    differ = [n for n in ab.OUTPUTS if got[n] != want[n]]
    assert not differ, f"{name}: bits of {differ} differ from the recorded build"


@pytest.mark.parametrize("name", list(ab.CASES))
def test_against_cpu_reference(name, own_process_dir):
    case = ab.CASES[name]
    got = _outputs(name, own_process_dir)
    want = _reference(case.shape, case.causal, case.doc)
    for n, tol in (("o", TOL_O), ("dq", TOL_GRAD), ("dk", TOL_GRAD), ("dv", TOL_GRAD)):
        g = got[n].float()
        assert bool(torch.isfinite(g).all()), f"{name} {n} not finite"
        print(f"{name} {n}: max abs diff {float((g - want[n]).abs().max()):.3e}")
        torch.testing.assert_close(g, want[n], atol=tol, rtol=tol,
                                   msg=lambda m, n=n: f"{name} {n}: {m}")
    assert bool(torch.isfinite(got["lse"]).all()), f"{name} lse not finite"
