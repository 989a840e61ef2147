"""The bf16 serving attention kernels (ragged decode and chunked prefill,
contiguous and paged) keep the bits of the build that
tests/golden/serving_bits.json was recorded on
(tools/record_attn_bits.py --suite serving). That these outputs are right is
checked against the fp32 reference by tests/test_kv_paged_gpu.py on the same
shapes; the cases: tests/serving_bits_cases.py."""
import pytest

from tests import serving_bits_cases as sb

pytestmark = pytest.mark.gpu


def test_golden_file_lists_exactly_the_cases():
    assert sorted(sb.load_golden()) == sorted(sb.CASES)


@pytest.mark.parametrize("name", list(sb.CASES))
def test_same_bits_as_recorded(name):
    got = sb.digests(sb.run_here(sb.CASES[name]))
    want = sb.load_golden()[name]
    differ = [n for n in sb.OUTPUTS if got[n] != want[n]]
    assert not differ, f"{name}: bits of {differ} differ from the recorded build"
