"""-m gpu: the sum-product chain of bigram_post_chain_kernel (csrc/decode_bigram_posterior.hip) and bigram_counts_chain_kernel
(csrc/decode_bigram_counts.hip) after it was written once, in csrc/bigram_sumproduct.h, and decode_post_chain_kernel
(csrc/decode_posterior.hip) after its path-posterior pieces moved to csrc/path_posterior.h: bit identity of
wfl_decode_bigram_posterior, wfl_decode_bigram_counts and wfl_decode_posterior (and of wfl_decode_bigram, whose entry was edited on
the host side) against tests/golden/bigram_sumproduct_parent.npz, recorded from the build before that change by
tests/golden/make_bigram_sumproduct_parent.py (cases: tests/bigram_sumproduct_cases.py) -- tobytes() of every output and the status
lists.  The float64 comparisons of test_gpu_decode_posterior.py, test_gpu_decode_bigram_posterior.py and
test_gpu_decode_bigram_counts.py are the second line of defence."""
import os

import numpy as np
import pytest

import bigram_sumproduct_cases as S

pytestmark = pytest.mark.gpu
GOLDEN = "bigram_sumproduct_parent.npz"


@pytest.fixture(scope="module")
def runs():
    return S.run_all()


@pytest.fixture(scope="module")
def want(golden_dir):
    return dict(np.load(os.path.join(golden_dir, GOLDEN)))


def test_the_cases_are_the_recorded_ones(runs, want, golden_dir):
    assert sorted(runs) == sorted(want)
    assert os.path.getsize(os.path.join(golden_dir, GOLDEN)) < 256 * 1024


def _groups():
    return [f"bigram.P{P}.forbid{f}." for P in S.SB.PHONEMES for f, _ in S.BIGRAM_CASES] + [f"flat.{n}." for n in S.FLAT_TABLES] + ["status."]


@pytest.mark.parametrize("prefix", _groups())
def test_outputs_equal_the_parent_build_bit_for_bit(prefix, runs, want):
    keys = [k for k in sorted(want) if k.startswith(prefix)]
    assert keys, prefix
    for k in keys:
        g, w = runs[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, k
        if g.tobytes() != w.tobytes():
            nd = int((g.view(np.uint8) != w.view(np.uint8)).sum()) if g.size else 0
            pytest.fail(f"{k}: differs from the parent build's ({nd} of {g.nbytes} bytes"
                        f"{'; a digest of the whole output' if k.endswith('.sha256') else ''})")
