"""-m gpu: the sum-product sweeps of post_kernel (csrc/align_posterior.h) and edits_fb_kernel (csrc/align_edits.hip) after they were
written once, in csrc/lattice_sums.h: bit identity of wfl_align_posterior, wfl_align_posterior_windowed,
wfl_align_min_duration_posterior, wfl_align_edits and wfl_align_insertions against tests/golden/sumproduct_parent.npz, recorded from
the build before that change by tests/golden/make_sumproduct_parent.py (cases: tests/sumproduct_cases.py) -- tobytes() of every
output and the status lists.  The float64 comparisons of test_gpu_align_posterior*.py, test_gpu_align_duration_posterior.py,
test_gpu_align_edits.py and test_gpu_align_insertions.py are the second line of defence."""
import os

import numpy as np
import pytest

import sumproduct_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs():
    return S.run_all()


@pytest.fixture(scope="module")
def want(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "sumproduct_parent.npz")))


def test_the_cases_are_the_recorded_ones(runs, want):
    assert sorted(runs) == sorted(want)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "sumproduct_parent.npz")) < 256 * 1024


def _groups():
    calls = ["configs", "frames"] + [f"C{C}" for C in S.STAGE_C]
    return [f"{c}.{e}." for c in calls for e in S.ENTRIES] + ["edits.", "insertions."]


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
