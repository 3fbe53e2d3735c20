"""No GPU: the float64 restatement of wfl_align_optional_posterior (tests/optional_posterior_ref.py) against the enumeration of every
path of tiny skip lattices; the option rules of `optional_scores`; the OptionalTokenScore rows and their files; the argument refusals
of align.optional_posteriors that are raised before any GPU work."""
import itertools

import numpy as np
import pytest

import optional_posterior_ref as OP
import posterior_ref as P
import viterbi_ref as V
from wfl_asr_amd import align as AL
from wfl_asr_amd import options as OPT
from wfl_asr_amd import reports as RP

C = 12
GAPS = [0, 11]


def _alts(N, rng):
    ph = rng.choice(np.arange(1, 6), size=N, replace=True)
    return [[(int(2 * p - 1), int(2 * p))] for p in ph]


@pytest.mark.parametrize("lam", [0.0, 0.7, 3.0])
def test_reference_equals_the_enumeration_of_every_path(lam):
    """Every T <= 5, N <= 4, every flag pattern: logz and keep_post within 1e-10 of the enumeration (rounding is 1e-15; a wrong arc is
    of order 1e-2)."""
    rng = np.random.default_rng(int(lam * 10) + 5)
    worst_z = worst_k = 0.0
    n_cases = 0
    for T in range(1, 6):
        for N in range(0, 5):
            for flags in itertools.product([0, 1], repeat=N):
                alts = _alts(N, rng)
                z = (rng.standard_normal((T, C)) * 2.0).astype(np.float32)
                en = OP.enumerate_paths(z, alts, GAPS, flags, lam)
                fb = OP.forward_backward(z, alts, GAPS, flags, lam)
                assert (en is None) == (fb is None), (T, N, flags)
                if en is None:
                    continue
                n_cases += 1
                worst_z = max(worst_z, abs(en["logz"] - fb["logz"]))
                if N:
                    worst_k = max(worst_k, float(np.abs(en["keep_post"] - fb["sum_gamma_b"]).max()))
    print(f"lam {lam}: {n_cases} lattices, logz off by {worst_z:.2e}, keep_post by {worst_k:.2e}")
    assert n_cases > 100
    assert worst_z <= 1e-10 and worst_k <= 1e-10


def test_windows_in_the_reference_equal_the_enumeration():
    rng = np.random.default_rng(3)
    for T, N, flags, wins in [(5, 3, (0, 1, 0), [(0, 4), (3, 2), (0, 4)]), (5, 3, (1, 1, 1), [(1, 2), (0, 4), (2, 4)]),
                              (4, 2, (0, 1), [(0, 0), (2, 3)])]:
        alts = _alts(N, rng)
        z = (rng.standard_normal((T, C)) * 2.0).astype(np.float32)
        en = OP.enumerate_paths(z, alts, GAPS, flags, 0.7, windows=wins)
        fb = OP.forward_backward(z, alts, GAPS, flags, 0.7, windows=wins)
        assert abs(en["logz"] - fb["logz"]) <= 1e-10
        assert np.abs(en["keep_post"] - fb["sum_gamma_b"]).max() <= 1e-10
        if (3, 2) in wins:                       # an optional token with an empty window is never present
            assert fb["sum_gamma_b"][wins.index((3, 2))] == 0.0


def test_with_every_flag_0_the_reference_is_posterior_ref():
    rng = np.random.default_rng(11)
    for T, N in [(9, 4), (40, 7), (17, 1)]:
        alts = _alts(N, rng)
        z = (rng.standard_normal((T, C)) * 2.0).astype(np.float32)
        states, _ = V.viterbi(z, alts, GAPS)
        _, tok = V.outputs(states, z, alts, 0)
        for dt in (np.float64, np.float32):
            a = P.forward_backward(z, alts, GAPS, tok=tok, dtype=dt)
            b = OP.forward_backward(z, alts, GAPS, np.zeros(N, int), 2.5, tok=tok, dtype=dt)
            assert a["logz"] == b["logz"]
            for k in ("tok_post", "start_mean", "start_sd"):
                np.testing.assert_array_equal(a[k], b[k])
            np.testing.assert_allclose(b["keep_post"], 1.0, atol=1e-5 if dt is np.float32 else 1e-12)


# ---------------------------------------------------------------------------------------------------------------- option rules
def _resolve(post):
    return OPT.resolve(post)


def test_rule_25_optional_scores_needs_viterbi():
    with pytest.raises(ValueError, match="optional_scores.*align: viterbi"):
        _resolve({"optional_scores": True})                      # (rule 25 comes before rule 26; with optional_tokens rule 20 speaks)
    with pytest.raises(ValueError, match="optional_tokens needs align"):
        _resolve({"optional_scores": True, "optional_tokens": ["cl"]})


def test_rule_26_optional_scores_needs_optional_tokens():
    with pytest.raises(ValueError, match="optional_scores.*optional_tokens"):
        _resolve({"align": "viterbi", "optional_scores": True})


def test_optional_scores_is_accepted_beside_optional_tokens_and_defaults_to_off():
    o = _resolve({"align": "viterbi", "optional_tokens": ["cl"], "optional_scores": True})
    assert o.optional_scores is True
    assert _resolve({"align": "viterbi", "optional_tokens": ["cl"]}).optional_scores is False
    assert _resolve({}).optional_scores is False


@pytest.mark.parametrize("key", ["align_scores", "align_edits", "align_insertions", "duration_scores"])
def test_every_rule_23_combination_is_still_refused(key):
    post = {"align": "viterbi", "optional_tokens": ["cl"], "optional_scores": True, key: True}
    if key == "duration_scores":
        post["min_duration"] = 0.02
    with pytest.raises(ValueError):
        _resolve(post)


# -------------------------------------------------------------------------------------------------------- rows and their files
def _rows():
    transcript = ["a", "cl", "k", "q", "o", "br"]
    optional = [0, 1, 0, 1, 0, 1]
    skipped = [0, 1, 0, 0, 0, 1]
    keep = [1.0, 0.7, 1.0, 0.9, 1.0, 0.2]
    segments = [(0.0, 0.1, "a"), (0.2, 0.3, "k"), (0.3, 0.35, "q"), (0.35, 0.5, "o")]
    return AL.optional_token_scores(optional, skipped, keep, segments, transcript)


def test_optional_token_scores_rows_and_the_doubt_rule():
    rows = _rows()
    assert [(r.index, r.token, r.kept) for r in rows] == [(1, "cl", False), (3, "q", True), (5, "br", False)]
    assert rows[0].start_s == rows[0].end_s == 0.2                  # the place: the start of the next kept token
    assert (rows[1].start_s, rows[1].end_s) == (0.3, 0.35)
    assert rows[2].start_s == rows[2].end_s == 0.5                  # nothing follows: the end of the last segment
    assert [round(r.confidence, 6) for r in rows] == [0.3, 0.9, 0.8]
    assert [r.doubt for r in rows] == [True, False, False]           # skipped at keep 0.7: the other decision has more mass
    half = AL.OptionalTokenScore(0, "x", True, 0.5, 0.0, 0.1)
    assert not half.doubt                                             # exactly 0.5 is not below 0.5
    with pytest.raises(ValueError):
        AL.optional_token_scores([0, 1], [0, 1, 0], [1.0, 0.5, 1.0], [], ["a", "b", "c"])


def test_the_tsv_writers_and_the_folder_order():
    rows = _rows()
    text = RP.file_text("optional", rows)
    lines = text.split("\n")
    assert lines[0] == "index\ttoken\tdecision\tkeep_posterior\tstart_s\tend_s\tdoubt"
    assert lines[1] == "1\tcl\tskipped\t0.700000\t0.2000000\t0.2000000\t1"
    assert lines[2] == "3\tq\tkept\t0.900000\t0.3000000\t0.3500000\t0"
    assert len(lines) == 5 and lines[-1] == ""
    assert RP.file_text("optional", []) == lines[0] + "\n"
    other = [AL.OptionalTokenScore(0, "cl", True, 0.55, 0.0, 0.1)]
    folder = RP.folder_text("optional", [("a.wav", rows), ("b.wav", other)]).split("\n")
    assert folder[0] == "file\t" + lines[0]
    assert [ln.split("\t")[0:2] for ln in folder[1:-1]] == [["a.wav", "1"], ["b.wav", "0"], ["a.wav", "5"], ["a.wav", "3"]]
    conf = [r.confidence for _, r in RP.folder_rows("optional", [("a.wav", rows), ("b.wav", other)])]
    assert conf == sorted(conf)


# ------------------------------------------------------------------------------------------ refusals that need no GPU
class _FakePacked:
    def __init__(self, d_min):
        self.d_min, self.N, self.nb = d_min, np.array([2], np.int32), 1


def test_optional_posteriors_refuses_min_frames_and_a_bad_penalty():
    with pytest.raises(ValueError, match="min_frames"):
        AL.optional_posteriors(None, [4], None, None, 0, [[0, 1]], None, packed=_FakePacked(object()))
    for lam in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="skip_penalty"):
            AL.optional_posteriors(None, [4], None, None, 0, [[0, 1]], None, skip_penalty=lam, packed=_FakePacked(None))


def test_the_library_exports_the_two_entries():
    from wfl_asr_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "wfl_align_optional_posterior") and hasattr(lib, "wfl_align_optional_posterior_workspace_bytes")
    assert AL.optional_posterior_workspace_bytes([200, 50], [100, 20]) == AL.posterior_workspace_bytes([200, 50], [100, 20])
    assert AL.optional_posterior_workspace_bytes([0], [5]) == 0
