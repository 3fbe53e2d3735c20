"""CPU (-m "not gpu"): the phoneme duration prior (wfl-asr_amd/durations.py): the estimate from hand-counted `.lab` files, its
normalisation, what smoothing 0 forbids, the JSON file, the refusals by name, the search's table, and the command line."""
import json
import math

import numpy as np
import pytest

import __graft_entry__  # noqa: F401
from wfl_asr_amd import durations as DU

FD = 0.02


def _lab(path, segs):
    """segs: [(start frame, frames, name)] -> an HTK .lab on the 20 ms clock."""
    path.write_text("".join(f"{int(round(s * FD * 1e7))} {int(round((s + n) * FD * 1e7))} {name}\n" for s, n, name in segs))
    return str(path)


@pytest.fixture()
def labs(tmp_path):
    """a: 1, 1, 2, 3, 3, 5 frames; b: 2, 7 frames; two files."""
    one = _lab(tmp_path / "one.lab", [(0, 1, "a"), (1, 2, "b"), (5, 1, "a"), (6, 2, "a"), (10, 3, "a")])
    two = _lab(tmp_path / "two.lab", [(2, 3, "a"), (5, 7, "b"), (12, 5, "a")])
    return [one, two]


def test_hand_counted_files(labs):
    p = DU.estimate(labs, max_frames=3, smoothing=1.0)
    assert p.phonemes == ["a", "b"] and p.max_frames == 3 and p.frame_duration == FD
    assert p.counts == [{1: 2, 2: 1, 3: 2, 5: 1}, {2: 1, 7: 1}]
    # a: n_tot 6, K D = 3 -> denominator 9; c_ge = 3 (3, 3, 5); excess = 0 + 0 + 2
    P1, P2, M = 3 / 9, 2 / 9, 4 / 9
    m = (2 + 1) / (3 + 1)
    rho = m / (1 + m)
    assert np.allclose(np.exp(p.log_prob[0]), [P1, P2, M * (1 - rho)], rtol=0, atol=1e-15)
    assert math.isclose(p.log_tail[0], math.log(rho), abs_tol=1e-15)
    # b: n_tot 2 -> 5; c_ge = 1 (7), excess 4
    m = (4 + 1) / (1 + 1)
    rho = m / (1 + m)
    assert np.allclose(np.exp(p.log_prob[1]), [1 / 5, 2 / 5, (2 / 5) * (1 - rho)], rtol=0, atol=1e-15)
    assert math.isclose(p.log_tail[1], math.log(rho), abs_tol=1e-15)


@pytest.mark.parametrize("D, K", [(1, 1.0), (2, 0.0), (3, 1.0), (4, 0.5), (8, 0.0), (32, 1.0)])
def test_every_phoneme_sums_to_one(labs, D, K):
    p = DU.estimate(labs, max_frames=D, smoothing=K)
    for row, tail in zip(p.log_prob, p.log_tail):
        P = np.exp(row)
        rho = math.exp(tail)
        M = P[-1] / (1 - rho)                              # P(D) = M (1 - rho)
        assert abs(P.sum() + M * rho - 1.0) < 1e-12
        assert abs(P.sum() + sum(P[-1] * rho ** i for i in range(1, 4000)) - 1.0) < 1e-9      # the geometric tail itself


def test_smoothing_zero_forbids_the_unseen(labs):
    p = DU.estimate(labs, max_frames=8, smoothing=0.0)
    a, b = p.log_prob
    assert np.isfinite(a[[0, 1, 2, 4]]).all() and np.isneginf(a[[3, 5, 6, 7]]).all() and np.isneginf(p.log_tail[0])
    assert np.isfinite(b[[1, 6]]).all() and np.isneginf(b[[0, 2, 3, 4, 5, 7]]).all()
    q = DU.estimate(labs, max_frames=3, smoothing=0.0)     # b at D = 3: nothing of 1 or 3 frames, one of 7: P(3) = 1/2 (1 - rho)
    assert np.isneginf(q.log_prob[1][0]) and math.isclose(math.exp(q.log_tail[1]), 4 / 5, abs_tol=1e-15)
    assert all(np.isfinite(r).all() for r in DU.estimate(labs, max_frames=8, smoothing=1.0).log_prob)


def test_rounding_and_the_frame_clock(tmp_path):
    assert [DU.frames_of(0, s, FD) for s in (0.0, 0.004, 0.02, 0.029, 0.03, 0.031, 0.05, 0.0501)] == [1, 1, 1, 1, 2, 2, 3, 3]
    lab = _lab(tmp_path / "x.lab", [(0, 4, "a")])
    assert DU.estimate([lab], max_frames=8, smoothing=0, frame_duration=0.01).counts == [{8: 1}]


def test_json_round_trip_and_null_rows(labs, tmp_path):
    p = DU.estimate(labs, symbols=["b", "zz", "a"], max_frames=5, smoothing=0.0)
    assert p.phonemes == ["b", "zz", "a"] and p.log_prob[1] is None
    path = tmp_path / "sub" / "phoneme_durations.json"
    DU.save(p, str(path))
    d = json.loads(path.read_text())
    assert sorted(d) == ["frame_duration", "log_prob", "log_tail", "max_frames", "phonemes"]
    assert d["frame_duration"] == FD and d["max_frames"] == 5 and d["phonemes"] == ["b", "zz", "a"]
    assert d["log_prob"][1] is None and d["log_prob"][0][0] is None and isinstance(d["log_prob"][0][1], float)
    assert d["log_tail"][2] is None                        # a: nothing longer than 5 frames was seen, K = 0
    q = DU.load(str(path))
    assert q.phonemes == p.phonemes and q.max_frames == 5 and q.log_prob[1] is None
    for r, s in zip(p.log_prob, q.log_prob):
        assert r is None and s is None or np.array_equal(r, s)
    assert np.array_equal(p.log_tail[[0, 2]], q.log_tail[[0, 2]])
    for text, match in (('{"phonemes": []}', "not a phoneme duration file"),
                        (json.dumps({**d, "max_frames": 40}), "max_frames must be"),
                        (json.dumps({**d, "phonemes": ["a", "a", "b"]}), "distinct"),
                        (json.dumps({**d, "log_tail": [0.5, None, None]}), "above 0"),
                        (json.dumps({**d, "log_prob": [[0.0], None, None]}), "rows of 5 values")):
        bad = tmp_path / "bad.json"
        bad.write_text(text)
        with pytest.raises(ValueError, match=match):
            DU.load(str(bad))


def test_refusals_by_name(labs):
    with pytest.raises(ValueError, match="not among the symbols: b$"):
        DU.estimate(labs, symbols=["a"])
    for kw, match in ((dict(max_frames=0), "max_frames"), (dict(max_frames=33), "max_frames"), (dict(smoothing=-1), "smoothing"),
                      (dict(smoothing=float("nan")), "smoothing"), (dict(frame_duration=0), "frame_duration")):
        with pytest.raises(ValueError, match=match):
            DU.estimate(labs, **kw)
    p = DU.estimate(labs, max_frames=4)
    DU.check(p, ["a", "b", "c"], FD)
    with pytest.raises(ValueError, match="no output name of the label set: b$"):
        DU.check(p, ["a", "c"], FD)
    with pytest.raises(ValueError, match=r"x\.json: counted on frames of 0\.02 s, the model's frames last 0\.01 s"):
        DU.check(p, ["a", "b"], 0.01, path="x.json")


def test_table_keeps_minus_infinity_at_every_weight(labs):
    p = DU.estimate(labs, symbols=["a", "zz", "b"], max_frames=8, smoothing=0.0)
    for w in (0.0, 0.5, 1.0, 3.0):
        t = DU.table(p, w)
        assert t.dtype == np.float32 and t.shape == (3, 9)
        for i in (0, 2):
            full = np.concatenate([p.log_prob[i], [p.log_tail[i]]])
            assert np.array_equal(np.isneginf(t[i]), np.isneginf(full))
            assert np.allclose(t[i][np.isfinite(full)], w * full[np.isfinite(full)], rtol=1e-6)
        assert (t[1] == 0).all() and not np.isnan(t).any() and not np.isposinf(t).any()
    assert (DU.table(p, 0)[0][:8][np.isfinite(p.log_prob[0])] == 0).all()
    for bad in (-1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="duration_prior_weight"):
            DU.table(p, bad)


def test_command_line(labs, tmp_path, capsys):
    phon = tmp_path / "phonemes.txt"
    phon.write_text("O\nB-a\nI-a\nB-b\nI-b\nB-q\nI-q\n")
    out = tmp_path / "d.json"
    DU.main([str(tmp_path), "-o", str(out), "--phonemes", str(phon), "--max-frames", "4", "--smoothing", "0.5"])
    said = capsys.readouterr().out
    assert "no sample, no prior: q" in said and "2 .lab files, 8 segments, 2 phonemes with a prior" in said
    p = DU.load(str(out))
    assert p.phonemes == ["a", "b", "q"] and p.max_frames == 4 and p.log_prob[2] is None
    want = DU.estimate(labs, ["a", "b", "q"], 4, 0.5)
    assert all(np.allclose(r, s) for r, s in zip(p.log_prob[:2], want.log_prob[:2]))
    (tmp_path / "nothing_here").mkdir()
    with pytest.raises(SystemExit):
        DU.main([str(tmp_path / "nothing_here"), "-o", str(out)])
    phon.write_text("O\nB-a\nI-a\n")
    with pytest.raises(SystemExit):
        DU.main([str(tmp_path), "-o", str(out), "--phonemes", str(phon)])
    assert "not among the symbols: b" in capsys.readouterr().err
