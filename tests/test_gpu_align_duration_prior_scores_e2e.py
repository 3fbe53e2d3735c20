"""-m gpu: `postprocess.duration_prior_scores` end to end on the fixtures of test_gpu_align_duration_prior_e2e.py (the synthetic tiny
Whisper checkpoint, priors written by hand): the .lab files are byte for byte what they are without the option, the three kinds of
files are written with the documented headers, token_durations.tsv lists the tokens with a prior row by their log_prior, a file the
prior left no path for is scored by wfl_align_posterior with one line and gets no .durations.tsv, a file that fell back to the greedy
alignment gets no score file and one line, and Labeler.label_files returns the rows."""
import os
import shutil

import numpy as np
import pytest

from test_gpu_align_duration_prior_e2e import CT, FD, NAMES, NEG, _prior, _transcript, whisper  # noqa: F401  (whisper: the fixture)
from test_gpu_align_e2e import _write_tr
from wfl_asr_amd import align as AL
from wfl_asr_amd import infer as I
from wfl_asr_amd import reports as RP

pytestmark = pytest.mark.gpu


def _folder(d, tmp_path):
    """a.wav: searched and scored under the prior; b.wav: its ten p00 need 320 of its 200 frames, the prior leaves no path; c.wav: a
    token that is no output name, the greedy alignment; e.wav: no transcript."""
    folder = tmp_path / "in"
    os.makedirs(folder)
    for name, src in (("a.wav", "a.wav"), ("b.wav", "plain.wav"), ("c.wav", "plain.wav"), ("e.wav", "plain.wav")):
        shutil.copyfile(str(d / "wavs" / src), str(folder / name))
    rng = np.random.default_rng(11)
    tr_a = [str(x) for x in rng.choice(NAMES[1:], size=40)]
    tr_a = tr_a[:10] + ["p00"] + tr_a[10:20] + ["SP"] + tr_a[20:30] + ["p00"] + tr_a[30:]
    _write_tr(str(folder / "a.wav"), tr_a)
    _write_tr(str(folder / "b.wav"), ["p00", "p01"] * 10)
    _write_tr(str(folder / "c.wav"), ["p01", "zz9", "p02"])
    # p00: at least 32 frames; p01: a soft histogram; p02: one to three frames, never more; p03: no samples, no row
    soft = [-2.0, -1.0, -0.4, -1.5] + [-3.0] * 28
    short = [-0.7, -0.7, -0.9] + [NEG] * 29
    pr_path, prior = _prior(d, "scores.json", [[NEG] * 31 + [0.0], soft, short, None], [0.0, -0.4, NEG, NEG], 32)
    return folder, tr_a, pr_path, prior


def test_the_reports_and_both_fallbacks(whisper, tmp_path, capsys):  # noqa: F811
    d, lab = whisper
    folder, tr_a, pr_path, prior = _folder(d, tmp_path)
    kw = dict(folder_path=str(folder), config_path=str(d / "config.yaml"), checkpoint_path=str(d / "best_model.pt"),
              confidence_threshold=CT, align="viterbi", duration_prior=pr_path)
    I.infer_folder(output_dir=str(tmp_path / "without"), **kw)
    capsys.readouterr()
    I.infer_folder(output_dir=str(tmp_path / "with"), duration_prior_scores=True, **kw)
    out = capsys.readouterr().out
    assert sorted(os.listdir(tmp_path / "without")) == ["a.lab", "b.lab", "c.lab", "e.lab"]
    assert sorted(os.listdir(tmp_path / "with")) == ["a.durations.tsv", "a.lab", "a.scores.tsv", "alignment_scores.tsv", "b.lab",
                                                      "b.scores.tsv", "c.lab", "e.lab", "token_durations.tsv"]
    for name in ("a.lab", "b.lab", "c.lab", "e.lab"):
        assert open(tmp_path / "with" / name, "rb").read() == open(tmp_path / "without" / name, "rb").read(), name
    # the two fallbacks, one line each
    assert out.count(I.DURATION_PRIOR_INFEASIBLE) == 1 and out.count(I.DURATION_PRIOR_SCORES_PLAIN) == 1
    assert out.count("no duration-prior scores (the file was not Viterbi-aligned)") == 1
    assert f"{folder / 'b.wav'}: {I.DURATION_PRIOR_SCORES_PLAIN}" in out and f"{folder / 'c.wav'}: no duration-prior scores" in out
    # {stem}.scores.tsv, align_scores' format
    for name, n in (("a.scores.tsv", len(tr_a)), ("b.scores.tsv", 20)):
        lines = open(tmp_path / "with" / name).read().split("\n")
        assert lines[0].startswith("# path_log_posterior=") and "min_posterior=" in lines[0] and len(lines) == n + 2
        assert all(len(ln.split("\t")) == 6 for ln in lines[1:-1])
        assert float(lines[0].split("\t")[0].split("=")[1]) <= 1e-3 * 350            # score <= logz, within the search's own bound
    # {stem}.durations.tsv
    lines = open(tmp_path / "with" / "a.durations.tsv").read().split("\n")
    assert lines[0] == RP.REPORTS["durations"].header and len(lines) == len(tr_a) + 2 and lines[-1] == ""
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert [r[1] for r in rows] == tr_a and [int(r[0]) for r in rows] == list(range(len(tr_a)))
    frames = np.array([int(r[4]) for r in rows])
    for r, t in zip(rows, tr_a):
        d_k = int(r[4])
        if t in ("SP", "p03"):
            assert r[5] == "none"
        else:
            want = prior.log_prob[NAMES.index(t)][d_k - 1] if d_k <= 32 else None
            assert want is None or float(r[5]) == pytest.approx(want, abs=1e-5)
            assert float(r[5]) > NEG                                                  # the search kept to the table
        assert 0.0 <= float(r[6]) <= 1.0 and float(r[8]) >= 0 and float(r[10]) >= 0
        assert float(r[11]) == pytest.approx(d_k + (float(r[9]) - float(r[7])) / FD, abs=2e-3)
    assert (frames[[t == "p00" for t in tr_a]] >= 32).all() and (frames[[t == "p02" for t in tr_a]] <= 3).all()
    # alignment_scores.tsv: the two scored files; token_durations.tsv: a's tokens that have a row, the lowest log_prior first
    review = open(tmp_path / "with" / "alignment_scores.tsv").read().split("\n")
    assert review[0].startswith("# file\tmin_posterior") and sorted(ln.split("\t")[0] for ln in review[1:-1]) == ["a.wav", "b.wav"]
    lines = open(tmp_path / "with" / "token_durations.tsv").read().split("\n")
    assert lines[0] == "file\t" + RP.REPORTS["durations"].header
    listed = [ln.split("\t") for ln in lines[1:-1]]
    assert len(listed) == sum(t in ("p00", "p01", "p02") for t in tr_a) and {r[0] for r in listed} == {"a.wav"}
    priors = [float(r[6]) for r in listed]
    assert priors == sorted(priors) and len(set(priors)) > 1          # (an order that says something: more than one value)
    assert sorted(tuple(r[1:]) for r in listed) == sorted(tuple(r) for r, t in zip(rows, tr_a) if t in ("p00", "p01", "p02"))


def test_label_files_returns_the_rows_and_one_file_gets_its_files(whisper, tmp_path, capsys):  # noqa: F811
    d, lab = whisper
    folder, tr_a, pr_path, prior = _folder(d, tmp_path)
    paths = [str(folder / n) for n in ("a.wav", "b.wav", "c.wav", "e.wav")]
    plain = lab.label_files(paths, confidence_threshold=CT, align="viterbi", duration_prior=pr_path)
    final, scores, durations = lab.label_files(paths, confidence_threshold=CT, align="viterbi", duration_prior=pr_path,
                                               duration_prior_scores=True)
    assert final == plain
    assert isinstance(scores[0], AL.FileScore) and isinstance(scores[1], AL.FileScore) and scores[2] is None and scores[3] is None
    assert durations[1] is None and durations[2] is None and durations[3] is None
    assert [r.token for r in durations[0]] == tr_a and all(isinstance(r, AL.TokenDuration) for r in durations[0])
    assert [r.posterior for r in durations[0]] == [t.posterior for t in scores[0].tokens]
    assert sum(r.frames for r in durations[0]) <= 350
    # the config key gives the same
    lab.config["postprocess"]["duration_prior"] = pr_path
    lab.config["postprocess"]["duration_prior_scores"] = True
    try:
        again = lab.label_files(paths[:1], confidence_threshold=CT, align="viterbi")
        assert again[0] == final[:1] and again[2][0] == durations[0]
    finally:
        lab.config["postprocess"].pop("duration_prior", None)
        lab.config["postprocess"].pop("duration_prior_scores", None)
    # infer_audio: the file's own two reports beside its .lab
    os.makedirs(tmp_path / "one")
    I.infer_audio(paths[0], config_path=str(d / "config.yaml"), checkpoint_path=str(d / "best_model.pt"),
                  output_lab_path=str(tmp_path / "one" / "a.lab"), confidence_threshold=CT, align="viterbi", duration_prior=pr_path, duration_prior_scores=True)
    assert sorted(os.listdir(tmp_path / "one")) == ["a.durations.tsv", "a.lab", "a.scores.tsv"]
    assert open(tmp_path / "one" / "a.durations.tsv").read() == RP.file_text("durations", durations[0])
    # the CLI flag reaches infer_folder; without a prior it is refused before a model is loaded
    seen = {}
    real = I.infer_folder
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(I, "infer_folder", lambda **k: (seen.update(k), real(**k))[1])
        args = [str(folder), "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml"), "--align", "viterbi", "-o",
                str(tmp_path / "cli")]
        with pytest.raises(SystemExit) as e:
            I.main(args + ["--duration-prior", pr_path, "--duration-prior-scores"])
        assert e.value.code == 0 and seen["duration_prior_scores"] is True
        assert os.path.exists(tmp_path / "cli" / "token_durations.tsv")
        mp.setattr(I, "_labeler", lambda *a, **k: pytest.fail("a model was loaded"))
        with pytest.raises(SystemExit) as e:
            I.main(args + ["--duration-prior-scores"])
        assert e.value.code == 2
