"""-m gpu: `postprocess.optional_scores` end to end on the synthetic tiny Whisper checkpoint of test_gpu_align_optional_e2e.py: the
.lab and the .skipped.tsv are the same with and without the option, {stem}.optional.tsv has one row per optional token of the
transcript, agrees with the .skipped.tsv and carries the posteriors of align.optional_posteriors called on the same logits, the folder
files are there and sorted, the option without optional_tokens is refused before a model is loaded, and a file that fell back to the
greedy alignment gets no score file and one line."""
import os
import shutil

import numpy as np
import pytest

from test_gpu_align_e2e import _write_tr
from test_gpu_align_min_duration_e2e import CT, _bytes, _transcript, whisper  # noqa: F401  (the module's fixture, built once here)
from wfl_asr_amd import align as AL
from wfl_asr_amd import infer as I
from wfl_asr_amd import reports as RP

pytestmark = pytest.mark.gpu


@pytest.fixture
def posterior_calls(monkeypatch):
    """Every optional_posteriors call of the Labeler: its outputs on the host."""
    calls = []
    real = AL.optional_posteriors

    def f(*a, **kw):
        out = real(*a, **kw)
        calls.append(dict(optional=a[5], skip_penalty=a[7], out=[x.cpu().numpy() for x in out]))
        return out
    monkeypatch.setattr(AL, "optional_posteriors", f)
    return calls


def _label(lab, path, tr, **kw):
    _write_tr(path, tr)
    try:
        return lab.label_files([path], confidence_threshold=CT, align="viterbi", **kw)
    finally:
        os.remove(path.replace(".wav", ".txt"))


def test_label_files_scores_the_decisions(whisper, posterior_calls):  # noqa: F811
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    tr = _transcript(90)
    flags = AL.optional_flags(tr, ["p01", "p03"])
    segs0, skipped0 = _label(lab, path, tr, optional_tokens=["p01", "p03"], skip_penalty=0.5)
    segs, scores, skipped, optional = _label(lab, path, tr, optional_tokens=["p01", "p03"], skip_penalty=0.5, optional_scores=True)
    assert segs == segs0 and skipped == skipped0 and skipped0[0], "the path skips no token (test setup)"
    rows, sc = optional[0], scores[0]
    assert [r.index for r in rows] == [k for k, f in enumerate(flags) if f] and all(r.token == tr[r.index] for r in rows)
    assert [r.index for r in rows if not r.kept] == [r.index for r in skipped[0]]
    # the posteriors are the entry's own, called by the Labeler on the forward's logits with the search's flags and penalty
    call = posterior_calls[-1]
    logz, keep, tok_post, _, _, st = call["out"]
    assert call["optional"] == [flags] and call["skip_penalty"] == 0.5 and st[0] == 0
    assert [r.keep_posterior for r in rows] == [float(keep[r.index]) for r in rows]
    assert all(0.0 <= r.keep_posterior <= 1.0 for r in rows)
    assert [r.doubt for r in rows] == [(r.keep_posterior if r.kept else 1.0 - r.keep_posterior) < 0.5 for r in rows]
    kept = [k for k in range(len(tr)) if k not in {r.index for r in skipped[0]}]
    assert isinstance(sc, AL.FileScore) and [t.token for t in sc.tokens] == [tr[k] for k in kept]
    assert [t.posterior for t in sc.tokens] == [float(tok_post[k]) for k in kept]
    assert sc.path_log_posterior <= 0.05 and np.isfinite(sc.path_log_posterior)      # the best path is one of the paths logZ sums
    # a mandatory token with mandatory neighbours is on every path
    lone = [k for k in range(1, len(tr) - 1) if not (flags[k - 1] or flags[k] or flags[k + 1])]
    assert lone and all(abs(float(keep[k]) - 1.0) < 1e-4 for k in lone)


def test_the_files_of_a_folder(whisper, tmp_path, monkeypatch, capsys):  # noqa: F811
    d, lab = whisper
    folder = tmp_path / "in"
    os.makedirs(folder)
    for name, src in (("a.wav", "a.wav"), ("b.wav", "a.wav"), ("short.wav", "plain.wav")):
        shutil.copyfile(str(d / "wavs" / src), str(folder / name))
    tr_a, tr_b, tr_s = _transcript(90), _transcript(60), _transcript(499)
    assert AL.min_frames_needed(AL.optional_flags(tr_s, ["p01", "p03"])) > 200     # short: 4 s = 200 frames, no path even with the skips
    for name, tr in (("a.wav", tr_a), ("b.wav", tr_b), ("short.wav", tr_s)):
        _write_tr(str(folder / name), tr)
    args = [str(folder), "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml"), "--align", "viterbi", "--optional", "p01",
            "--optional", "p03", "--skip-penalty", "0.5"]
    with pytest.raises(SystemExit) as e:
        I.main(args + ["-o", str(tmp_path / "without")])
    assert e.value.code == 0
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        I.main(args + ["-o", str(tmp_path / "with"), "--optional-scores"])
    out = capsys.readouterr().out
    assert e.value.code == 0
    w, wo = tmp_path / "with", tmp_path / "without"
    for f in sorted(os.listdir(wo)):                          # .lab, .skipped.tsv and skipped_tokens.tsv: byte for byte the same
        assert open(w / f, "rb").read() == open(wo / f, "rb").read(), f
    assert sorted(set(os.listdir(w)) - set(os.listdir(wo))) == ["a.optional.tsv", "a.scores.tsv", "alignment_scores.tsv", "b.optional.tsv",
                                                                 "b.scores.tsv", "optional_scores.tsv"]
    assert out.count("short.wav: no optional-token scores (the file was not Viterbi-aligned)") == 1
    for stem, tr in (("a", tr_a), ("b", tr_b)):
        rows = [ln.split("\t") for ln in open(w / f"{stem}.optional.tsv", encoding="utf-8").read().split("\n")[1:-1]]
        flags = AL.optional_flags(tr, ["p01", "p03"])
        assert [int(r[0]) for r in rows] == [k for k, f in enumerate(flags) if f]
        left_out = [ln.split("\t")[0] for ln in open(w / f"{stem}.skipped.tsv", encoding="utf-8").read().split("\n")[1:-1]]
        assert [r[0] for r in rows if r[2] == "skipped"] == left_out and all(r[2] in ("kept", "skipped") for r in rows)
        assert all((float(r[3]) if r[2] == "kept" else 1 - float(r[3])) < 0.5 for r in rows if r[6] == "1")
    lines = open(w / "optional_scores.tsv", encoding="utf-8").read().split("\n")
    assert lines[0] == "file\t" + RP.REPORTS["optional"].header and lines[-1] == ""
    body = [ln.split("\t") for ln in lines[1:-1]]
    conf = [float(r[4]) if r[3] == "kept" else 1.0 - float(r[4]) for r in body]
    assert {r[0] for r in body} == {"a.wav", "b.wav"} and all(x <= y + 1e-6 for x, y in zip(conf, conf[1:]))   # least confident first
    review = open(w / "alignment_scores.tsv", encoding="utf-8").read()
    assert "a.wav" in review and "b.wav" in review and "short.wav" not in review
    # refused before a model is loaded: the option without optional_tokens, and without the Viterbi alignment
    monkeypatch.setattr(I, "_labeler", lambda *a, **kw: pytest.fail("a model was loaded"))
    base = [str(folder), "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml")]
    for extra in (["--align", "viterbi", "--optional-scores"], ["--optional-scores"],
                  ["--align", "viterbi", "--optional", "p01", "--optional-scores", "--align-scores"]):
        with pytest.raises(SystemExit) as e:
            I.main(base + extra)
        assert e.value.code == 2


def test_without_the_key_nothing_is_scored(whisper, posterior_calls):  # noqa: F811
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    out = _label(lab, path, _transcript(90), optional_tokens=["p01"])
    assert len(out) == 2 and not posterior_calls                 # (segments, skipped) as before the option
