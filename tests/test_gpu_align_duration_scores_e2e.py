"""-m gpu: `postprocess.duration_scores` end to end on the synthetic tiny Whisper checkpoint of test_gpu_align_min_duration_e2e.py
(its fixtures and helpers, imported): beside a min_duration the option writes `{stem}.scores.tsv` and leaves the .lab alone, the
posteriors are those of the float64 forward-backward over the minimum-duration lattice on the logits the Labeler scored, a file whose
durations no path can meet is scored by the pass without them and one line says so, a folder gets its alignment_scores.tsv, and
align_scores beside a min_duration is refused as before."""
import os
import shutil

import numpy as np
import pytest

import duration_posterior_ref as DP
from test_gpu_align_e2e import _write_tr
from test_gpu_align_min_duration_e2e import CT, FD, _transcript, whisper  # noqa: F401  (whisper: the module's fixture)
from wfl_asr_amd import align as AL
from wfl_asr_amd import infer as I
from wfl_asr_amd.options import MIN_DURATION_SCORES_ERROR

pytestmark = pytest.mark.gpu


@pytest.fixture
def spy(monkeypatch):
    """Every duration_posteriors / alignment_posteriors call of the Labeler, with its inputs on the host."""
    calls = []

    def wrap(name):
        real = getattr(AL, name)

        def f(lg, n_frames, token_classes, gaps, o_id, tok, **kw):
            calls.append(dict(entry=name, z=lg.cpu().numpy(), n_frames=list(n_frames), alts=token_classes, gaps=gaps,
                              tok=tok.cpu().numpy(), offs=kw.get("frame_offsets"), packed=kw.get("packed")))
            return real(lg, n_frames, token_classes, gaps, o_id, tok, **kw)
        monkeypatch.setattr(AL, name, f)
    wrap("duration_posteriors")
    wrap("alignment_posteriors")
    return calls


def _rows(tsv_path):
    lines = open(tsv_path).read().split("\n")
    return lines[0], [ln.split("\t") for ln in lines[1:] if ln]


def _infer(d, wav, out, **kw):
    return I.infer_audio(wav, str(d / "config.yaml"), str(d / "best_model.pt"), str(out), confidence_threshold=CT, align="viterbi", **kw)


def test_the_option_writes_the_scores_of_the_duration_lattice(whisper, spy, tmp_path):
    d, lab = whisper
    wav = str(tmp_path / "a.wav")
    shutil.copyfile(str(d / "wavs" / "a.wav"), wav)
    tr = _transcript(90)
    _write_tr(wav, tr)
    _infer(d, wav, tmp_path / "x" / "a.lab", min_duration=0.06)
    assert os.listdir(tmp_path / "x") == ["a.lab"] and not spy
    _infer(d, wav, tmp_path / "y" / "a.lab", min_duration=0.06, duration_scores=True)
    assert sorted(os.listdir(tmp_path / "y")) == ["a.lab", "a.scores.tsv"]
    assert open(tmp_path / "x" / "a.lab", "rb").read() == open(tmp_path / "y" / "a.lab", "rb").read()
    # scored once, by the entry of the duration lattice, on the PackedClips of the search
    assert [c["entry"] for c in spy] == ["duration_posteriors"]
    call = spy[0]
    D = [3] * len(tr)
    assert call["packed"] is not None and call["packed"].d_min.cpu().numpy().tolist() == D and call["packed"].d_win is None
    T = call["n_frames"][0]
    z, tok = call["z"][:T], call["tok"][:T]
    r64 = DP.forward_backward(z, call["alts"][0], call["gaps"][0], D, tok=tok)
    r32 = DP.forward_backward(z, call["alts"][0], call["gaps"][0], D, tok=tok, dtype=np.float32)
    head, rows = _rows(tmp_path / "y" / "a.scores.tsv")
    # the header line gains nothing: the four figures of align_scores' file
    assert [f.split("=")[0] for f in head.split("\t")] == ["# path_log_posterior", "mean_frame_logprob", "mean_frame_logz", "min_posterior"]
    assert [r[2] for r in rows] == tr and all(len(r) == 6 for r in rows)
    lab_lines = [ln.split() for ln in open(tmp_path / "y" / "a.lab").read().split("\n") if ln]
    assert [r[:3] for r in rows] == lab_lines
    # the posteriors: 4 x the float32 restatement's deviation from float64 (half an fp32 ulp added where that exceeds it), and half a
    # unit of the sixth decimal the file prints
    post = np.array([float(r[3]) for r in rows])
    yard = float(np.abs(r32["tok_post"] - r64["tok_post"]).max())
    h = 0.5 * np.spacing(np.abs(r64["tok_post"]).astype(np.float32)).astype(np.float64)
    dev = np.abs(post - r64["tok_post"])
    print(f"tok_post: file {dev.max():.3e}, float32 restatement {yard:.3e}, allowed 4 x = {4 * yard:.3e} + 5e-7")
    assert (dev <= 4 * yard + np.where(yard < h, h, 0.0) + 0.5e-6).all()
    sd = np.array([float(r[4]) for r in rows])
    yard_sd = float(np.abs(r32["start_sd"] - r64["start_sd"]).max()) * FD
    print(f"start_sd_s: file {np.abs(sd - r64['start_sd'] * FD).max():.3e}, float32 restatement {yard_sd:.3e}")
    assert (np.abs(sd - r64["start_sd"] * FD) <= 4 * yard_sd + 0.5e-4 + 1e-9).all()
    assert post.min() < 0.9 and float(head.split("min_posterior=")[1]) == pytest.approx(post.min(), abs=1e-6)
    # label_files returns the scores as align_scores does
    segs, scores = lab.label_files([wav], confidence_threshold=CT, align="viterbi", min_duration=0.06, duration_scores=True)
    assert isinstance(scores[0], AL.FileScore) and [f"{t.posterior:.6f}" for t in scores[0].tokens] == [r[3] for r in rows]
    # align_scores beside a min_duration is still refused, with the old message
    with pytest.raises(ValueError) as e:
        lab.label_files([wav], align="viterbi", min_duration=0.06, align_scores=True)
    assert str(e.value) == MIN_DURATION_SCORES_ERROR
    with pytest.raises(ValueError, match="duration_scores needs a min_duration"):
        lab.label_files([wav], align="viterbi", duration_scores=True)


def test_a_file_without_its_durations_is_scored_by_the_plain_pass(whisper, spy, capsys):
    d, lab = whisper
    p = str(d / "wavs" / "plain.wav")
    tr = _transcript(59)                                  # 60 tokens of 4 frames at least in 4 s = 200 frames: no path
    plain_segs, plain_scores = _label_scored(lab, p, tr, align_scores=True)
    assert [c["entry"] for c in spy] == ["alignment_posteriors"]
    capsys.readouterr()
    segs, scores = _label_scored(lab, p, tr, min_duration=0.08, duration_scores=True)
    out = capsys.readouterr().out
    assert out.count(I.MIN_DURATION_INFEASIBLE) == 1 and out.count(I.DURATION_SCORES_PLAIN) == 1
    assert [c["entry"] for c in spy] == ["alignment_posteriors"] * 2 and spy[1]["packed"].d_min is None
    # searched without durations, scored on that lattice: the figures of align_scores for the same file
    assert segs == plain_segs and scores[0] == plain_scores[0] and isinstance(scores[0], AL.FileScore)


def _label_scored(lab, path, tr, **kw):
    _write_tr(path, tr)
    try:
        return lab.label_files([path], confidence_threshold=CT, align="viterbi", **kw)
    finally:
        os.remove(path.replace(".wav", ".txt"))


def test_a_folder_gets_its_review_list(whisper, tmp_path, capsys):
    d, lab = whisper
    folder = tmp_path / "in"
    os.makedirs(folder)
    shutil.copyfile(str(d / "wavs" / "a.wav"), str(folder / "f0.wav"))
    _write_tr(str(folder / "f0.wav"), _transcript(90))
    shutil.copyfile(str(d / "wavs" / "plain.wav"), str(folder / "f1.wav"))
    _write_tr(str(folder / "f1.wav"), _transcript(69))    # 70 tokens of 3 frames in 200: infeasible, scored without durations
    shutil.copyfile(str(d / "wavs" / "plain.wav"), str(folder / "f2.wav"))                                  # no transcript
    common = dict(confidence_threshold=CT, align="viterbi", min_duration=0.06)
    I.infer_folder(str(folder), str(d / "config.yaml"), str(d / "best_model.pt"), str(tmp_path / "ref"), **common)
    capsys.readouterr()
    I.infer_folder(str(folder), str(d / "config.yaml"), str(d / "best_model.pt"), str(tmp_path / "out"), duration_scores=True, **common)
    assert capsys.readouterr().out.count(I.DURATION_SCORES_PLAIN) == 1
    out = tmp_path / "out"
    assert sorted(os.listdir(tmp_path / "ref")) == ["f0.lab", "f1.lab", "f2.lab"]
    assert sorted(os.listdir(out)) == ["alignment_scores.tsv", "f0.lab", "f0.scores.tsv", "f1.lab", "f1.scores.tsv", "f2.lab"]
    for i in range(3):
        assert open(out / f"f{i}.lab", "rb").read() == open(tmp_path / "ref" / f"f{i}.lab", "rb").read()
    review = [ln.split("\t") for ln in open(out / "alignment_scores.tsv").read().split("\n") if ln and not ln.startswith("#")]
    assert sorted(r[0] for r in review) == ["f0.wav", "f1.wav"] and [float(r[1]) for r in review] == sorted(float(r[1]) for r in review)
    for r in review:
        assert f"min_posterior={r[1]}" in open(out / (r[0][:-4] + ".scores.tsv")).readline()
