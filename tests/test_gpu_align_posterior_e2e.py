"""-m gpu: `align_scores` end to end on the synthetic tiny checkpoints of test_gpu_align_e2e.py (random weights; transcripts derived
from the free decode): the segments and .lab bytes do not change, one TokenScore per transcript token, the FileScore equals the host
float64 forward-backward over the forward's own logits (tolerance: 4 x the float32 restatement's deviation on the same logits, with
half an fp32 ulp of the value added only where that exceeds the restatement's deviation, as in test_gpu_align_posterior.py), long files, fall-backs, the folder's review list, WavLM ragged
clips."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import posterior_ref as P
import synthetic as synth
from cases import tiny_wavlm_config, tiny_whisper_config
from test_gpu_align_e2e import LABELS, ROOT, _core, _setup, _write_tr
from wfl_asr_amd import align as AL
from wfl_asr_amd import audio as A
from wfl_asr_amd import infer as I
from wfl_asr_amd import postprocess as pp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def whisper(tmp_path_factory):
    d = tmp_path_factory.mktemp("vs")
    cfg = tiny_whisper_config(enable_bilstm=False)
    cfg["model"]["encoder_arch"]["max_positions"] = 1500
    lab = _setup(d, cfg, 41)
    A.write_wav(str(d / "wavs" / "a.wav"), synth.make_clip(800, 16000 * 7, seed=41) * 0.9, 16000)
    A.write_wav(str(d / "wavs" / "long.wav"), synth.make_clip(801, 16000 * 65, seed=41) * 0.8, 16000)
    A.write_wav(str(d / "wavs" / "plain.wav"), synth.make_clip(802, 16000 * 4, seed=41) * 0.7, 16000)
    return d, lab


def _transcript(lab, path, n=40):
    free = lab.label_files([path], confidence_threshold=0.3, align="greedy")[0]
    names = [s[2] for s in free if s[2] in ("p00", "p01", "p02", "p03")]
    assert len(names) >= 1, "the free decode has no phoneme segment (test setup)"
    return names[:n] + ["p03", "p00", "p03"]            # (tokens the free decode does not have: some posteriors well below 1)


def _close(name, got, ref64, ref32):
    """|got - float64| <= 4 x the float32 restatement's maximum deviation from float64; half an fp32 ulp of the float64 value is added
    only where it exceeds that deviation (the outputs are fp32).  Prints before it asserts."""
    got, ref64, ref32 = (np.atleast_1d(np.asarray(x, np.float64)) for x in (got, ref64, ref32))
    yard = float(np.abs(ref32 - ref64).max())
    h = 0.5 * np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    d = np.abs(got - ref64)
    over = d - (4 * yard + np.where(yard < h, h, 0.0))
    print(f"{name}: kernel {float(d.max()):.3e}, float32 restatement {yard:.3e}, allowed 4 x = {4 * yard:.3e}, over by "
          f"{max(float(over.max()), 0.0):.3e}")
    assert over.max() <= 0, (name, float(d.max()), yard)


def _host_reference(lab, path, tr, dtype):
    """The clip through model.label(want_logits=True), wfl_align for the path, and the numpy forward-backward on those logits."""
    chunks = lab._load_chunks(path)
    assert len(chunks) == 1
    x = np.zeros((lab.batch_size, lab.chunk_samples), np.float32)
    x[0, :len(chunks[0])] = chunks[0]
    lens = np.zeros(lab.batch_size, np.int32)
    lens[0] = len(chunks[0])
    res = lab.model.label(torch.from_numpy(x).cuda(), None, threshold=0.3, lens=lens, average_languages=True, want_logits=True)
    tv = lab._valid_frames(len(chunks[0]), res.ids.shape[1])
    lg = res.logits[0, :tv].contiguous()
    remap, names = lab._names_for(None)
    alts, why = AL.token_alternatives(tr, lab._table, remap, names, LABELS)
    assert why is None
    gaps = AL.gap_classes(LABELS, tr)
    _, tok, score, st = AL.viterbi_align(lg, [tv], [alts], [gaps], LABELS.index("O"))
    assert int(st[0]) == 0
    z, tok = lg.cpu().numpy(), tok.cpu().numpy()
    r = P.forward_backward(z, alts, gaps, tok=tok, dtype=dtype)
    r["path_score"] = P.path_score(z, alts, gaps, tok)             # float64 score of wfl_align's own path
    return r, float(score[0]), tv


def test_scores_leave_the_segments_alone_and_equal_the_host_forward_backward(whisper):
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    tr = _transcript(lab, path)
    _write_tr(path, tr)
    try:
        plain = lab.label_files([path], confidence_threshold=0.3, align="viterbi")
        segs, scores = lab.label_files([path], confidence_threshold=0.3, align="viterbi", align_scores=True)
        r64, score, tv = _host_reference(lab, path, tr, np.float64)
        r32, _, _ = _host_reference(lab, path, tr, np.float32)
    finally:
        os.remove(path.replace(".wav", ".txt"))
    assert segs == plain and isinstance(segs, list) and len(scores) == 1
    fs = scores[0]
    core = _core(segs[0])
    assert [t.token for t in fs.tokens] == tr and [(t.start_s, t.end_s, t.token) for t in fs.tokens] == core
    fd = pp.FRAME_DURATION
    _close("tok_post", [t.posterior for t in fs.tokens], r64["tok_post"], r32["tok_post"])
    _close("start_sd", [t.start_sd_s / fd for t in fs.tokens], r64["start_sd"], r32["start_sd"])
    _close("start_mean", [t.start_shift_s / fd for t in fs.tokens], r64["start_mean"], r32["start_mean"])
    _close("logz", fs.mean_frame_logz * tv, r64["logz"], r32["logz"])
    assert fs.min_posterior == min(t.posterior for t in fs.tokens) and 0 <= fs.min_posterior <= 1
    assert fs.mean_frame_logprob == pytest.approx(score / tv, abs=1e-6)
    # logZ sums over every path, Viterbi's among them: logz >= the float64 score of that path, up to the logz tolerance
    yard = abs(r32["logz"] - r64["logz"])
    hz = 0.5 * float(np.spacing(np.float32(abs(r64["logz"]))))
    assert fs.mean_frame_logz * tv >= r64["path_score"] - (4 * yard + (hz if yard < hz else 0.0))
    # path_log_posterior is the difference of the two fp32 figures as returned
    assert fs.path_log_posterior == pytest.approx(fs.mean_frame_logprob * tv - fs.mean_frame_logz * tv, abs=2 * hz)


def test_long_file_fallbacks_and_files_without_transcript(whisper, capsys):
    d, lab = whisper
    long_p, plain_p, a_p = (str(d / "wavs" / n) for n in ("long.wav", "plain.wav", "a.wav"))
    rng = np.random.default_rng(2)
    tr = [str(x) for x in rng.choice(["p00", "p01", "p02", "p03"], size=120)]
    _write_tr(long_p, tr)
    _write_tr(a_p, ["p00", "zz", "p01"])             # a token that matches no phoneme: greedy for this file, with a message
    try:
        capsys.readouterr()
        plain = lab.label_files([long_p, plain_p, a_p], confidence_threshold=0.3, align="viterbi")
        out_plain = capsys.readouterr().out
        segs, scores = lab.label_files([long_p, plain_p, a_p], confidence_threshold=0.3, align="viterbi", align_scores=True)
        out = capsys.readouterr().out
    finally:
        os.remove(long_p.replace(".wav", ".txt"))
        os.remove(a_p.replace(".wav", ".txt"))
    assert segs == plain and out == out_plain and "'zz'" in out           # the existing message, nothing more
    assert scores[1] is None and scores[2] is None
    fs = scores[0]                                                          # several chunks, one search, one score over all tokens
    assert [t.token for t in fs.tokens] == tr
    assert [(t.start_s, t.end_s, t.token) for t in fs.tokens] == _core(segs[0])
    assert any(t.start_s < 30.0 for t in fs.tokens) and any(t.end_s > 60.0 for t in fs.tokens)
    assert all(0 <= t.posterior <= 1 + 1e-6 and t.start_sd_s >= 0 for t in fs.tokens)


def test_infeasible_falls_back_without_a_score(whisper, capsys):
    d, lab = whisper
    p = str(d / "wavs" / "plain.wav")
    _write_tr(p, ["p00"] * 400)                          # 4 s = 200 frames: fewer frames than tokens
    try:
        segs, scores = lab.label_files([p], confidence_threshold=0.3, align="viterbi", align_scores=True)
        assert "400 tokens for 200 frames" in capsys.readouterr().out and scores == [None]
        assert segs == lab.label_files([p], confidence_threshold=0.3, align="greedy")
        with pytest.raises(ValueError, match="align_scores"):
            lab.label_files([p], align="greedy", align_scores=True)
    finally:
        os.remove(p.replace(".wav", ".txt"))


def test_cli_and_folder_write_the_score_files(whisper, tmp_path):
    d, lab = whisper
    folder = tmp_path / "in"
    os.makedirs(folder)
    trs = {}
    for i, name in enumerate(("a.wav", "plain.wav")):
        src = str(d / "wavs" / name)
        shutil.copy(src, str(folder / f"f{i}.wav"))
        trs[i] = _transcript(lab, str(folder / f"f{i}.wav"), 12 if i == 0 else 4)
        _write_tr(str(folder / f"f{i}.wav"), trs[i])
    shutil.copy(str(d / "wavs" / "plain.wav"), str(folder / "f2.wav"))                                       # no transcript
    shutil.copy(str(d / "wavs" / "a.wav"), str(folder / "f3.wav"))
    _write_tr(str(folder / "f3.wav"), ["p00", "zz", "p01"])          # falls back to greedy: a token that matches no phoneme
    shutil.copy(str(d / "wavs" / "plain.wav"), str(folder / "f4.wav"))
    _write_tr(str(folder / "f4.wav"), ["p00"] * 400)                 # falls back to greedy: 400 tokens for 200 frames
    base = [sys.executable, os.path.join(ROOT, "infer.py"), str(folder / "f0.wav"), "-ckpt", str(d / "best_model.pt"), "-c",
            str(d / "config.yaml"), "--align", "viterbi"]
    r0 = subprocess.run(base + ["-o", str(tmp_path / "x" / "f0.lab")], capture_output=True, text=True, timeout=300)
    r1 = subprocess.run(base + ["-o", str(tmp_path / "y" / "f0.lab"), "--align-scores"], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    assert open(tmp_path / "x" / "f0.lab", "rb").read() == open(tmp_path / "y" / "f0.lab", "rb").read()
    assert not os.path.exists(tmp_path / "x" / "f0.scores.tsv")
    lab_lines = [ln.split() for ln in open(tmp_path / "y" / "f0.lab").read().split("\n") if ln and ln.split()[2] not in ("SP", "AP")]
    tsv = open(tmp_path / "y" / "f0.scores.tsv").read().split("\n")
    assert tsv[0].startswith("# path_log_posterior=")
    rows = [ln.split("\t") for ln in tsv[1:] if ln]
    assert [r[2] for r in rows] == trs[0] and [r[:3] for r in rows] == lab_lines
    r2 = subprocess.run(base + ["-o", str(tmp_path / "z" / "f0.lab"), "--align-scores", "--align", "greedy"], capture_output=True,
                        text=True, timeout=300)
    assert r2.returncode == 2
    r3 = subprocess.run([a if a != str(folder / "f0.wav") else str(folder / "f3.wav") for a in base]
                        + ["-o", str(tmp_path / "w" / "f3.lab"), "--align-scores"], capture_output=True, text=True, timeout=300)
    assert r3.returncode == 0, r3.stderr                             # a file that falls back: its .lab, the message, no scores file
    assert os.listdir(tmp_path / "w") == ["f3.lab"] and "'zz'" in r3.stdout
    out = tmp_path / "out"
    I.infer_folder(str(folder), str(d / "config.yaml"), str(d / "best_model.pt"), str(out), confidence_threshold=0.3, align="viterbi",
                   align_scores=True)
    ref = tmp_path / "out_plain"
    I.infer_folder(str(folder), str(d / "config.yaml"), str(d / "best_model.pt"), str(ref), confidence_threshold=0.3, align="viterbi")
    for i in range(5):
        assert open(out / f"f{i}.lab", "rb").read() == open(ref / f"f{i}.lab", "rb").read()
    # scores beside the two aligned files only: none for the file without a transcript, none for the two that fell back
    assert sorted(os.listdir(out)) == sorted([f"f{i}.lab" for i in range(5)] + ["f0.scores.tsv", "f1.scores.tsv", "alignment_scores.tsv"])
    assert sorted(os.listdir(ref)) == [f"f{i}.lab" for i in range(5)]
    review = [ln.split("\t") for ln in open(out / "alignment_scores.tsv").read().split("\n") if ln and not ln.startswith("#")]
    assert sorted(r[0] for r in review) == ["f0.wav", "f1.wav"]
    assert [float(r[1]) for r in review] == sorted(float(r[1]) for r in review)
    for r in review:
        head = open(out / (r[0][:-4] + ".scores.tsv")).readline()
        assert f"min_posterior={r[1]}" in head


def test_wavlm_ragged_clips_in_one_wave(tmp_path):
    lab = _setup(tmp_path, tiny_wavlm_config(False), 43)
    paths, trs = [], []
    for i, sec in enumerate((2.3, 3.7, 1.1)):
        p = str(tmp_path / "wavs" / f"w{i}.wav")
        A.write_wav(p, synth.make_clip(900 + i, int(16000 * sec), seed=43) * 0.8, 16000)
        tr = ["p00", "p01", "p02", "p03", "p01"][:2 + i]
        _write_tr(p, tr)
        paths.append(p)
        trs.append(tr)
    plain = lab.label_files(paths, confidence_threshold=0.0, align="viterbi")
    segs, scores = lab.label_files(paths, confidence_threshold=0.0, align="viterbi", align_scores=True)
    assert segs == plain
    for sg, fs, tr in zip(segs, scores, trs):
        assert [(t.start_s, t.end_s, t.token) for t in fs.tokens] == _core(sg) and [t.token for t in fs.tokens] == tr
        assert all(0 <= t.posterior <= 1 + 1e-6 for t in fs.tokens)
    alone = lab.label_files(paths[1:2], confidence_threshold=0.0, align="viterbi", align_scores=True)[1][0]
    assert alone == scores[1]                            # a clip alone equals the clip in the wave, bit for bit
