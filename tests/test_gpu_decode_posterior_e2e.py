"""-m gpu: `decode_scores` end to end on a synthetic tiny Whisper checkpoint (30 s windows): the per-file and per-folder score files of
the grammar search's paths, their agreement with decode_posteriors called directly on the files' logits, one clip per long file, no
trace of the feature with the key absent, the argmax fallback, and both kinds of scores in one call of the CLI."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bio_viterbi_ref as R
import synthetic as synth
from cases import tiny_whisper_config
from test_gpu_decode_e2e import LABELS, _file_logits, _setup
from wfl_asr_amd import audio as A
from wfl_asr_amd import decode as DC
from wfl_asr_amd import infer as I
from wfl_asr_amd import postprocess as pp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = 2.0
NAMES = ("a.wav", "long.wav", "plain.wav")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("ds")
    cfg = tiny_whisper_config(enable_bilstm=False)
    cfg["model"]["encoder_arch"]["max_positions"] = 1500
    _setup(d, cfg, 41)
    A.write_wav(str(d / "wavs" / "a.wav"), synth.make_clip(800, 16000 * 7, seed=41) * 0.9, 16000)
    A.write_wav(str(d / "wavs" / "long.wav"), synth.make_clip(801, 16000 * 65, seed=41) * 0.8, 16000)
    A.write_wav(str(d / "wavs" / "plain.wav"), synth.make_clip(802, 16000 * 4, seed=41) * 0.7, 16000)
    cfg_path, ckpt = str(d / "config.yaml"), str(d / "best_model.pt")
    lab = I._labeler(cfg_path, ckpt, "cuda")               # the instance infer_audio / infer_folder use
    out = d / "out_on"
    I.infer_folder(str(d / "wavs"), cfg_path, ckpt, str(out), decode="viterbi", switch_penalty=LAM, decode_scores=True)
    return d, lab, cfg_path, ckpt, out


def _tsv(path):
    lines = open(path, encoding="utf-8").read().split("\n")
    assert lines[-1] == "" and lines[0].startswith("# ")
    head = lines[0][2:].split("\t")
    figures = dict(kv.split("=") for kv in head[:4])
    return figures, head[4], [ln.split("\t") for ln in lines[1:-1]]


def _direct(lab, path, lam):
    """The file's FreeScore from bio_viterbi + decode_posteriors called directly on the file's logits, and its path's segments."""
    table = DC.class_table(LABELS)
    z, cf, co, cc = _file_logits(lab, path, 0.0)
    lg = torch.from_numpy(z).cuda()
    ids, score, st = DC.bio_viterbi(lg, [len(z)], table, lam, 0.0)
    logz, post, cls, pst = DC.decode_posteriors(lg, [len(z)], table, lam, 0.0, ids)
    assert st.cpu().tolist() == [0] and pst.cpu().tolist() == [0]
    ids = ids.cpu().numpy()
    lse = float(R.prepass(z, 0.0)[0].sum())
    fs = DC.free_score(float(score[0]), float(logz[0]), lse, post.cpu().numpy(), cls.cpu().numpy(), ids, cf, co, cc, lab._table,
                       pp.FRAME_DURATION)
    return fs, DC.path_segments_free(ids, cf, co, cc, lab._table, pp.FRAME_DURATION), ids


def test_key_on_writes_the_score_files(world):
    d, lab, cfg_path, ckpt, out = world
    mins = {}
    for name in NAMES:
        stem = name[:-4]
        figures, counts, rows = _tsv(out / f"{stem}.decode_scores.tsv")
        assert list(figures) == ["path_log_posterior", "mean_frame_logprob", "legal_log_mass_per_frame", "min_posterior"]
        fs, (s, e, ph), _ = _direct(lab, str(d / "wavs" / name), LAM)
        n_lab = len(open(out / f"{stem}.lab").read().splitlines())
        assert counts == f"runs={len(s)} lab_lines={n_lab}" and len(rows) == len(s) == len(fs.runs) > 0
        for row, r, j in zip(rows, fs.runs, range(len(s))):          # run j of the scores is segment j of the path
            assert len(row) == 6
            assert [int(row[0]), int(row[1]), row[2]] == [I._lab_int(s[j]), I._lab_int(e[j]), lab._table.names[ph[j]]]
            assert (r.start_s, r.end_s) == (s[j], e[j])
            got = [float(x) for x in row[3:]]
            assert got == pytest.approx([r.posterior, r.start_posterior, r.min_frame_posterior], abs=2e-6)
            assert 0 <= got[1] <= got[0] + 1e-6 and got[2] <= got[0] + 1e-6 <= 1 + 2e-6
        assert float(figures["path_log_posterior"]) == pytest.approx(fs.path_log_posterior, abs=2e-2)
        assert float(figures["path_log_posterior"]) <= 1e-2
        assert float(figures["mean_frame_logprob"]) == pytest.approx(fs.mean_frame_logprob, abs=1e-4)
        assert float(figures["legal_log_mass_per_frame"]) == pytest.approx(fs.legal_log_mass_per_frame, abs=1e-4)
        assert float(figures["min_posterior"]) == pytest.approx(fs.min_posterior, abs=2e-6)
        mins[name] = float(figures["min_posterior"])
        assert not os.path.exists(out / f"{stem}.scores.tsv")
    review = open(out / "decode_scores.tsv").read().split("\n")
    assert review[0].startswith("# file\tmin_posterior") and review[-1] == "" and len(review) == 2 + len(NAMES)
    listed = [(r.split("\t")[0], float(r.split("\t")[1])) for r in review[1:-1]]
    assert listed == sorted(listed, key=lambda r: (r[1], r[0])) and dict(listed) == pytest.approx(mins)
    assert not os.path.exists(out / "alignment_scores.tsv")


def test_a_long_file_is_scored_as_one_clip(world, tmp_path):
    d, lab, cfg_path, ckpt, out = world
    table = DC.class_table(LABELS)
    p = str(d / "wavs" / "long.wav")
    z, cf, co, cc = _file_logits(lab, p, 0.0)
    assert cf[:2] == [1500, 1500] and len(cf) == 3
    kind = lab._table.kind
    lam = None
    for cand in (2.0, 1.0, 4.0, 0.5, 8.0, 0.0):
        ref, _ = R.viterbi(z, table, cand)
        if any(kind[ref[s]] == 2 for s in (1500, 3000)):      # I-p opens a chunk: the continuation of the run before
            lam = cand
            break
    assert lam is not None, "no run crosses a seam at any of the penalties tried (test setup)"
    seams = [30.0 * (i + 1) for i, s in enumerate((1500, 3000)) if kind[ref[s]] == 2]
    I.infer_audio(p, cfg_path, ckpt, str(tmp_path / "long.lab"), decode="viterbi", switch_penalty=lam, decode_scores=True)
    _, counts, rows = _tsv(tmp_path / "long.decode_scores.tsv")
    assert len(rows) == int((kind[ref] == 1).sum())           # a seam that cut a run in two would add a line
    for t in seams:
        assert sum(1 for r in rows if int(r[0]) < I._lab_int(t) < int(r[1])) == 1
    fs, _, ids = _direct(lab, p, lam)                          # the whole file as one clip, its logits concatenated
    assert (ids == ref).all() and len(fs.runs) == len(rows)
    assert [float(r[3]) for r in rows] == pytest.approx([r.posterior for r in fs.runs], abs=2e-6)


def test_key_absent_leaves_no_trace(world, tmp_path):
    d, lab, cfg_path, ckpt, out = world
    off = tmp_path / "out_off"
    I.infer_folder(str(d / "wavs"), cfg_path, ckpt, str(off), decode="viterbi", switch_penalty=LAM)
    for name in NAMES:
        assert open(off / (name[:-4] + ".lab"), "rb").read() == open(out / (name[:-4] + ".lab"), "rb").read()
    assert sorted(os.listdir(off)) == sorted(n[:-4] + ".lab" for n in NAMES)
    assert not glob.glob(str(off / "*decode_scores*"))
    # and the Labeler's return value keeps its shape
    paths = [str(d / "wavs" / n) for n in NAMES]
    plain = lab.label_files(paths, decode="viterbi", switch_penalty=LAM)
    segs, scores = lab.label_files(paths, decode="viterbi", switch_penalty=LAM, decode_scores=True)
    assert plain == segs and all(isinstance(sc, DC.FreeScore) for sc in scores)
    with pytest.raises(ValueError, match="no lattice to score"):
        lab.label_files(paths, decode_scores=True)


def test_a_file_that_falls_back_to_argmax_gets_no_scores(world, tmp_path, capsys):
    """A stub class table that uses one class twice makes wfl_decode report status 4 for every clip: no fault is provoked."""
    d, lab, cfg_path, ckpt, out = world
    capsys.readouterr()
    lab._decode_table = (LABELS.index("O"), [(0, 1), (0, 1)])
    try:
        I.infer_folder(str(d / "wavs"), cfg_path, ckpt, str(tmp_path / "fb"), decode="viterbi", switch_penalty=LAM, decode_scores=True)
    finally:
        lab._decode_table = None
    text = capsys.readouterr().out
    assert text.count("viterbi decode not possible (wfl_decode status 4); using the argmax decode") == len(NAMES)
    assert not glob.glob(str(tmp_path / "fb" / "*.decode_scores.tsv"))
    assert open(tmp_path / "fb" / "decode_scores.tsv").read().count("\n") == 1          # the review list: its header alone
    assert len(glob.glob(str(tmp_path / "fb" / "*.lab"))) == len(NAMES)


def test_both_kinds_of_scores_give_each_file_its_own(world, tmp_path):
    d, lab, cfg_path, ckpt, out = world
    folder = tmp_path / "mixed"
    os.makedirs(folder)
    for n in ("a.wav", "plain.wav"):
        A.write_wav(str(folder / n), A.load_clip(str(d / "wavs" / n), 16000), 16000)
    free = lab.label_files([str(folder / "a.wav")], decode="viterbi", switch_penalty=LAM)[0]
    names = [s[2] for s in free if s[2] not in ("SP", "AP")]
    assert len(names) >= 3, "the decode has too few segments (test setup)"
    with open(folder / "a.txt", "w") as f:
        f.write(" ".join(names[1:-1:2] or names[:1]))
    base = [sys.executable, os.path.join(ROOT, "infer.py"), str(folder), "-ckpt", ckpt, "-c", cfg_path, "-o", str(tmp_path / "both"), "-ct", "0"]
    r = subprocess.run(base + ["--align", "viterbi", "--align-scores", "--decode", "viterbi", "--switch-penalty", str(LAM),
                               "--decode-scores"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = sorted(os.listdir(tmp_path / "both"))
    assert got == ["a.lab", "a.scores.tsv", "alignment_scores.tsv", "decode_scores.tsv", "plain.decode_scores.tsv", "plain.lab"], got
    assert [ln.split("\t")[0] for ln in open(tmp_path / "both" / "alignment_scores.tsv").read().split("\n")[1:-1]] == ["a.wav"]
    assert [ln.split("\t")[0] for ln in open(tmp_path / "both" / "decode_scores.tsv").read().split("\n")[1:-1]] == ["plain.wav"]
    r = subprocess.run(base + ["--decode-scores"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "decode_scores needs decode='viterbi'" in r.stderr      # (a usage error, options.resolve's text)
