"""-m gpu: `align_edits` end to end on the synthetic tiny checkpoint of test_gpu_align_e2e.py (random weights): the segments and
.lab bytes do not change, one row of `{stem}.edits.tsv` per transcript token, the rows equal a direct align.edit_scores call on the
forward's own logits (the kernel against float64 is tests/test_gpu_align_edits.py), with a draft on the windowed lattice, the folder's
`transcript_edits.tsv`, and no file for a file that fell back to the greedy alignment."""
import os
import shutil

import numpy as np
import pytest
import torch

import synthetic as synth
from cases import tiny_whisper_config
from test_gpu_align_e2e import LABELS, _core, _setup, _write_tr
from wfl_asr_amd import align as AL
from wfl_asr_amd import audio as A
from wfl_asr_amd import infer as I
from wfl_asr_amd import native_post as npost
from wfl_asr_amd import postprocess as pp
from wfl_asr_amd import reports as RP

pytestmark = pytest.mark.gpu
CT = 0.3


@pytest.fixture(scope="module")
def whisper(tmp_path_factory):
    d = tmp_path_factory.mktemp("ve")
    cfg = tiny_whisper_config(enable_bilstm=False)
    cfg["model"]["encoder_arch"]["max_positions"] = 1500
    lab = _setup(d, cfg, 41)
    A.write_wav(str(d / "wavs" / "a.wav"), synth.make_clip(800, 16000 * 7, seed=41) * 0.9, 16000)
    A.write_wav(str(d / "wavs" / "plain.wav"), synth.make_clip(802, 16000 * 4, seed=41) * 0.7, 16000)
    os.makedirs(d / "drafts")
    return d, lab


def _transcript(n, seed=7, sp=False):
    names = [str(x) for x in np.random.default_rng(seed).choice(["p00", "p01", "p02", "p03"], size=n)]
    return names[:n // 2] + ["SP"] + names[n // 2:] if sp else names


def _direct(lab, path, tr, segments, windows_of=None):
    """The clip through model.label(want_logits=True), then align.edit_scores on those logits and the host's row builder -> the
    cells of the file's .edits.tsv.  windows_of(tv): the start windows, for the windowed lattice."""
    chunks = lab._load_chunks(path)
    assert len(chunks) == 1
    x = np.zeros((lab.batch_size, lab.chunk_samples), np.float32)
    x[0, :len(chunks[0])] = chunks[0]
    lens = np.zeros(lab.batch_size, np.int32)
    lens[0] = len(chunks[0])
    res = lab.model.label(torch.from_numpy(x).cuda(), None, threshold=CT, lens=lens, average_languages=True, want_logits=True)
    tv = lab._valid_frames(len(chunks[0]), res.ids.shape[1])
    lg = res.logits[0, :tv].contiguous()
    remap, names = lab._names_for(None)
    alts, why = AL.token_alternatives(tr, lab._table, remap, names, LABELS)
    assert why is None
    gaps = AL.gap_classes(LABELS, tr)
    sub_names, pairs = AL.substitute_table(LABELS)
    out_names = AL.substitute_output_names(sub_names, lab._table, remap, names)
    packed = AL.pack_clips(lg, [tv], [alts], [gaps], windows=None if windows_of is None else [windows_of(tv)])
    logz, edits, st = AL.edit_scores(lg, [tv], [alts], [gaps], LABELS.index("O"), pairs, packed=packed)
    assert int(st[0]) == 0 and edits.shape == (len(tr), len(pairs) + 1)
    rows = AL.token_edits(edits.cpu().numpy(), segments, out_names)
    return [RP.REPORTS["edits"].cells(r) for r in rows], out_names


def test_edits_leave_the_segments_alone_and_equal_a_direct_call(whisper, capsys):
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    tr = _transcript(14)
    _write_tr(path, tr)
    try:
        plain = lab.label_files([path], confidence_threshold=CT, align="viterbi")
        segs, edits = lab.label_files([path], confidence_threshold=CT, align="viterbi", align_edits=True)
        segs3, scores, edits3 = lab.label_files([path], confidence_threshold=CT, align="viterbi", align_scores=True, align_edits=True)
        with pytest.raises(ValueError, match="align_edits needs align='viterbi'"):
            lab.label_files([path], align="greedy", align_edits=True)
    finally:
        os.remove(path.replace(".wav", ".txt"))
    assert segs == plain == segs3 and len(edits) == 1 and edits3 == edits and scores[0] is not None
    rows = edits[0]
    core = _core(segs[0])
    assert [(r.start_s, r.end_s, r.token) for r in rows] == core and [r.token for r in rows] == tr
    assert [r.index for r in rows] == list(range(len(tr)))
    want, out_names = _direct(lab, path, tr, core)
    assert [RP.REPORTS["edits"].cells(r) for r in rows] == want
    for r in rows:                                        # a token's own name is never its substitute; best and second differ
        assert r.best != r.token and r.second != r.token and r.best != r.second and r.best in out_names and r.second in out_names
        assert r.best_ratio >= r.second_ratio and r.flag == int(max(r.best_ratio, r.deletion_ratio) > 0)
    print("ratios:", [(r.token, r.best, round(r.best_ratio, 2), round(r.deletion_ratio, 2), r.flag) for r in rows])


def test_with_a_draft_the_windowed_lattice_is_the_one_scored(whisper):
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    tr = _transcript(12, sp=True)
    _write_tr(path, tr)
    try:
        base = lab.label_files([path], confidence_threshold=CT, align="viterbi")[0]
        assert [s[2] for s in base] == tr
        with open(str(d / "drafts" / "a.lab"), "wb") as f:
            f.write(npost.format_lab_tuples(base))
        draft = AL.read_draft(str(d / "drafts" / "a.lab"))
        segs, edits = lab.label_files([path], confidence_threshold=CT, align="viterbi", align_edits=True,
                                      align_draft=str(d / "drafts"), draft_tolerance=0.06)
    finally:
        os.remove(path.replace(".wav", ".txt"))
        if os.path.exists(str(d / "drafts" / "a.lab")):
            os.remove(str(d / "drafts" / "a.lab"))
    assert npost.format_lab_tuples(segs[0]) == npost.format_lab_tuples(base)
    windowed, _ = _direct(lab, path, tr, segs[0], lambda tv: AL.draft_windows(draft, [tv], [0.0], 0.06, pp.FRAME_DURATION))
    open_, _ = _direct(lab, path, tr, segs[0])
    got = [RP.REPORTS["edits"].cells(r) for r in edits[0]]
    assert got == windowed
    assert got != open_                                   # (inside +-0.06 s windows fewer boundaries are summed: other ratios)


def test_folder_writes_the_edit_files_and_the_flagged_rows_in_order(whisper, tmp_path, capsys):
    d, lab = whisper
    folder = tmp_path / "in"
    os.makedirs(folder)
    trs = {0: _transcript(12, 3), 1: _transcript(5, 4)}
    for i, name in enumerate(("a.wav", "plain.wav")):
        shutil.copy(str(d / "wavs" / name), str(folder / f"f{i}.wav"))
        _write_tr(str(folder / f"f{i}.wav"), trs[i])
    shutil.copy(str(d / "wavs" / "plain.wav"), str(folder / "f2.wav"))                                       # no transcript
    shutil.copy(str(d / "wavs" / "a.wav"), str(folder / "f3.wav"))
    _write_tr(str(folder / "f3.wav"), ["p00", "zz", "p01"])          # falls back to greedy: a token that matches no phoneme
    shutil.copy(str(d / "wavs" / "plain.wav"), str(folder / "f4.wav"))
    _write_tr(str(folder / "f4.wav"), ["p00"] * 400)                 # falls back to greedy: 400 tokens for 200 frames
    out, ref = tmp_path / "out", tmp_path / "out_plain"
    capsys.readouterr()
    I.infer_folder(str(folder), str(d / "config.yaml"), str(d / "best_model.pt"), str(out), confidence_threshold=CT, align="viterbi",
                   align_edits=True)
    said = capsys.readouterr().out
    I.infer_folder(str(folder), str(d / "config.yaml"), str(d / "best_model.pt"), str(ref), confidence_threshold=CT, align="viterbi")
    for i in range(5):
        assert open(out / f"f{i}.lab", "rb").read() == open(ref / f"f{i}.lab", "rb").read()
    # edits beside the two aligned files only: none for the two that fell back (one line each says so)
    assert sorted(os.listdir(out)) == sorted([f"f{i}.lab" for i in range(5)] + ["f0.edits.tsv", "f1.edits.tsv", "transcript_edits.tsv"])
    assert sorted(os.listdir(ref)) == [f"f{i}.lab" for i in range(5)]
    for i in (3, 4):
        assert said.count(f"f{i}.wav: no transcript edits") == 1
    flagged = []
    for i in (0, 1):
        lines = open(out / f"f{i}.edits.tsv").read().split("\n")
        assert lines[0] == RP.REPORTS["edits"].header and lines[-1] == ""
        rows = [ln.split("\t") for ln in lines[1:-1]]
        assert [r[1] for r in rows] == trs[i] and [int(r[0]) for r in rows] == list(range(len(trs[i])))
        lab_lines = [ln.split() for ln in open(out / f"f{i}.lab").read().split("\n") if ln and ln.split()[2] not in ("SP", "AP")]
        assert [r[1] for r in rows] == [ph for _, _, ph in lab_lines]
        assert all(abs(float(r[2]) - int(a) / 1e7) < 1.5e-7 and abs(float(r[3]) - int(b) / 1e7) < 1.5e-7 for r, (a, b, _) in zip(rows, lab_lines))
        for r in rows:
            assert int(r[9]) == int(max(float(r[5]), float(r[7]), float(r[8])) > 0)
        flagged += [[f"f{i}.wav"] + r for r in rows if r[9] == "1"]
    lines = open(out / "transcript_edits.tsv").read().split("\n")
    assert lines[0] == "file\t" + RP.REPORTS["edits"].header and lines[-1] == ""
    got = [ln.split("\t") for ln in lines[1:-1]]
    assert sorted(got) == sorted(flagged) and len(flagged) > 0, "no token is flagged (test setup)"
    largest = [max(float(r[6]), float(r[8]), float(r[9])) for r in got]
    assert largest == sorted(largest, reverse=True)
