"""-m gpu: `align_insertions` end to end on the synthetic tiny checkpoint of test_gpu_align_e2e.py (random weights): the segments, the
.lab bytes and the .edits.tsv bytes do not change, N + 1 rows of `{stem}.insertions.tsv` per aligned file, the rows equal a direct
align.insertion_scores call on the forward's own logits (the kernel against float64 is tests/test_gpu_align_insertions.py), with a
draft on the windowed lattice, the folder's `transcript_insertions.tsv`, and no file for a file without a transcript or one that fell
back to the greedy alignment.  A synthetic checkpoint carries no meaning, so nothing here asserts that a removed phoneme is found: the
kernel-level identity (inserting a deleted token again) is the proof of meaning."""
import os
import shutil

import numpy as np
import pytest
import torch

from test_gpu_align_e2e import LABELS, _core, _write_tr
from test_gpu_align_edits_e2e import CT, _transcript, whisper  # noqa: F401  (the fixture: the same checkpoint and clips)
from wfl_asr_amd import align as AL
from wfl_asr_amd import infer as I
from wfl_asr_amd import native_post as npost
from wfl_asr_amd import postprocess as pp
from wfl_asr_amd import reports as RP

pytestmark = pytest.mark.gpu


def _direct(lab, path, tr, segments, windows_of=None):
    """The clip through model.label(want_logits=True), then align.insertion_scores on those logits and the host's row builder -> the
    cells of the file's .insertions.tsv.  windows_of(tv): the start windows, for the windowed lattice."""
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
    logz, ins, st = AL.insertion_scores(lg, [tv], [alts], [gaps], LABELS.index("O"), pairs, packed=packed)
    assert int(st[0]) == 0 and ins.shape == (len(tr) + 1, len(pairs))
    rows = AL.place_insertions(ins.cpu().numpy(), segments, out_names)
    return [RP.REPORTS["insertions"].cells(r) for r in rows], out_names


def test_insertions_leave_segments_and_edits_alone_and_equal_a_direct_call(whisper):  # noqa: F811
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    tr = _transcript(14)
    _write_tr(path, tr)
    try:
        plain = lab.label_files([path], confidence_threshold=CT, align="viterbi")
        segs, ins = lab.label_files([path], confidence_threshold=CT, align="viterbi", align_insertions=True)
        _, edits = lab.label_files([path], confidence_threshold=CT, align="viterbi", align_edits=True)
        segs4, scores, edits4, ins4 = lab.label_files([path], confidence_threshold=CT, align="viterbi", align_scores=True,
                                                      align_edits=True, align_insertions=True)
        with pytest.raises(ValueError, match="align_insertions needs align='viterbi'"):
            lab.label_files([path], align="greedy", align_insertions=True)
    finally:
        os.remove(path.replace(".wav", ".txt"))
    assert segs == plain == segs4 and len(ins) == 1 and ins4 == ins and edits4 == edits and scores[0] is not None
    rows = ins[0]
    core = _core(segs[0])
    assert len(rows) == len(tr) + 1 and [r.index for r in rows] == list(range(len(tr) + 1))
    assert [r.before for r in rows] == tr + [""] and [r.after for r in rows] == [""] + tr
    assert [r.at_s for r in rows] == [core[0][0]] + [e for _, e, _ in core]
    want, out_names = _direct(lab, path, tr, core)
    assert [RP.REPORTS["insertions"].cells(r) for r in rows] == want
    for r in rows:
        assert r.best != r.second and r.best in out_names and r.second in out_names
        assert r.best_ratio >= r.second_ratio and r.flag == int(r.best_ratio > 0)
    print("ratios:", [(r.after, r.before, r.best, round(r.best_ratio, 2), r.flag) for r in rows])


def test_with_a_draft_the_windowed_lattice_is_the_one_scored(whisper):  # noqa: F811
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
        segs, ins = lab.label_files([path], confidence_threshold=CT, align="viterbi", align_insertions=True,
                                    align_draft=str(d / "drafts"), draft_tolerance=0.06)
    finally:
        os.remove(path.replace(".wav", ".txt"))
        if os.path.exists(str(d / "drafts" / "a.lab")):
            os.remove(str(d / "drafts" / "a.lab"))
    assert npost.format_lab_tuples(segs[0]) == npost.format_lab_tuples(base)
    windowed, _ = _direct(lab, path, tr, segs[0], lambda tv: AL.draft_windows(draft, [tv], [0.0], 0.06, pp.FRAME_DURATION))
    open_, _ = _direct(lab, path, tr, segs[0])
    got = [RP.REPORTS["insertions"].cells(r) for r in ins[0]]
    assert got == windowed
    assert got != open_                                   # (inside +-0.06 s windows fewer boundaries are summed: other ratios)


def test_folder_writes_the_insertion_files_and_the_flagged_rows_in_order(whisper, tmp_path, capsys):  # noqa: F811
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
    out, both, ed, ref = tmp_path / "out", tmp_path / "out_both", tmp_path / "out_edits", tmp_path / "out_plain"
    args = (str(folder), str(d / "config.yaml"), str(d / "best_model.pt"))
    capsys.readouterr()
    I.infer_folder(*args, str(out), confidence_threshold=CT, align="viterbi", align_insertions=True)
    said = capsys.readouterr().out
    I.infer_folder(*args, str(both), confidence_threshold=CT, align="viterbi", align_edits=True, align_insertions=True)
    I.infer_folder(*args, str(ed), confidence_threshold=CT, align="viterbi", align_edits=True)
    I.infer_folder(*args, str(ref), confidence_threshold=CT, align="viterbi")
    labs = [f"f{i}.lab" for i in range(5)]
    for name in labs:
        assert open(out / name, "rb").read() == open(ref / name, "rb").read() == open(both / name, "rb").read()
    # insertions beside the two aligned files only: none for the file without a transcript, none for the two that fell back (one
    # line each says so)
    ins_files = ["f0.insertions.tsv", "f1.insertions.tsv", "transcript_insertions.tsv"]
    assert sorted(os.listdir(out)) == sorted(labs + ins_files)
    assert sorted(os.listdir(both)) == sorted(os.listdir(ed) + ins_files)
    for name in ("f0.edits.tsv", "f1.edits.tsv", "transcript_edits.tsv"):
        assert open(both / name, "rb").read() == open(ed / name, "rb").read()
    for name in ins_files:
        assert open(both / name, "rb").read() == open(out / name, "rb").read()
    for i in (3, 4):
        assert said.count(f"f{i}.wav: no transcript insertions") == 1
    assert "f2.wav: no transcript insertions" not in said
    flagged = []
    for i in (0, 1):
        lines = open(out / f"f{i}.insertions.tsv").read().split("\n")
        assert lines[0] == RP.REPORTS["insertions"].header and lines[-1] == ""
        rows = [ln.split("\t") for ln in lines[1:-1]]
        n = len(trs[i])
        assert len(rows) == n + 1 and [int(r[0]) for r in rows] == list(range(n + 1))
        assert [r[2] for r in rows] == trs[i] + [""] and [r[1] for r in rows] == [""] + trs[i]
        lab_lines = [ln.split() for ln in open(out / f"f{i}.lab").read().split("\n") if ln and ln.split()[2] not in ("SP", "AP")]
        bounds = [int(lab_lines[0][0])] + [int(b) for _, b, _ in lab_lines]
        assert all(abs(float(r[3]) - b / 1e7) < 1.5e-7 for r, b in zip(rows, bounds))
        for r in rows:
            assert int(r[8]) == int(float(r[5]) > 0) and float(r[5]) >= float(r[7]) and r[4] != r[6]
        flagged += [[f"f{i}.wav"] + r for r in rows if r[8] == "1"]
    lines = open(out / "transcript_insertions.tsv").read().split("\n")
    assert lines[0] == "file\t" + RP.REPORTS["insertions"].header and lines[-1] == ""
    got = [ln.split("\t") for ln in lines[1:-1]]
    assert sorted(got) == sorted(flagged) and len(flagged) > 0, "no place is flagged (test setup)"
    best = [float(r[6]) for r in got]
    assert best == sorted(best, reverse=True)
