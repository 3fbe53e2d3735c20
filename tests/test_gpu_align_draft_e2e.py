"""-m gpu: `postprocess.align_draft` end to end on the synthetic tiny Whisper checkpoint of test_gpu_align_e2e.py (random weights,
rebuilt here): a draft equal to the unwindowed Viterbi .lab comes back byte for byte, a shifted draft gives the segments of the float64
windowed DP over the forward's own logits, a 65 s file's tokens find their chunk either side of the 30 s seams, an infeasible draft
falls back to the unwindowed alignment with a message, a file without a draft is labelled as without the option, and a folder gets
draft_moves.tsv through the CLI flags."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import synthetic as synth
import viterbi_ref as V
import viterbi_window_ref as W
from cases import tiny_whisper_config
from test_gpu_align_e2e import LABELS, ROOT, _setup, _write_tr
from wfl_asr_amd import align as AL
from wfl_asr_amd import audio as A
from wfl_asr_amd import infer as I
from wfl_asr_amd import native_post as npost
from wfl_asr_amd import postprocess as pp
from wfl_asr_amd import reports as RP

pytestmark = pytest.mark.gpu
FD = pp.FRAME_DURATION
CT = 0.3


@pytest.fixture(scope="module")
def whisper(tmp_path_factory):
    d = tmp_path_factory.mktemp("vd")
    cfg = tiny_whisper_config(enable_bilstm=False)
    cfg["model"]["encoder_arch"]["max_positions"] = 1500
    lab = _setup(d, cfg, 41)
    A.write_wav(str(d / "wavs" / "a.wav"), synth.make_clip(800, 16000 * 7, seed=41) * 0.9, 16000)
    A.write_wav(str(d / "wavs" / "long.wav"), synth.make_clip(801, 16000 * 65, seed=41) * 0.8, 16000)
    A.write_wav(str(d / "wavs" / "plain.wav"), synth.make_clip(802, 16000 * 4, seed=41) * 0.7, 16000)
    os.makedirs(d / "drafts")
    return d, lab


def _bytes(segs):
    return npost.format_lab_tuples(segs)


def _write_draft(d, name, segs):
    path = str(d / "drafts" / (name + ".lab"))
    with open(path, "wb") as f:
        f.write(_bytes(segs))
    return path


def _unwindowed(lab, path, tr):
    """The file's Viterbi alignment to `tr` as without the option.  tr spells SP, so no pause of the free decode joins the result:
    the .lab is the path's segments, one per token."""
    assert "SP" in tr
    _write_tr(path, tr)
    try:
        segs = lab.label_files([path], confidence_threshold=CT, align="viterbi")[0]
    finally:
        os.remove(path.replace(".wav", ".txt"))
    assert [s[2] for s in segs] == tr
    return segs


def _short_transcript(lab, path, n=12):
    """A transcript of its own (the weights are random: what the free decode hears does not matter here), SP spelled as a token."""
    names = [str(x) for x in np.random.default_rng(7).choice(["p00", "p01", "p02", "p03"], size=n)]
    return names[:n // 2] + ["SP"] + names[n // 2:]


def _host_reference(lab, path, draft, tol):
    """The clip through model.label(want_logits=True) and the float64 windowed DP inside the draft's windows, assembled by the host
    helpers (as test_gpu_align_e2e._host_reference is built) -> (segments, the path's start rows, the windows)."""
    chunks = lab._load_chunks(path)
    assert len(chunks) == 1
    x = np.zeros((lab.batch_size, lab.chunk_samples), np.float32)
    x[0, :len(chunks[0])] = chunks[0]
    lens = np.zeros(lab.batch_size, np.int32)
    lens[0] = len(chunks[0])
    res = lab.model.label(torch.from_numpy(x).cuda(), None, threshold=CT, lens=lens, average_languages=True, want_logits=True)
    tv = lab._valid_frames(len(chunks[0]), res.ids.shape[1])
    z = res.logits[0, :tv].cpu().numpy()
    offs = res.offsets[0, :tv].cpu().numpy()
    tr = [s[2] for s in draft]
    remap, names = lab._names_for(None)
    alts, why = AL.token_alternatives(tr, lab._table, remap, names, LABELS)
    assert why is None
    gaps = AL.gap_classes(LABELS, tr)
    wins = AL.draft_windows(draft, [tv], [0.0], tol, FD)
    states, _ = W.viterbi(z, alts, gaps, wins)
    if states is None:
        return None, None, wins
    ids, tok = V.outputs(states, z, alts, LABELS.index("O"))
    return AL.path_segments(ids, tok, [tv], [offs], [0.0], lab._table, alts, tr, FD), W.starts(states, len(tr)), wins


def _shifted_draft(lab, path, base):
    """`base` with a block of three tokens' starts 0.2 s later (or, where no such block leaves a path, earlier), the first block for
    which the windows at tolerance 0.06 s stay feasible (the float64 windowed DP of the host reference) -> (draft, block start, shift)."""
    for shift in (0.2, -0.2):
        for k in range(1, len(base) - 3):
            draft = [(max(s + shift, 0.0), e, ph) if k <= j < k + 3 else (s, e, ph) for j, (s, e, ph) in enumerate(base)]
            if all(abs(draft[j][0] - base[j][0]) > 0.19 for j in range(k, k + 3)) and _host_reference(lab, path, draft, 0.06)[0] is not None:
                return draft, k, shift
    pytest.fail("no block of three tokens can be moved 0.2 s in this file (test setup)")


def test_a_draft_equal_to_the_unwindowed_result_comes_back_byte_for_byte(whisper, capsys):
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    tr = _short_transcript(lab, path)
    base = _unwindowed(lab, path, tr)
    _write_draft(d, "a", base)
    capsys.readouterr()
    try:
        got = lab.label_files([path], confidence_threshold=CT, align="viterbi", align_draft=str(d / "drafts"), draft_tolerance=0.1)[0]
        assert "the draft wins" not in capsys.readouterr().out
        assert _bytes(got) == _bytes(base)
        # the default tolerance is 0.1 s; the draft wins over a .txt that spells something else, and says so
        _write_tr(path, ["p00", "p01"])
        got = lab.label_files([path], confidence_threshold=CT, align="viterbi", align_draft=str(d / "drafts"))[0]
        assert "the draft wins" in capsys.readouterr().out and _bytes(got) == _bytes(base)
        # the windowed posterior scores the same file: one TokenScore per draft token, nothing refused
        segs, scores = lab.label_files([path], confidence_threshold=CT, align="viterbi", align_scores=True,
                                       align_draft=str(d / "drafts"))
        assert _bytes(segs[0]) == _bytes(base) and [t.token for t in scores[0].tokens] == tr
        assert "no alignment scores" not in capsys.readouterr().out
    finally:
        os.remove(str(d / "drafts" / "a.lab"))
        if os.path.exists(path.replace(".wav", ".txt")):
            os.remove(path.replace(".wav", ".txt"))


def test_a_shifted_draft_gives_the_host_windowed_dp_and_an_infeasible_one_falls_back(whisper, capsys, monkeypatch):
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    tr = _short_transcript(lab, path)
    base = _unwindowed(lab, path, tr)
    draft, k, shift = _shifted_draft(lab, path, base)
    _write_draft(d, "a", draft)
    try:
        draft = AL.read_draft(str(d / "drafts" / "a.lab"))                       # (as the Labeler reads it: times truncated to 100 ns)
        ref, _, _ = _host_reference(lab, path, draft, 0.06)
        capsys.readouterr()
        got = lab.label_files([path], confidence_threshold=CT, align="viterbi", align_draft=str(d / "drafts"), draft_tolerance=0.06)[0]
        assert I.DRAFT_INFEASIBLE not in capsys.readouterr().out
        assert got == ref
        # 0.2 s are 10 frames, the tolerance 3: the moved tokens left their old starts, the way the draft went
        assert _bytes(got) != _bytes(base) and all((got[j][0] - base[j][0]) * shift > 0 for j in range(k, k + 3))
        # two starts on one frame, pinned: no path; the unwindowed alignment of the same transcript, with the message
        bad = list(base)
        bad[4] = (bad[3][0], bad[4][1], bad[4][2])
        _write_draft(d, "a", bad)
        got = lab.label_files([path], confidence_threshold=CT, align="viterbi", align_draft=str(d / "drafts"), draft_tolerance=0)[0]
        assert I.DRAFT_INFEASIBLE in capsys.readouterr().out
        assert _bytes(got) == _bytes(base)
        # the safety net: were the host rule to miss it, the kernel's status 1 sends the clip to the unwindowed search all the same
        monkeypatch.setattr(AL, "windows_feasible", lambda T, w: True)
        segs, scores = lab.label_files([path], confidence_threshold=CT, align="viterbi", align_draft=str(d / "drafts"), draft_tolerance=0,
                                       align_scores=True)
        out = capsys.readouterr().out
        assert out.count(I.DRAFT_INFEASIBLE) == 1 and "no alignment scores" not in out
        assert _bytes(segs[0]) == _bytes(base) and [t.token for t in scores[0].tokens] == tr
    finally:
        os.remove(str(d / "drafts" / "a.lab"))


def test_a_long_files_tokens_find_their_chunk_either_side_of_the_seams(whisper, capsys):
    d, lab = whisper
    long_p, plain_p = str(d / "wavs" / "long.wav"), str(d / "wavs" / "plain.wav")
    # a draft by hand: a token every second from 0.5 s to 63.5 s, so 30 of them before the first seam, 30 between the seams, 4 after
    names = ["p00", "p01", "p02", "p03"]
    base = [(0.5 + k, 0.9 + k, names[k % 4] if k != 40 else "SP") for k in range(64)]
    tr = [s[2] for s in base]
    assert sum(s[0] < 30.0 for s in base) == 30 and sum(30.0 < s[0] < 60.0 for s in base) == 30 and sum(s[0] > 60.0 for s in base) == 4
    plain = lab.label_files([plain_p], confidence_threshold=CT, align="viterbi")[0]
    _write_draft(d, "long", base)
    try:
        capsys.readouterr()
        opts = lab.options(align="viterbi", align_draft=str(d / "drafts"), draft_tolerance=0.1)
        reports = RP.Reports.for_options(opts)
        got, _ = lab._label_scored([plain_p, long_p], opts, None, CT, False, reports)
        moves = reports.moves
        assert I.DRAFT_INFEASIBLE not in capsys.readouterr().out
    finally:
        os.remove(str(d / "drafts" / "long.lab"))
    assert [s[2] for s in got[1]] == tr
    assert got[0] == plain                                           # the file without a draft, in the same call: as without the option
    # every token opens within 5 rows of the row its draft start maps to IN ITS CHUNK, and a start is written at (row + offset) frame
    # durations from the chunk's clock with an offset in (0, 1): at most 6 frame durations from the draft start.  A token sent to the
    # wrong chunk would be 30 s off.
    assert list(moves) == [1] and len(moves[1]) == len(tr)
    worst = max(abs(m.move_s) for m in moves[1])
    print(f"largest move {worst:.4f} s")
    assert worst <= 6 * FD + 1e-6
    assert [m.start_s for m in moves[1]] == [s[0] for s in got[1]]


def test_folder_through_the_cli_draft_moves_and_the_mixed_folder(whisper, tmp_path, monkeypatch):
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    tr = _short_transcript(lab, path)
    base = _unwindowed(lab, path, tr)
    draft, k, _ = _shifted_draft(lab, path, base)
    folder = tmp_path / "in"
    os.makedirs(folder)
    for n in ("a.wav", "plain.wav"):
        shutil.copyfile(str(d / "wavs" / n), str(folder / n))
    _write_draft(d, "a", draft)
    try:
        draft = AL.read_draft(str(d / "drafts" / "a.lab"))
        ref, starts, wins = _host_reference(lab, str(folder / "a.wav"), draft, 0.06)
        plain = lab.label_files([str(folder / "plain.wav")], confidence_threshold=CT)[0]
        r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), str(folder), "-ckpt", str(d / "best_model.pt"), "-c",
                            str(d / "config.yaml"), "-o", str(tmp_path / "out"), "--align", "viterbi", "--align-draft",
                            str(d / "drafts"), "--draft-tolerance", "0.06"], capture_output=True, text=True, timeout=300)
    finally:
        os.remove(str(d / "drafts" / "a.lab"))
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "out" / "a.lab", "rb").read() == _bytes(ref)
    assert open(tmp_path / "out" / "plain.lab", "rb").read() == _bytes(plain)           # no draft: the .lab it gets today
    rows = [ln.split("\t") for ln in open(tmp_path / "out" / "draft_moves.tsv").read().split("\n") if ln and not ln.startswith("#")]
    assert [r_[0] for r_ in rows] == ["a.wav"] * len(tr) and [int(r_[1]) for r_ in rows] == list(range(len(tr)))
    assert [r_[2] for r_ in rows] == tr
    on_edge = [int(s in (lo, hi)) for s, (lo, hi) in zip(starts, wins)]
    assert [int(r_[6]) for r_ in rows] == on_edge                    # exactly the tokens pressed against a window edge
    assert [int(r_[3]) for r_ in rows] == [I._lab_int(s[0]) for s in draft] and [int(r_[4]) for r_ in rows] == [I._lab_int(s[0]) for s in ref]
    assert all(float(r_[5]) == pytest.approx(g[0] - dr[0], abs=1e-4) for r_, g, dr in zip(rows, ref, draft))
    # --align-draft without --align viterbi: refused before a model is loaded
    monkeypatch.setattr(I, "_labeler", lambda *a, **kw: pytest.fail("a model was loaded"))
    with pytest.raises(SystemExit) as e:
        I.main([str(folder), "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml"), "--align-draft", str(d / "drafts")])
    assert e.value.code == 2
