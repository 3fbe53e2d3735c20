"""-m gpu: `postprocess.min_duration` end to end on the synthetic tiny Whisper checkpoint of test_gpu_align_e2e.py (random weights,
rebuilt here): a 7 s file gives the segments of the float64 constrained DP over the forward's own logits and every token of `tok` has its
rows, a per-name mapping constrains the named tokens alone, a 65 s file with a draft carries a run across a 30 s seam with both
constraints held, an infeasible request falls back with its message, the CLI flags reach infer_folder, and without the key nothing
changes."""
import os
import shutil

import numpy as np
import pytest
import torch

import synthetic as synth
import viterbi_min_ref as M
import viterbi_ref as V
from cases import tiny_whisper_config
from test_gpu_align_e2e import LABELS, _setup, _write_tr
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
    d = tmp_path_factory.mktemp("vm")
    cfg = tiny_whisper_config(enable_bilstm=False)
    cfg["model"]["encoder_arch"]["max_positions"] = 1500
    lab = _setup(d, cfg, 41)
    A.write_wav(str(d / "wavs" / "a.wav"), synth.make_clip(800, 16000 * 7, seed=41) * 0.9, 16000)
    A.write_wav(str(d / "wavs" / "long.wav"), synth.make_clip(801, 16000 * 65, seed=41) * 0.8, 16000)
    A.write_wav(str(d / "wavs" / "plain.wav"), synth.make_clip(802, 16000 * 4, seed=41) * 0.7, 16000)
    os.makedirs(d / "drafts")
    return d, lab


@pytest.fixture
def spy(monkeypatch):
    """Every viterbi_align call of the Labeler: its keyword arguments and its outputs on the host."""
    calls = []
    real = AL.viterbi_align

    def viterbi_align(*a, **kw):
        out = real(*a, **kw)
        calls.append(dict(kw, n_frames=list(a[1]), tok=out[1].cpu().numpy(), status=out[3].cpu().numpy()))
        return out
    monkeypatch.setattr(AL, "viterbi_align", viterbi_align)
    return calls


def _bytes(segs):
    return npost.format_lab_tuples(segs)


def _transcript(n, seed=7):
    """A transcript of its own (the weights are random: what the free decode hears does not matter here), SP spelled as a token, so no
    pause of the free decode joins the result: the .lab is the path's segments, one per token."""
    names = [str(x) for x in np.random.default_rng(seed).choice(["p00", "p01", "p02", "p03"], size=n)]
    return names[:n // 2] + ["SP"] + names[n // 2:]


def _label(lab, path, tr, **kw):
    _write_tr(path, tr)
    try:
        return lab.label_files([path], confidence_threshold=CT, align="viterbi", **kw)[0]
    finally:
        os.remove(path.replace(".wav", ".txt"))


def _host_reference(lab, path, tr, D):
    """The clip through model.label(want_logits=True) and the float64 DP with the minimum durations D (None: without), assembled by the
    host helpers (as test_gpu_align_e2e._host_reference is built) -> (segments, the path's run lengths)."""
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
    remap, names = lab._names_for(None)
    alts, why = AL.token_alternatives(tr, lab._table, remap, names, LABELS)
    assert why is None
    gaps = AL.gap_classes(LABELS, tr)
    states, _ = V.viterbi(z, alts, gaps) if D is None else M.viterbi(z, alts, gaps, D)
    assert states is not None
    ids, tok = V.outputs(states, z, alts, LABELS.index("O"))
    return AL.path_segments(ids, tok, [tv], [offs], [0.0], lab._table, alts, tr, FD), M.run_lengths(states, len(tr))


def _rows_per_token(tok, n):
    return np.bincount(tok[tok >= 0], minlength=n)


def test_a_min_duration_gives_the_host_constrained_dp(whisper, spy):
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    tr = _transcript(90)                                  # 91 tokens in 350 frames: the unconstrained optimum has short runs
    free_ref, free_runs = _host_reference(lab, path, tr, None)
    assert (free_runs < 3).sum() >= 5, "the unconstrained optimum has no short runs (test setup)"
    ref, runs = _host_reference(lab, path, tr, [3] * len(tr))
    assert (runs >= 3).all() and ref != free_ref
    got = _label(lab, path, tr, min_duration=0.06)
    assert got == ref
    assert len(spy) == 1 and spy[0]["min_frames"] == [[3] * len(tr)] and spy[0]["windows"] is None and spy[0]["status"][0] == 0
    assert (_rows_per_token(spy[0]["tok"], len(tr)) >= 3).all()          # every token of `tok` has at least 3 rows
    # the config key gives the same, and without the key the search and the .lab are as they were
    lab.config["postprocess"]["min_duration"] = 0.06
    try:
        assert _label(lab, path, tr) == ref
    finally:
        del lab.config["postprocess"]["min_duration"]
    plain = _label(lab, path, tr)
    assert plain == free_ref and spy[-1]["min_frames"] is None and _bytes(plain) != _bytes(ref)


def test_a_mapping_constrains_the_named_tokens_alone(whisper, spy):
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    tr = _transcript(90)
    D = [5 if t == "p01" else 1 for t in tr]
    assert AL.min_frames_for(tr, {"p01": 0.1}, FD) == D and 5 in D
    ref, runs = _host_reference(lab, path, tr, D)
    free_runs = _host_reference(lab, path, tr, None)[1]
    named = np.array(D) == 5
    assert (free_runs[named] < 5).any(), "the unconstrained optimum already meets the durations (test setup)"
    got = _label(lab, path, tr, min_duration={"p01": 0.1})
    assert got == ref
    rows = _rows_per_token(spy[-1]["tok"], len(tr))
    assert (rows[named] >= 5).all()
    assert (runs[~named] < 3).any()                       # (the others stay free: short runs remain among them)
    # with a default beside the name
    ref2, runs2 = _host_reference(lab, path, tr, [5 if t == "p01" else 2 for t in tr])
    assert _label(lab, path, tr, min_duration={"p01": 0.1, "default": 0.04}) == ref2 and (runs2 >= 2).all()


def test_a_long_file_with_a_draft_carries_a_run_across_the_seam(whisper, spy, capsys):
    d, lab = whisper
    long_p = str(d / "wavs" / "long.wav")
    names = ["p00", "p01", "p02", "p03"]
    # a draft by hand: a token every second from 0.5 s, the one at 29.5 s moved to 29.94 s: with 8 frames at least, a run that opens
    # within a frame of row 1497 crosses the seam at row 1500
    base = [((29.94 if k == 29 else 0.5 + k), 0.9 + k, names[k % 4] if k != 40 else "SP") for k in range(64)]
    tr = [s[2] for s in base]
    with open(str(d / "drafts" / "long.lab"), "wb") as f:
        f.write(_bytes(base))
    try:
        capsys.readouterr()
        opts = lab.options(align="viterbi", align_draft=str(d / "drafts"), draft_tolerance=0.02, min_duration=0.16)
        reports = RP.Reports.for_options(opts)
        got, _ = lab._label_scored([long_p], opts, None, CT, False, reports)
        moves = reports.moves
        out = capsys.readouterr().out
    finally:
        os.remove(str(d / "drafts" / "long.lab"))
    assert I.DRAFT_INFEASIBLE not in out and I.MIN_DURATION_INFEASIBLE not in out
    assert [s[2] for s in got[0]] == tr
    call = spy[-1]
    assert call["min_frames"] == [[8] * 64] and call["windows"] is not None and call["status"][0] == 0
    tok = call["tok"]
    assert (_rows_per_token(tok, 64) >= 8).all()          # the durations hold ...
    first = np.array([int(np.nonzero(tok == k)[0][0]) for k in range(64)])
    lo, hi = np.array(call["windows"][0]).T
    assert (first >= lo).all() and (first <= hi).all()    # ... and so do the windows
    assert tok[1499] == 29 and tok[1500] == 29            # one run either side of the seam between the chunks
    assert got[0][29][0] < 30.0 < got[0][29][1]
    assert max(abs(m.move_s) for m in moves[0]) <= 2 * FD + 1e-6


def test_an_infeasible_request_falls_back_with_its_message(whisper, spy, capsys, monkeypatch):
    d, lab = whisper
    p = str(d / "wavs" / "plain.wav")
    tr = _transcript(59)                                  # 60 tokens of 4 frames at least in 4 s = 200 frames: no path
    plain = _label(lab, p, tr)
    capsys.readouterr()
    got = _label(lab, p, tr, min_duration=0.08)
    assert capsys.readouterr().out.count(I.MIN_DURATION_INFEASIBLE) == 1
    assert got == plain and spy[-1]["min_frames"] is None                 # found on the host: the search ran without them
    # the safety net: were the host rule to miss it, the kernel's status 1 sends the clip to the search without durations all the same
    monkeypatch.setattr(AL, "windows_feasible", lambda *a: True)
    n = len(spy)
    got = _label(lab, p, tr, min_duration=0.08)
    assert capsys.readouterr().out.count(I.MIN_DURATION_INFEASIBLE) == 1 and got == plain
    assert len(spy) == n + 2 and spy[n]["status"][0] == AL.STATUS_INFEASIBLE and spy[n + 1].get("min_frames") is None


def test_the_cli_flags_reach_infer_folder_and_the_folder_gets_its_labs(whisper, tmp_path, monkeypatch):
    d, lab = whisper
    folder = tmp_path / "in"
    os.makedirs(folder)
    shutil.copyfile(str(d / "wavs" / "a.wav"), str(folder / "a.wav"))
    path = str(folder / "a.wav")
    tr = _transcript(90)
    ref = _label(lab, path, tr, min_duration={"p01": 0.1, "default": 0.06})
    plain = _label(lab, path, tr)
    seen = {}
    real = I.infer_folder

    def infer_folder(**kw):
        seen.update(kw)
        return real(**kw)
    monkeypatch.setattr(I, "infer_folder", infer_folder)
    _write_tr(path, tr)
    args = [str(folder), "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml"), "--align", "viterbi"]
    with pytest.raises(SystemExit) as e:
        I.main(args + ["-o", str(tmp_path / "out"), "--min-duration", "0.06", "--min-duration", "p01=0.1"])
    assert e.value.code == 0
    assert seen["min_duration"] == (("default", 0.06), ("p01", 0.1))
    assert open(tmp_path / "out" / "a.lab", "rb").read() == _bytes(ref)
    with pytest.raises(SystemExit) as e:                  # without the flag (and the key): the .lab it gets without the option
        I.main(args + ["-o", str(tmp_path / "out2")])
    assert e.value.code == 0 and seen["min_duration"] is None
    assert open(tmp_path / "out2" / "a.lab", "rb").read() == _bytes(plain) != _bytes(ref)
    # refused before a model is loaded: no --align viterbi, a value over the cap, a scoring pass beside it
    monkeypatch.setattr(I, "_labeler", lambda *a, **kw: pytest.fail("a model was loaded"))
    for extra in (["--align", "greedy", "--min-duration", "0.06"], ["--min-duration", "0.5"], ["--min-duration", "0.06", "--align-scores"]):
        with pytest.raises(SystemExit) as e:
            I.main(args + extra)
        assert e.value.code == 2
