"""-m gpu: `postprocess.filler_token` end to end on the synthetic tiny Whisper checkpoint of test_gpu_align_min_duration_e2e.py
(random weights, rebuilt here): a 7 s file whose transcript has one filler gives the token segments of the float64 DP with the filler
emission over the forward's own logits, the filler's span holds the file's own free segments clipped to it and .fillers.tsv lists
it; without the key the same .txt falls back to the greedy alignment as it always did; a file without a filler is searched by
viterbi_align alone and gives the same bytes; the config key and the CLI flags reach infer_folder; a 65 s file carries a filler across
the 30 s seam as one span; adjacent fillers are collapsed; a filler_token that is a label-set name is refused by name."""
import os
import shutil

import numpy as np
import pytest
import torch

import viterbi_filler_ref as R
from test_gpu_align_e2e import LABELS, _write_tr
from test_gpu_align_min_duration_e2e import CT, FD, _bytes, _transcript, whisper  # noqa: F401  (the module's fixture, built once here)
from wfl_asr_amd import align as AL
from wfl_asr_amd import infer as I
from wfl_asr_amd import reports as RP

pytestmark = pytest.mark.gpu
F = "<unk>"


@pytest.fixture
def spy(monkeypatch):
    """Every search call of the Labeler, by entry, with its outputs on the host; and the free segments of every file of a wave."""
    calls = []

    def wrap(name):
        real = getattr(AL, name)

        def f(*a, **kw):
            out = real(*a, **kw)
            rec = dict(kw, entry=name, n_frames=list(a[1]), tok=out[1].cpu().numpy(), ids=out[0].cpu().numpy(), status=out[3].cpu().numpy())
            if name == "viterbi_align_filler":
                rec.update(fillers=a[5], filler_penalty=a[6])
            calls.append(rec)
            return out
        monkeypatch.setattr(AL, name, f)
    wrap("viterbi_align")
    wrap("viterbi_align_filler")
    wrap("viterbi_align_optional")
    real_plans = I.Labeler._greedy_and_plans

    def plans(self, *a, **kw):
        out = real_plans(self, *a, **kw)
        calls.append(dict(entry="free", free_segs=dict(out[1])))
        return out
    monkeypatch.setattr(I.Labeler, "_greedy_and_plans", plans)
    return calls


def _label(lab, path, tr, **kw):
    _write_tr(path, tr)
    try:
        out = lab.label_files([path], confidence_threshold=CT, align="viterbi", **kw)
    finally:
        os.remove(path.replace(".wav", ".txt"))
    return (out[0][0], out[1][0]) if isinstance(out, tuple) else (out[0], None)


def _with_filler(tr):
    """The 91-token transcript with tokens 30 .. 44 replaced by one filler."""
    return tr[:30] + [F] + tr[45:]


def _host_reference(lab, path, tr, phi):
    """The clip through model.label(want_logits=True) and the float64 DP with the filler emission, assembled by the host helpers ->
    (one span per token, the filler's among them; the DP's tok)."""
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
    alts, why = AL.token_alternatives(tr, lab._table, remap, names, LABELS, filler=F)
    assert why is None
    fill = AL.filler_flags(tr, F)
    states, _ = R.viterbi(z, alts, AL.gap_classes(LABELS, tr), fill, phi)
    assert states is not None
    ids, tok = R.outputs(states, z, alts, LABELS.index("O"), fill)
    return AL.path_segments(ids, tok, [tv], [offs], [0.0], lab._table, alts, tr, FD, fillers=fill), tok


def test_a_filler_gives_the_host_dp_and_holds_the_free_segments(whisper, spy, capsys):  # noqa: F811
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    tr = _with_filler(_transcript(90))
    assert len(tr) == 77 and tr.count(F) == 1 and tr[30] == F and "SP" in tr
    spans, rtok = _host_reference(lab, path, tr, 1.0)
    assert [s[2] for s in spans] == tr
    capsys.readouterr()
    got, fillers = _label(lab, path, tr, filler_token=F)
    out = capsys.readouterr().out
    call = [c for c in spy if c["entry"] != "free"][-1]
    free = [c for c in spy if c["entry"] == "free"][-1]["free_segs"][0]
    assert call["entry"] == "viterbi_align_filler" and call["fillers"] == [AL.filler_flags(tr, F)] and call["filler_penalty"] == 1.0
    assert call["status"][0] == 0 and (call["tok"] == rtok).all()
    assert "1 filler in the transcript" in out and "using the greedy alignment" not in out
    # every other token has its one segment, the reference's; the filler's span holds the free segments that overlap it, clipped
    a, b = spans[30][:2]
    held = [(max(s, a), min(e, b), ph) for s, e, ph in free if min(e, b) > max(s, a)]
    assert got == spans[:30] + held + spans[31:]
    assert all(a <= s < e <= b for s, e, _ in held) and held == AL.filler_segments(spans[30], free)
    assert all(x[1] <= y[0] + 1e-9 for x, y in zip(got, got[1:]))
    assert fillers == [AL.FillerSpan(30, a, b, int((rtok == 30).sum()), tuple(ph for _, _, ph in held))] and fillers[0].frames >= 1
    assert RP.file_text("fillers", fillers).count("\n") == 2
    # a larger price: the reference's again, and a shorter (or equal) run
    spans5, rtok5 = _host_reference(lab, path, tr, 5.0)
    got5, fillers5 = _label(lab, path, tr, filler_token=F, filler_penalty=5.0)
    assert got5 == spans5[:30] + AL.filler_segments(spans5[30], free) + spans5[31:]
    assert fillers5[0].frames == int((rtok5 == 30).sum()) <= fillers[0].frames
    # without the key: the same .txt falls back to the greedy alignment, as it always did
    capsys.readouterr()
    n = len(spy)
    plain, nothing = _label(lab, path, tr)
    out = capsys.readouterr().out
    assert nothing is None and f"viterbi alignment not possible (token {F!r} matches no phoneme of the label set); using the greedy alignment" in out
    assert [c["entry"] for c in spy[n:] if c["entry"] != "free"] == []
    # a filler_token that is an output name of the label set is refused by name
    with pytest.raises(ValueError, match="filler_token: 'p01' is an output name"):
        _label(lab, path, tr, filler_token="p01")


def test_a_file_without_a_filler_is_searched_as_ever(whisper, spy):  # noqa: F811
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    tr = _transcript(90)
    plain, _ = _label(lab, path, tr)
    n = len(spy)
    got, fillers = _label(lab, path, tr, filler_token=F, filler_penalty=0.5)
    assert _bytes(got) == _bytes(plain) and got == plain and fillers is None
    assert [c["entry"] for c in spy[n:] if c["entry"] != "free"] == ["viterbi_align"]


def test_the_config_key_and_the_cli_flags_reach_infer_folder(whisper, tmp_path, monkeypatch):  # noqa: F811
    d, lab = whisper
    folder = tmp_path / "in"
    os.makedirs(folder)
    shutil.copyfile(str(d / "wavs" / "a.wav"), str(folder / "a.wav"))
    path = str(folder / "a.wav")
    tr = _with_filler(_transcript(90))
    ref, fillers = _label(lab, path, tr, filler_token=F, filler_penalty=0.5)
    assert len(fillers) == 1
    seen = {}
    real = I.infer_folder

    def infer_folder(**kw):
        seen.clear()
        seen.update(kw)
        return real(**kw)
    monkeypatch.setattr(I, "infer_folder", infer_folder)
    _write_tr(path, tr)
    args = [str(folder), "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml"), "--align", "viterbi"]
    with pytest.raises(SystemExit) as e:
        I.main(args + ["-o", str(tmp_path / "out"), "--filler-token", F, "--filler-penalty", "0.5"])
    assert e.value.code == 0 and seen["filler_token"] == F and seen["filler_penalty"] == 0.5
    assert open(tmp_path / "out" / "a.lab", "rb").read() == _bytes(ref)
    want = RP.file_text("fillers", fillers)
    assert open(tmp_path / "out" / "a.fillers.tsv", encoding="utf-8").read() == want and want.count("\n") == 2
    assert open(tmp_path / "out" / "filler_spans.tsv", encoding="utf-8").read() == RP.folder_text("fillers", [("a.wav", fillers)])
    assert sorted(os.listdir(tmp_path / "out")) == ["a.fillers.tsv", "a.lab", "filler_spans.tsv"]
    with pytest.raises(SystemExit) as e:                  # the default price
        I.main(args + ["-o", str(tmp_path / "out1"), "--filler-token", F])
    assert e.value.code == 0 and seen["filler_token"] == F and seen["filler_penalty"] == 1.0
    with pytest.raises(SystemExit) as e:                  # without the flags (and the keys): the greedy fallback, no new file
        I.main(args + ["-o", str(tmp_path / "out2")])
    assert e.value.code == 0 and seen["filler_token"] is None and seen["filler_penalty"] is None
    assert sorted(os.listdir(tmp_path / "out2")) == ["a.lab"]
    lab.config["postprocess"].update(filler_token=F, filler_penalty=0.5)                     # the keys from the config
    try:
        os.remove(path.replace(".wav", ".txt"))
        assert _label(lab, path, tr) == (ref, fillers)
    finally:
        del lab.config["postprocess"]["filler_token"], lab.config["postprocess"]["filler_penalty"]
    # refused before a model is loaded
    monkeypatch.setattr(I, "_labeler", lambda *a, **kw: pytest.fail("a model was loaded"))
    for extra in (["--align", "greedy", "--filler-token", F], ["--filler-penalty", "1"], ["--filler-token", F, "--align-scores"],
                  ["--filler-token", F, "--min-duration", "0.06"], ["--filler-token", F, "--filler-penalty", "-1"],
                  ["--filler-token", F, "--optional", "p01"]):
        with pytest.raises(SystemExit) as e:
            I.main(args + extra)
        assert e.value.code == 2


def test_a_filler_across_the_30_s_seam_is_one_span(whisper, spy):  # noqa: F811
    """At a price of 0 a filler is never worse than any other state, so with two tokens either side it takes nearly the whole file."""
    d, lab = whisper
    long_p = str(d / "wavs" / "long.wav")
    tr = ["p00", "p01", F, "p02", "p03"]
    got, fillers = _label(lab, long_p, tr, filler_token=F, filler_penalty=0.0)
    call = [c for c in spy if c["entry"] != "free"][-1]
    free = [c for c in spy if c["entry"] == "free"][-1]["free_segs"][0]
    tok = call["tok"]
    assert call["entry"] == "viterbi_align_filler" and call["status"][0] == 0 and 3200 <= call["n_frames"][0] <= 3250
    assert tok[1499] == tok[1500] == 2 and tok[2999] == tok[3000] == 2, "the filler does not span the seams (test setup)"
    assert len(fillers) == 1 and fillers[0].index == 2 and fillers[0].frames == int((tok == 2).sum())
    a, b = fillers[0].start_s, fillers[0].end_s
    assert a < 30.0 < 60.0 < b <= 65.0 + 1e-6
    run = np.nonzero(tok == 2)[0]
    assert abs(a - run[0] * FD) <= 2 * FD and abs(b - (run[-1] + 1) * FD) <= 2 * FD        # one span, on the file's clock
    held = AL.filler_segments((a, b, F), free)
    assert held and fillers[0].names == tuple(s[2] for s in held)
    plain = [s for s in got if s not in held]
    assert [s[2] for s in plain if s[2] not in ("SP", "AP")] == ["p00", "p01", "p02", "p03"]
    # nothing overlaps: the tokens lie outside the span, what the span holds inside it, and two neighbours of the .lab overlap only where
    # the free decode's own segments do (its chunks' last frames close on their own offsets), never a token and anything else
    over = lambda segs: [(x, y) for x, y in zip(segs, segs[1:]) if x[1] > y[0] + 1e-9]      # noqa: E731
    print("overlapping neighbours of the .lab:", over(got), "of the free decode:", over(free))
    tokens = [s for s in plain if s[2] not in ("SP", "AP")]
    assert tokens[1][1] <= a + 1e-9 and b <= tokens[2][0] + 1e-9 and all(a <= s < e <= b for s, e, _ in held)
    assert all(x[0] <= x[1] for x in got) and [s[0] for s in got] == sorted(s[0] for s in got)
    assert all(x in held and y in held for x, y in over(got)) and len(over(got)) <= len(over(free))


def test_adjacent_fillers_are_collapsed_with_their_line(whisper, spy, capsys):  # noqa: F811
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    base = _transcript(90)
    one = _with_filler(base)
    three = base[:30] + [F, F, F] + base[45:]
    ref, ref_rows = _label(lab, path, one, filler_token=F)
    capsys.readouterr()
    got, rows = _label(lab, path, three, filler_token=F)
    out = capsys.readouterr().out
    assert got == ref and rows == ref_rows and "2 adjacent filler tokens collapsed" in out
    call = [c for c in spy if c["entry"] != "free"][-1]
    assert call["entry"] == "viterbi_align_filler" and sum(call["fillers"][0]) == 1 and len(call["fillers"][0]) == 77


def test_the_greedy_fallback_gets_the_transcript_without_its_fillers(whisper, spy, capsys):  # noqa: F811
    d, lab = whisper
    p = str(d / "wavs" / "plain.wav")
    base = _transcript(299)                               # 300 tokens in 4 s = 200 frames: no path, with or without a filler
    tr = base[:100] + [F] + base[100:]
    plain, _ = _label(lab, p, base)                       # (more tokens than frames: the greedy alignment already)
    capsys.readouterr()
    got, fillers = _label(lab, p, tr, filler_token=F)
    out = capsys.readouterr().out
    assert got == plain and fillers is None
    assert "viterbi alignment not possible (301 tokens for 200 frames); using the greedy alignment" in out
    call = [c for c in spy if c["entry"] != "free"][-1]
    assert call["entry"] == "viterbi_align_filler" and call["status"][0] == AL.STATUS_INFEASIBLE and (call["tok"] == -1).all()
