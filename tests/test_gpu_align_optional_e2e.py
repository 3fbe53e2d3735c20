"""-m gpu: `postprocess.optional_tokens` end to end on the synthetic tiny Whisper checkpoint of test_gpu_align_min_duration_e2e.py
(random weights, rebuilt here): a 7 s file gives the segments of the float64 DP with skip arcs over the forward's own logits and its
.skipped.tsv lists the tokens that DP leaves out, a large penalty gives the plain Viterbi .lab, without the keys nothing changes, the
config key and the CLI flags reach infer_folder, a 65 s file with a draft keeps its kept tokens inside their windows, the safety net
keeps the flags when it drops a draft's windows, and a request with more mandatory tokens than frames falls back to the greedy
alignment with its message."""
import os
import shutil

import numpy as np
import pytest
import torch

import viterbi_optional_ref as R
from test_gpu_align_e2e import LABELS, _write_tr
from test_gpu_align_min_duration_e2e import CT, FD, _bytes, _transcript, whisper  # noqa: F401  (the module's fixture, built once here)
from wfl_asr_amd import align as AL
from wfl_asr_amd import infer as I
from wfl_asr_amd import reports as RP

pytestmark = pytest.mark.gpu


@pytest.fixture
def spy(monkeypatch):
    """Every search call of the Labeler, by entry: its keyword arguments and its outputs on the host."""
    calls = []

    def wrap(name):
        real = getattr(AL, name)

        def f(*a, **kw):
            out = real(*a, **kw)
            rec = dict(kw, entry=name, n_frames=list(a[1]), tok=out[1].cpu().numpy(), status=out[3].cpu().numpy())
            if name == "viterbi_align_optional":
                rec.update(optional=a[5], skip_penalty=a[6], skipped=out[4].cpu().numpy())
            calls.append(rec)
            return out
        monkeypatch.setattr(AL, name, f)
    wrap("viterbi_align")
    wrap("viterbi_align_optional")
    return calls


def _label(lab, path, tr, **kw):
    _write_tr(path, tr)
    try:
        out = lab.label_files([path], confidence_threshold=CT, align="viterbi", **kw)
    finally:
        os.remove(path.replace(".wav", ".txt"))
    return (out[0][0], out[1][0]) if isinstance(out, tuple) else (out[0], None)


def _host_reference(lab, path, tr, flags, lam):
    """The clip through model.label(want_logits=True) and the float64 DP with skip arcs, assembled by the host helpers -> (segments,
    the DP's skipped flags)."""
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
    states, _ = R.viterbi(z, alts, gaps, flags, lam)
    assert states is not None
    ids, tok, sk = R.outputs(states, z, alts, LABELS.index("O"))
    return AL.path_segments(ids, tok, [tv], [offs], [0.0], lab._table, alts, tr, FD, skipped=sk), sk


def test_optional_tokens_give_the_host_dp_with_skip_arcs(whisper, spy, capsys):  # noqa: F811
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    tr = _transcript(90)                                  # 91 tokens in 350 frames
    flags = AL.optional_flags(tr, ["p01"])
    assert any(flags) and not all(flags)
    ref, sk = _host_reference(lab, path, tr, flags, 0.0)
    plain_ref, none = _host_reference(lab, path, tr, None, 0.0)
    assert sk.sum() >= 1 and not none.any(), "the reference skips no token (test setup)"
    assert all(flags[k] for k in np.nonzero(sk)[0]) and len(ref) == len(tr) - sk.sum()
    capsys.readouterr()
    got, skipped = _label(lab, path, tr, optional_tokens=["p01"])
    out = capsys.readouterr().out
    assert got == ref and [s[2] for s in got] == [t for t, f in zip(tr, sk) if not f]
    assert [r.index for r in skipped] == np.nonzero(sk)[0].tolist() and all(r.token == "p01" for r in skipped)
    assert f"{int(sk.sum())} of {sum(flags)} optional tokens skipped" in out
    call = spy[-1]
    assert call["entry"] == "viterbi_align_optional" and call["optional"] == [flags] and call["skip_penalty"] == 0.0
    assert (call["skipped"] == sk).all() and call["status"][0] == 0
    assert not set(np.nonzero(sk)[0].tolist()) & set(call["tok"].tolist())       # a skipped token never appears in tok
    # a penalty larger than any path difference: the plain Viterbi .lab, byte for byte; and a moderate one is the reference's again
    n = len(spy)
    big, big_skipped = _label(lab, path, tr, optional_tokens=["p01"], skip_penalty=1.0e4)
    assert _bytes(big) == _bytes(plain_ref) != _bytes(ref) and big_skipped == [] and spy[n]["entry"] == "viterbi_align_optional"
    ref2, sk2 = _host_reference(lab, path, tr, flags, 1.5)
    got2, skipped2 = _label(lab, path, tr, optional_tokens=["p01"], skip_penalty=1.5)
    assert got2 == ref2 and [r.index for r in skipped2] == np.nonzero(sk2)[0].tolist() and sk2.sum() <= sk.sum()
    # without the keys: the search and the .lab are as they were
    n = len(spy)
    plain, nothing = _label(lab, path, tr)
    assert plain == plain_ref and nothing is None and [c["entry"] for c in spy[n:]] == ["viterbi_align"]
    # a name the label set does not have is refused by name
    with pytest.raises(ValueError, match="'zz' is no output name"):
        _label(lab, path, tr, optional_tokens=["p01", "zz"])


def test_the_config_key_and_the_cli_flags_reach_infer_folder(whisper, tmp_path, monkeypatch):  # noqa: F811
    d, lab = whisper
    folder = tmp_path / "in"
    os.makedirs(folder)
    shutil.copyfile(str(d / "wavs" / "a.wav"), str(folder / "a.wav"))
    path = str(folder / "a.wav")
    tr = _transcript(90)
    ref, skipped = _label(lab, path, tr, optional_tokens=["p01", "p03"], skip_penalty=0.5)
    plain, _ = _label(lab, path, tr)
    assert skipped and _bytes(ref) != _bytes(plain)
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
        I.main(args + ["-o", str(tmp_path / "out"), "--optional", "p03", "--optional", "p01", "--skip-penalty", "0.5"])
    assert e.value.code == 0 and seen["optional_tokens"] == ("p01", "p03") and seen["skip_penalty"] == 0.5
    assert open(tmp_path / "out" / "a.lab", "rb").read() == _bytes(ref)
    want = RP.file_text("skipped", skipped)
    assert open(tmp_path / "out" / "a.skipped.tsv", encoding="utf-8").read() == want and want.count("\n") == len(skipped) + 1
    assert open(tmp_path / "out" / "skipped_tokens.tsv", encoding="utf-8").read() == RP.folder_text("skipped", [("a.wav", skipped)])
    # '*' from the command line; the key from the config file
    with pytest.raises(SystemExit) as e:
        I.main(args + ["-o", str(tmp_path / "out_all"), "--optional", "*"])
    assert e.value.code == 0 and seen["optional_tokens"] == "*" and seen["skip_penalty"] == 0.0
    assert os.path.isfile(tmp_path / "out_all" / "skipped_tokens.tsv")
    with pytest.raises(SystemExit) as e:                  # without the flags (and the keys): the .lab it gets without the option
        I.main(args + ["-o", str(tmp_path / "out2")])
    assert e.value.code == 0 and seen["optional_tokens"] is None and seen["skip_penalty"] is None
    assert open(tmp_path / "out2" / "a.lab", "rb").read() == _bytes(plain)
    assert sorted(os.listdir(tmp_path / "out2")) == ["a.lab"]
    lab.config["postprocess"].update(optional_tokens=["p01", "p03"], skip_penalty=0.5)
    try:
        os.remove(path.replace(".wav", ".txt"))
        assert _label(lab, path, tr)[0] == ref
    finally:
        del lab.config["postprocess"]["optional_tokens"], lab.config["postprocess"]["skip_penalty"]
    # refused before a model is loaded
    monkeypatch.setattr(I, "_labeler", lambda *a, **kw: pytest.fail("a model was loaded"))
    for extra in (["--align", "greedy", "--optional", "p01"], ["--skip-penalty", "1"], ["--optional", "p01", "--align-scores"],
                  ["--optional", "p01", "--min-duration", "0.06"], ["--optional", "p01", "--skip-penalty", "-1"]):
        with pytest.raises(SystemExit) as e:
            I.main(args + extra)
        assert e.value.code == 2


def test_with_a_draft_kept_tokens_hold_their_windows(whisper, spy, capsys):  # noqa: F811
    d, lab = whisper
    long_p = str(d / "wavs" / "long.wav")
    names = ["p00", "p01", "p02", "p03"]
    base = [(0.5 + k, 0.9 + k, names[k % 4] if k != 40 else "SP") for k in range(64)]     # a token every second from 0.5 s
    tr = [s[2] for s in base]
    with open(str(d / "drafts" / "long.lab"), "wb") as f:
        f.write(_bytes(base))
    try:
        capsys.readouterr()
        opts = lab.options(align="viterbi", align_draft=str(d / "drafts"), draft_tolerance=0.1, optional_tokens="*", skip_penalty=0.0)
        reports = RP.Reports.for_options(opts)
        got, _ = lab._label_scored([long_p], opts, None, CT, False, reports)
        moves, skipped = reports.moves, reports.rows["skipped"]
        out = capsys.readouterr().out
    finally:
        os.remove(str(d / "drafts" / "long.lab"))
    assert I.DRAFT_INFEASIBLE not in out
    call = spy[-1]
    assert call["entry"] == "viterbi_align_optional" and call["windows"] is not None and call["status"][0] == 0
    sk, tok = call["skipped"], call["tok"]
    kept = [k for k in range(64) if not sk[k]]
    assert sk.any(), "the path skips no token (test setup)"
    assert [r.index for r in skipped[0]] == [k for k in range(64) if sk[k]] and len(kept) >= 32        # never two skips in a row
    assert [s[2] for s in got[0]] == [tr[k] for k in kept]
    lo, hi = np.array(call["windows"][0]).T
    first = {k: int(np.nonzero(tok == k)[0][0]) for k in kept}
    assert all(lo[k] <= first[k] <= hi[k] for k in kept) and not set(np.nonzero(sk)[0].tolist()) & set(tok.tolist())
    assert [m.index for m in moves[0]] == kept and [m.token for m in moves[0]] == [tr[k] for k in kept]
    assert max(abs(m.move_s) for m in moves[0]) <= 0.1 + 2 * FD + 1e-6
    text = I.format_draft_moves_tsv([("long.wav", moves[0])])
    assert text.count("\n") == len(kept) + 1


def test_the_safety_net_keeps_the_flags_when_it_drops_the_windows(whisper, spy, capsys):  # noqa: F811
    d, lab = whisper
    p = str(d / "wavs" / "a.wav")
    names = ["p00", "p01", "p02", "p03"]
    # two mandatory neighbours pinned onto one frame: no path inside the windows, with or without skips
    base = [(0.2 + 0.3 * (6 if k == 7 else k), 0.4 + 0.3 * k, names[k % 4] if k != 12 else "SP") for k in range(20)]
    tr = [s[2] for s in base]                             # (SP spelled: no pause of the free decode joins the result)
    flags = AL.optional_flags(tr, ["p01"])
    assert not flags[6] and not flags[7]
    with open(str(d / "drafts" / "a.lab"), "wb") as f:
        f.write(_bytes(base))
    try:
        capsys.readouterr()
        opts = lab.options(align="viterbi", align_draft=str(d / "drafts"), draft_tolerance=0.0, optional_tokens=["p01"])
        reports = RP.Reports.for_options(opts)
        got, _ = lab._label_scored([p], opts, None, CT, False, reports)
        moves, skipped = reports.moves, reports.rows["skipped"]
        out = capsys.readouterr().out
    finally:
        os.remove(str(d / "drafts" / "a.lab"))
    assert out.count(I.DRAFT_INFEASIBLE) == 1
    first, second = spy[-2], spy[-1]
    assert first["entry"] == second["entry"] == "viterbi_align_optional"
    assert first["windows"] is not None and first["status"][0] == AL.STATUS_INFEASIBLE and not first["skipped"].any()
    assert second["windows"] is None and second["optional"] == [flags] and second["status"][0] == AL.STATUS_OK
    sk = second["skipped"]
    assert [r.index for r in skipped[0]] == np.nonzero(sk)[0].tolist() and all(flags[k] for k in np.nonzero(sk)[0])
    assert [s[2] for s in got[0]] == [t for t, f in zip(tr, sk) if not f] and 0 not in moves      # (no windows held: no moves)


def test_more_mandatory_tokens_than_frames_fall_back_to_greedy(whisper, spy, capsys):  # noqa: F811
    d, lab = whisper
    p = str(d / "wavs" / "plain.wav")
    tr = _transcript(299)                                 # 300 tokens, a quarter of them optional, in 4 s = 200 frames: no path
    flags = AL.optional_flags(tr, ["p01"])
    need = AL.min_frames_needed(flags)
    assert 200 < need < 300 and any(flags)
    plain, _ = _label(lab, p, tr)                         # (more tokens than frames: the greedy alignment already)
    capsys.readouterr()
    got, skipped = _label(lab, p, tr, optional_tokens=["p01"])
    out = capsys.readouterr().out
    assert got == plain and skipped is None
    assert f"viterbi alignment not possible (300 tokens need {need} frames" in out and "using the greedy alignment" in out
    assert spy[-1]["entry"] == "viterbi_align_optional" and spy[-1]["status"][0] == AL.STATUS_INFEASIBLE
    assert not spy[-1]["skipped"].any()
    # with every token optional the same file has a path: 150 frames are enough
    assert AL.min_frames_needed([True] * 300) == 150
    got, skipped = _label(lab, p, tr, optional_tokens="*")
    assert spy[-1]["status"][0] == AL.STATUS_OK and len(got) + len(skipped) >= 300 and len(skipped) >= 100
