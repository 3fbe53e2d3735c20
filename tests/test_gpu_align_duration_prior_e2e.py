"""-m gpu: `postprocess.duration_prior` end to end on the synthetic tiny Whisper checkpoint of test_gpu_align_e2e.py (random weights,
rebuilt here): a 7 s file gives the segments of the float64 explicit-duration DP over the forward's own logits, a 65 s file carries a
run across the 30 s seam, a prior that forbids every path falls back with its message, a weight of 0 gives the plain alignment, the
CLI flags reach infer_folder, a prior that does not fit the model is refused by name, and without the key nothing changes and the new
entry is never called."""
import os
import shutil

import numpy as np
import pytest
import torch

import synthetic as synth
import viterbi_duration_prior_ref as DP
import viterbi_ref as V
from cases import tiny_whisper_config
from test_gpu_align_e2e import LABELS, _setup, _write_tr
from wfl_asr_amd import align as AL
from wfl_asr_amd import audio as A
from wfl_asr_amd import durations as DU
from wfl_asr_amd import infer as I
from wfl_asr_amd import native_post as npost
from wfl_asr_amd import postprocess as pp

pytestmark = pytest.mark.gpu
FD = pp.FRAME_DURATION
CT = 0.3
NEG = -np.inf
NAMES = ["p00", "p01", "p02", "p03"]


@pytest.fixture(scope="module")
def whisper(tmp_path_factory):
    d = tmp_path_factory.mktemp("vp")
    cfg = tiny_whisper_config(enable_bilstm=False)
    cfg["model"]["encoder_arch"]["max_positions"] = 1500
    lab = _setup(d, cfg, 41)
    A.write_wav(str(d / "wavs" / "a.wav"), synth.make_clip(800, 16000 * 7, seed=41) * 0.9, 16000)
    A.write_wav(str(d / "wavs" / "long.wav"), synth.make_clip(801, 16000 * 65, seed=41) * 0.8, 16000)
    A.write_wav(str(d / "wavs" / "plain.wav"), synth.make_clip(802, 16000 * 4, seed=41) * 0.7, 16000)
    return d, lab


def _prior(d, name, rows, tails, D, phonemes=NAMES, fd=FD):
    """A prior written by hand -> (its path, the DurationPrior)."""
    prior = DU.DurationPrior(fd, D, list(phonemes), [None if r is None else np.asarray(r, np.float64) for r in rows],
                             np.asarray(tails, np.float64))
    path = str(d / name)
    DU.save(prior, path)
    return path, DU.load(path)


@pytest.fixture
def spy(monkeypatch):
    """Every search call of the Labeler, in order: the entry, its table and rows, and its outputs on the host."""
    calls = []
    real_prior, real_plain = AL.viterbi_align_duration_prior, AL.viterbi_align

    def with_prior(*a, **kw):
        out = real_prior(*a, **kw)
        calls.append(dict(entry="prior", rows=a[5], table=np.array(a[6]), n_frames=list(a[1]), tok=out[1].cpu().numpy(),
                          status=out[3].cpu().numpy()))
        return out

    def plain(*a, **kw):
        out = real_plain(*a, **kw)
        calls.append(dict(entry="plain", n_frames=list(a[1]), tok=out[1].cpu().numpy(), status=out[3].cpu().numpy()))
        return out
    monkeypatch.setattr(AL, "viterbi_align_duration_prior", with_prior)
    monkeypatch.setattr(AL, "viterbi_align", plain)
    return calls


def _bytes(segs):
    return npost.format_lab_tuples(segs)


def _transcript(n, seed=7):
    """A transcript of its own (the weights are random), SP spelled as a token, so no pause of the free decode joins the result: the
    .lab is the path's segments, one per token."""
    names = [str(x) for x in np.random.default_rng(seed).choice(NAMES, size=n)]
    return names[:n // 2] + ["SP"] + names[n // 2:]


def _label(lab, path, tr, **kw):
    _write_tr(path, tr)
    try:
        return lab.label_files([path], confidence_threshold=CT, align="viterbi", **kw)[0]
    finally:
        os.remove(path.replace(".wav", ".txt"))


def _host_reference(lab, path, tr, prior, weight=1.0):
    """The clip through model.label(want_logits=True) and the float64 DP with the prior (None: the plain DP), assembled by the host
    helpers (as test_gpu_align_e2e._host_reference is built) -> (segments, the path's run lengths)."""
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
    if prior is None:
        states, _ = V.viterbi(z, alts, gaps)
    else:
        states, _, _ = DP.viterbi(z, alts, gaps, AL.duration_rows(tr, prior), DU.table(prior, weight))
    ids, tok = V.outputs(states, z, alts, LABELS.index("O"))
    return AL.path_segments(ids, tok, [tv], [offs], [0.0], lab._table, alts, tr, FD), DP.run_lengths(states, len(tr))


def _rows_per_token(tok, n):
    return np.bincount(tok[tok >= 0], minlength=n)


def test_a_prior_gives_the_host_explicit_duration_dp(whisper, spy):
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    tr = _transcript(90)                                  # 91 tokens in 350 frames: the plain optimum has short runs
    # p00: a soft histogram that likes 3 frames; p01: at least 3 frames and a tail; p02: one or two frames, never more; p03: none
    pr_path, prior = _prior(d, "durations.json", [[-3.0, -1.5, -0.2, -2.0], [NEG, NEG, -0.5, -1.0], [-0.7, -0.7, NEG, NEG], None],
                            [-0.5, -0.3, NEG, NEG], 4)
    assert AL.duration_rows(["p00", "SP", "p03", "p01"], prior) == [0, -1, -1, 1]
    free_ref, free_runs = _host_reference(lab, path, tr, None)
    ref, runs = _host_reference(lab, path, tr, prior)
    p01, p02 = np.array([t == "p01" for t in tr]), np.array([t == "p02" for t in tr])
    assert (free_runs[p01] < 3).any() and (runs[p01] >= 3).all() and (runs[p02] <= 2).all() and ref != free_ref, "test setup"
    got = _label(lab, path, tr, duration_prior=pr_path)
    assert got == ref
    assert len(spy) == 1 and spy[0]["entry"] == "prior" and spy[0]["status"][0] == 0
    assert spy[0]["rows"] == [AL.duration_rows(tr, prior)] and np.array_equal(spy[0]["table"], DU.table(prior, 1.0))
    rows = _rows_per_token(spy[0]["tok"], len(tr))
    assert (rows == runs).all()
    # the config keys give the same; another weight gives that weight's optimum
    lab.config["postprocess"]["duration_prior"] = pr_path
    try:
        assert _label(lab, path, tr) == ref
        lab.config["postprocess"]["duration_prior_weight"] = 0.25
        assert _label(lab, path, tr) == _host_reference(lab, path, tr, prior, 0.25)[0]
        assert np.array_equal(spy[-1]["table"], DU.table(prior, 0.25))
    finally:
        lab.config["postprocess"].pop("duration_prior", None)
        lab.config["postprocess"].pop("duration_prior_weight", None)


def test_weight_zero_without_forbidden_durations_is_the_plain_alignment(whisper, spy):
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    tr = _transcript(90)
    pr_path, _ = _prior(d, "soft.json", [[-3.0, -1.5, -0.2], [-0.1, -2.0, -4.0], [-1.0, -1.0, -1.0], [-0.3, -0.3, -5.0]], [-0.5] * 4, 3)
    plain = _label(lab, path, tr)
    assert spy[-1]["entry"] == "plain"
    got = _label(lab, path, tr, duration_prior=pr_path, duration_prior_weight=0)
    assert spy[-1]["entry"] == "prior" and (spy[-1]["table"] == 0).all()
    assert _bytes(got) == _bytes(plain)
    assert _bytes(_label(lab, path, tr, duration_prior=pr_path)) != _bytes(plain)      # (at weight 1 the prior does move boundaries)


def test_a_long_file_carries_a_run_across_the_seam(whisper, spy, capsys):
    d, lab = whisper
    long_p = str(d / "wavs" / "long.wav")
    # 65 s = 3250 rows in chunks of 1500, 1500 and 250; 100 tokens of at least 32 frames leave at most 50 gap frames
    hard = [NEG] * 31 + [0.0]
    pr_path, prior = _prior(d, "hard.json", [hard] * 4, [0.0] * 4, 32)
    tr = [NAMES[k % 4] for k in range(100)]
    capsys.readouterr()
    got = _label(lab, long_p, tr, duration_prior=pr_path)
    assert I.DURATION_PRIOR_INFEASIBLE not in capsys.readouterr().out
    assert [s[2] for s in got if s[2] in NAMES] == tr
    call = spy[-1]
    assert call["entry"] == "prior" and call["n_frames"] == [3250] and call["status"][0] == 0
    tok = call["tok"]
    assert (_rows_per_token(tok, 100) >= 32).all()
    k = int(tok[1499])
    assert k >= 0 and tok[1500] == k                       # one run either side of the seam between the chunks
    seg = [s for s in got if s[2] in NAMES][k]
    assert seg[0] < 30.0 < seg[1]


def test_a_prior_that_forbids_every_path_falls_back_with_its_message(whisper, spy, capsys):
    d, lab = whisper
    p = str(d / "wavs" / "plain.wav")
    tr = _transcript(40)
    pr_path, _ = _prior(d, "shut.json", [[NEG, NEG], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]], [NEG, 0.0, 0.0, 0.0], 2)
    assert "p00" in tr
    plain = _label(lab, p, tr)
    capsys.readouterr()
    n = len(spy)
    got = _label(lab, p, tr, duration_prior=pr_path)
    assert capsys.readouterr().out.count(I.DURATION_PRIOR_INFEASIBLE) == 1
    assert got == plain
    assert [c["entry"] for c in spy[n:]] == ["prior", "plain"] and spy[n]["status"][0] == AL.STATUS_INFEASIBLE
    assert (spy[n]["tok"] == -1).all() and spy[n + 1]["status"][0] == 0


def test_a_prior_that_does_not_fit_the_model_is_refused_by_name(whisper):
    d, lab = whisper
    path = str(d / "wavs" / "plain.wav")
    tr = _transcript(10)
    alien, _ = _prior(d, "alien.json", [[0.0], [0.0]], [0.0, 0.0], 1, phonemes=["p00", "zz9"])
    with pytest.raises(ValueError, match="no output name of the label set: zz9"):
        _label(lab, path, tr, duration_prior=alien)
    clock, _ = _prior(d, "clock.json", [[0.0]], [0.0], 1, phonemes=["p00"], fd=0.01)
    with pytest.raises(ValueError, match="counted on frames of 0.01 s"):
        _label(lab, path, tr, duration_prior=clock)
    with pytest.raises(ValueError, match="duration_prior cannot be combined"):
        _label(lab, path, tr, duration_prior=alien, min_duration=0.06)


def test_the_cli_flags_reach_infer_folder_and_without_the_key_nothing_changes(whisper, tmp_path, monkeypatch):
    d, lab = whisper
    folder = tmp_path / "in"
    os.makedirs(folder)
    shutil.copyfile(str(d / "wavs" / "a.wav"), str(folder / "a.wav"))
    shutil.copyfile(str(d / "wavs" / "plain.wav"), str(folder / "b.wav"))       # a file without a transcript
    path = str(folder / "a.wav")
    tr = _transcript(90)
    pr_path, prior = _prior(d, "cli.json", [[-3.0, -1.5, -0.2, -2.0], [NEG, NEG, -0.5, -1.0], [-0.7, -0.7, NEG, NEG], None],
                            [-0.5, -0.3, NEG, NEG], 4)
    ref = _label(lab, path, tr, duration_prior=pr_path, duration_prior_weight=0.5)
    assert ref == _host_reference(lab, path, tr, prior, 0.5)[0]
    plain = _label(lab, path, tr)
    assert plain == _host_reference(lab, path, tr, None)[0]
    untranscribed = lab.label_files([str(folder / "b.wav")], confidence_threshold=CT)[0]
    seen = {}
    real = I.infer_folder

    def infer_folder(**kw):
        seen.update(kw)
        return real(**kw)
    monkeypatch.setattr(I, "infer_folder", infer_folder)
    _write_tr(path, tr)
    args = [str(folder), "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml"), "--align", "viterbi"]
    with pytest.raises(SystemExit) as e:
        I.main(args + ["-o", str(tmp_path / "out"), "--duration-prior", pr_path, "--duration-prior-weight", "0.5"])
    assert e.value.code == 0
    assert seen["duration_prior"] == pr_path and seen["duration_prior_weight"] == 0.5
    assert open(tmp_path / "out" / "a.lab", "rb").read() == _bytes(ref)
    assert open(tmp_path / "out" / "b.lab", "rb").read() == _bytes(untranscribed)       # labelled exactly as in greedy mode
    # without the flag (and the key): the .lab it gets without the option, and the new entry is never called
    monkeypatch.setattr(AL, "viterbi_align_duration_prior", lambda *a, **kw: pytest.fail("the duration-prior entry was called"))
    monkeypatch.setattr(I.Labeler, "_duration_prior", lambda *a, **kw: pytest.fail("a duration prior was loaded"))
    with pytest.raises(SystemExit) as e:
        I.main(args + ["-o", str(tmp_path / "out2")])
    assert e.value.code == 0 and seen["duration_prior"] == "" and seen["duration_prior_weight"] is None
    assert open(tmp_path / "out2" / "a.lab", "rb").read() == _bytes(plain) != _bytes(ref)
    assert open(tmp_path / "out2" / "b.lab", "rb").read() == _bytes(untranscribed)
    assert sorted(os.listdir(tmp_path / "out2")) == ["a.lab", "b.lab"]
    # refused before a model is loaded: no --align viterbi, a bad weight, a weight alone, a lattice without a duration term beside it
    monkeypatch.setattr(I, "_labeler", lambda *a, **kw: pytest.fail("a model was loaded"))
    for extra in (["--align", "greedy", "--duration-prior", pr_path], ["--duration-prior", pr_path, "--duration-prior-weight", "-1"],
                  ["--duration-prior-weight", "1"], ["--duration-prior", pr_path, "--min-duration", "0.06"],
                  ["--duration-prior", pr_path, "--align-scores"]):
        with pytest.raises(SystemExit) as e:
            I.main(args + extra)
        assert e.value.code == 2
