"""-m gpu: `postprocess.decode_duration_scores` end to end on the synthetic tiny Whisper checkpoint and the two files of
tests/test_gpu_decode_duration_e2e.py (a 7 s file and a 65 s file, 30 s windows): the score files of a duration-prior decode and the
unchanged .lab files; no call of the new entry without the key; the files' figures against decode.free_score over the float64
reference (tests/bio_duration_posterior_ref.py) run on the Labeler's own logits, by the rule of
tests/test_gpu_decode_duration_posterior.py; a run across the 30 s seam as one row; agreement with `bigram_scores` under a flat prior
at weight 0; the refusals through the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bio_duration_posterior_ref as DP
import bio_duration_ref as R
import test_gpu_decode_duration_e2e as E
import test_gpu_decode_duration_posterior as TP
from test_gpu_decode_duration_e2e import logits, setup  # noqa: F401  (the module's fixtures: the checkpoint, the files, their logits)
from wfl_asr_amd import _lib
from wfl_asr_amd import decode as DC
from wfl_asr_amd import infer as I
from wfl_asr_amd import options as OPT
from wfl_asr_amd import postprocess as pp

pytestmark = pytest.mark.gpu
LABELS, NAMES, LAM, ROOT = E.LABELS, E.NAMES, E.LAM, E.ROOT


def _tsv(path):
    lines = open(path, encoding="utf-8").read().split("\n")
    assert lines[-1] == "" and lines[0].startswith("# ")
    head = lines[0][2:].split("\t")
    return dict(kv.split("=") for kv in head[:4]), head[4], [ln.split("\t") for ln in lines[1:-1]]


class _Counted:
    """Counts the calls of one entry of the loaded library while it is in place."""

    def __init__(self, monkeypatch, name):
        lib = _lib.load()
        real = getattr(lib, name)
        self.n = 0

        def counted(*a):
            self.n += 1
            return real(*a)
        monkeypatch.setattr(lib, name, counted, raising=False)


def test_the_key_writes_the_score_files_and_changes_no_lab(setup, tmp_path, monkeypatch):
    d, lab = setup
    cfg, ckpt, prior = str(d / "config.yaml"), str(d / "best_model.pt"), str(d / "min3.json")
    kw = dict(decode="viterbi", switch_penalty=LAM, decode_duration_prior=prior)
    calls = _Counted(monkeypatch, "wfl_decode_duration_posterior")
    I.infer_folder(str(d / "wavs"), cfg, ckpt, str(tmp_path / "off"), **kw)
    assert calls.n == 0                                      # without the key the new entry is never called
    I.infer_folder(str(d / "wavs"), cfg, ckpt, str(tmp_path / "on"), decode_duration_scores=True, **kw)
    assert calls.n >= 1
    on, off = tmp_path / "on", tmp_path / "off"
    stems = [n[:-4] for n in NAMES]
    assert sorted(os.listdir(off)) == sorted(s + ".lab" for s in stems)
    assert sorted(os.listdir(on)) == sorted([s + ".lab" for s in stems] + [s + ".decode_scores.tsv" for s in stems] + ["decode_scores.tsv"])
    mins = {}
    for s in stems:
        assert open(on / f"{s}.lab", "rb").read() == open(off / f"{s}.lab", "rb").read()
        figures, counts, rows = _tsv(on / f"{s}.decode_scores.tsv")
        assert list(figures) == ["path_log_posterior", "mean_frame_logprob", "legal_log_mass_per_frame", "min_posterior"]
        assert len(rows) > 0 and counts.startswith(f"runs={len(rows)} ")
        for row in rows:
            got = [float(x) for x in row[3:]]
            assert len(row) == 6 and 0 <= got[1] <= 1 and got[2] <= got[0] + 1e-6 <= 1 + 2e-6
        mins[s + ".wav"] = float(figures["min_posterior"])
    review = open(on / "decode_scores.tsv").read().split("\n")
    assert review[0].startswith("# file\tmin_posterior") and review[-1] == "" and len(review) == 2 + len(NAMES)
    listed = [(r.split("\t")[0], float(r.split("\t")[1])) for r in review[1:-1]]
    assert listed == sorted(listed, key=lambda r: (r[1], r[0])) and dict(listed) == pytest.approx(mins)


def test_the_scores_are_free_score_over_the_float64_reference(setup, logits):  # noqa: F811
    """Per file: the Labeler's FreeScore against decode.free_score over the float64 forward-backward on the Labeler's own logits and the
    search's own path.  Per-frame posteriors may deviate by the rule of tests/test_gpu_decode_duration_posterior.py (4 x the float32
    restatement's deviation, plus half an fp32 ulp); a run's figures are a mean, a single value and a minimum of them, so the same
    allowance holds for each.  The 65 s file's run across a 30 s seam is one row."""
    d, lab = setup
    prior = str(d / "min3.json")
    table = DC.class_table(LABELS)
    paths = [str(d / "wavs" / n) for n in NAMES]
    kw = dict(decode="viterbi", switch_penalty=LAM, decode_duration_prior=prior)
    plain = lab.label_files(paths, **kw)
    segs, scores = lab.label_files(paths, decode_duration_scores=True, **kw)
    assert plain == segs and all(isinstance(sc, DC.FreeScore) for sc in scores)
    trans, dur, sym_dur = lab._decode_duration_prior(prior, 1.0, LAM, None, None)
    kind = lab._table.kind
    seam_runs = 0
    for n, sc in zip(NAMES, scores):
        z, cf, co, cc = logits[n]
        ids, score, st = DC.bio_viterbi_duration(torch.from_numpy(z).cuda(), [len(z)], table, trans, dur, sym_dur, 0.0)
        ids = ids.cpu().numpy()
        assert st.cpu().tolist() == [0]
        r64 = DP.forward_backward(z, table, trans.astype(np.float64), dur, sym_dur, None, ids)
        r32 = DP.forward_backward(z, table, trans.astype(np.float64), dur, sym_dur, None, ids, dtype=np.float32)
        yard = [float(np.abs(np.atleast_1d(a) - np.atleast_1d(b)).max()) for a, b in zip(r32, r64)]
        lse = float(R.prepass(z, 0.0)[0].sum())
        obj = R.objective(ids, z, table, trans, dur, sym_dur)
        fs = DC.free_score(obj - lse, r64[0], lse, r64[1], r64[2], ids, cf, co, cc, lab._table, pp.FRAME_DURATION)
        assert len(sc.runs) == len(fs.runs) > 0
        tol_post = float(TP._allowed(yard[1], np.array([1.0]))[0])
        tol_cls = float(TP._allowed(yard[2], np.array([1.0]))[0])
        dev = [0.0, 0.0, 0.0]
        for a, b in zip(sc.runs, fs.runs):
            assert (a.start_s, a.end_s, a.phoneme) == (b.start_s, b.end_s, b.phoneme)
            dev = [max(dev[0], abs(a.posterior - b.posterior)), max(dev[1], abs(a.start_posterior - b.start_posterior)),
                   max(dev[2], abs(a.min_frame_posterior - b.min_frame_posterior))]
        print(f"{n}: runs {len(fs.runs)}: posterior {dev[0]:.3e}, min_frame_posterior {dev[2]:.3e} (allowed {tol_post:.3e}; float32 "
              f"restatement {yard[1]:.3e}), start_posterior {dev[1]:.3e} (allowed {tol_cls:.3e}; restatement {yard[2]:.3e})")
        assert dev[0] <= tol_post and dev[2] <= tol_post and dev[1] <= tol_cls
        assert abs(sc.min_posterior - fs.min_posterior) <= tol_post
        # path_log_posterior = score + sum lse - logz: fp32 figures of these sizes; logz within its own allowance
        terms = (obj - lse, r64[0], lse)
        ulp = float(sum(np.spacing(np.float32(abs(x))) for x in terms))
        tol = 4 * ulp + float(TP._allowed(yard[0], np.array([r64[0]]))[0]) + 1e-3 * len(z)     # (1e-3 T: the search's own score bound)
        print(f"{n}: path_log_posterior {sc.path_log_posterior:.4f} (float64 {fs.path_log_posterior:.4f}), allowed {tol:.3e}")
        assert abs(sc.path_log_posterior - fs.path_log_posterior) <= tol
        # a run that crosses a seam is one row
        pos = 0
        for tc in cf[:-1]:
            pos += tc
            seam_runs += int(kind[ids[pos]] == 2)
        n_runs = int((kind[ids] == 1).sum())
        assert len(sc.runs) == n_runs                          # a seam that cut a run in two would add a row
    assert seam_runs >= 1, "no run crosses a 30 s seam (test setup)"


def test_a_flat_prior_at_weight_zero_scores_as_bigram_scores(setup, logits):  # noqa: F811
    """The flat prior at weight 0 and a bigram: the search is the bigram's (identical .lab files, tests/test_gpu_decode_duration_e2e.py)
    and so is the grammar the posteriors sum over; the two entries' figures agree within the summed allowances of the two kernel
    tests' rule, each from its own float32 restatement on the file's logits and the bigram search's path."""
    import bio_bigram_posterior_ref as BP
    from wfl_asr_amd import phonotactics as PH
    d, lab = setup
    table = DC.class_table(LABELS)
    paths = [str(d / "wavs" / n) for n in NAMES]
    flat, bg = str(d / "flat.json"), str(d / "phoneme_bigram.json")
    kw = dict(decode="viterbi", switch_penalty=LAM, phoneme_bigram=bg, bigram_weight=0.7)
    s1, big = lab.label_files(paths, bigram_scores=True, **kw)
    s2, dur = lab.label_files(paths, decode_duration_prior=flat, decode_duration_prior_weight=0.0, decode_duration_scores=True, **kw)
    assert s1 == s2
    W = PH.transition_table(PH.load(bg), table, LABELS, LAM, 0.7)
    zero = np.zeros((1, 2), np.float32)
    for n, a, b in zip(NAMES, big, dur):
        z = logits[n][0]
        ids = DC.bio_viterbi_bigram(torch.from_numpy(z).cuda(), [len(z)], table, W, 0.0)[0].cpu().numpy()
        r64 = BP.forward_backward(z, table, W.astype(np.float64), None, ids)
        y_big = [float(np.abs(np.atleast_1d(x) - np.atleast_1d(y)).max())
                 for x, y in zip(BP.forward_backward(z, table, W.astype(np.float64), None, ids, dtype=np.float32), r64)]
        y_dur = [float(np.abs(np.atleast_1d(x) - np.atleast_1d(y)).max())
                 for x, y in zip(DP.forward_backward(z, table, W.astype(np.float64), zero, np.full(len(table.pairs), -1), None, ids,
                                                     dtype=np.float32), r64)]
        one = np.array([1.0])
        tol_post = float((TP._allowed(y_big[1], one) + TP._allowed(y_dur[1], one))[0])
        tol_cls = float((TP._allowed(y_big[2], one) + TP._allowed(y_dur[2], one))[0])
        tol_logz = float((TP._allowed(y_big[0], np.array([r64[0]])) + TP._allowed(y_dur[0], np.array([r64[0]])))[0])
        print(f"{n}: allowed between the two: post {tol_post:.3e}, cls_post {tol_cls:.3e}, logz {tol_logz:.3e}")
        assert isinstance(a, DC.FreeScore) and isinstance(b, DC.FreeScore) and len(a.runs) == len(b.runs) > 0
        for x, y in zip(a.runs, b.runs):
            assert (x.start_s, x.end_s, x.phoneme) == (y.start_s, y.end_s, y.phoneme)
            assert abs(x.posterior - y.posterior) <= tol_post and abs(x.min_frame_posterior - y.min_frame_posterior) <= tol_post
            assert abs(x.start_posterior - y.start_posterior) <= tol_cls
        assert abs(a.min_posterior - b.min_posterior) <= tol_post
        assert abs(a.legal_log_mass_per_frame - b.legal_log_mass_per_frame) * len(z) <= tol_logz      # (logz - sum lse) / T: the same lse


def test_a_file_that_falls_back_to_argmax_gets_no_scores(setup, tmp_path, capsys):
    """A stub class table that uses one class twice makes wfl_decode_duration report status 4: no fault is provoked."""
    d, lab = setup
    capsys.readouterr()
    lab._decode_table = DC.ClassTable(LABELS.index("O"), np.array([(0, 1)] * 6, np.int32))
    try:
        out = lab.label_files([str(d / "wavs" / "a.wav")], decode="viterbi", decode_duration_prior=str(d / "flat.json"),
                              decode_duration_scores=True)
    finally:
        lab._decode_table = None
    text = capsys.readouterr().out
    assert text.count("viterbi decode not possible (wfl_decode_duration status 4); using the argmax decode") == 1
    assert isinstance(out, tuple) and out[1] == [None]


def test_the_refusals_through_the_cli(setup, tmp_path):
    d, lab = setup
    p = str(d / "wavs" / "a.wav")
    prior = str(d / "min3.json")
    base = [sys.executable, os.path.join(ROOT, "infer.py"), p, "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml")]
    for flags, message in ((["--decode", "viterbi", "--decode-duration-scores"], "decode_duration_scores needs a decode_duration_prior"),
                           (["--decode-duration-prior", prior, "--decode-duration-scores"], "need decode='viterbi'"),
                           (["--decode", "viterbi", "--decode-duration-prior", prior, "--decode-scores"],
                            OPT.DECODE_DURATION_PRIOR_ERROR[:60])):
        r = subprocess.run(base + ["-o", str(tmp_path / "b.lab")] + flags, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and message in r.stderr and not os.path.exists(tmp_path / "b.lab"), (flags, r.stderr)
    r = subprocess.run(base + ["-o", str(tmp_path / "a.lab"), "--decode", "viterbi", "--switch-penalty", str(LAM), "--decode-duration-prior",
                               prior, "--decode-duration-scores"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want = lab.label_files([p], decode="viterbi", switch_penalty=LAM, decode_duration_prior=prior)[0]
    assert open(tmp_path / "a.lab", "rb").read() == E._lab_bytes(want)
    figures, counts, rows = _tsv(tmp_path / "a.decode_scores.tsv")
    assert len(rows) > 0 and counts.startswith(f"runs={len(rows)} ")
