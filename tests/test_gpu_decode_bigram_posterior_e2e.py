"""-m gpu: `bigram_scores` end to end on the synthetic tiny Whisper checkpoint and clips of tests/test_gpu_decode_bigram_e2e.py (30 s
windows): the score files of a bigram decode, their agreement with bio_viterbi_bigram + decode_posteriors_bigram called directly on
the files' logits, one clip per long file, no trace of the feature with the key absent, the config key, the argmax fallback, and the
refusal of decode_scores beside a bigram, which stays."""
import glob
import os

import numpy as np
import pytest
import torch
import yaml

import bio_bigram_ref as R
import synthetic as synth
import test_gpu_decode_bigram_e2e as E
from cases import tiny_whisper_config
from wfl_asr_amd import audio as A
from wfl_asr_amd import decode as DC
from wfl_asr_amd import infer as I
from wfl_asr_amd import phonotactics as PH
from wfl_asr_amd import postprocess as pp

pytestmark = pytest.mark.gpu
LABELS, LAM, WEIGHT = E.LABELS, E.LAM, E.WEIGHT
NAMES = ("a.wav", "long.wav", "t.wav")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgs")
    cfg = tiny_whisper_config(enable_bilstm=False)
    cfg["model"]["encoder_arch"]["max_positions"] = 1500
    cfg["output"]["save_dir"] = str(d / "save")
    cfg["postprocess"] = {"median_filter": 1, "merge_segments": "none", "confidence_threshold": 0.0}
    os.makedirs(d / "save")
    with open(d / "save" / "phonemes.txt", "w") as f:
        f.write("\n".join(LABELS) + "\n")
    with open(d / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, len(LABELS), seed=41).items()}
    torch.save(sd, d / "best_model.pt")
    os.makedirs(d / "wavs")
    A.write_wav(str(d / "wavs" / "a.wav"), synth.make_clip(800, 16000 * 7, seed=41) * 0.9, 16000)
    A.write_wav(str(d / "wavs" / "long.wav"), synth.make_clip(801, 16000 * 65, seed=41) * 0.8, 16000)
    A.write_wav(str(d / "wavs" / "t.wav"), synth.make_clip(802, 16000 * 12, seed=41) * 0.7, 16000)
    rng = np.random.default_rng(5)
    syms = ["O"] + list(E.PHONES[::-1])
    lp = -6.0 * rng.random((7, 7))
    mask = rng.random((7, 7)) < 0.2
    mask[:, 0] = False
    lp[mask] = -np.inf
    bg = str(d / "phoneme_bigram.json")
    PH.save(PH.Bigram(syms, lp), bg)
    cfg_path, ckpt = str(d / "config.yaml"), str(d / "best_model.pt")
    lab = I._labeler(cfg_path, ckpt, "cuda")               # the instance infer_audio / infer_folder use
    # t.wav gets a transcript, matched under align: greedy onto the searched segments
    free = lab.label_files([str(d / "wavs" / "t.wav")], decode="viterbi", switch_penalty=LAM, phoneme_bigram=bg, bigram_weight=WEIGHT)[0]
    names = [s[2] for s in free if s[2] not in ("SP", "AP")] or [s[2] for s in free]
    assert len(names) >= 1, "the decode has no segment to write a transcript from (test setup)"
    with open(d / "wavs" / "t.txt", "w") as f:
        f.write(" ".join(names[1:-1:2] or names[:1]))
    kw = dict(decode="viterbi", switch_penalty=LAM, phoneme_bigram=bg, bigram_weight=WEIGHT)
    I.infer_folder(str(d / "wavs"), cfg_path, ckpt, str(d / "out_on"), bigram_scores=True, **kw)
    I.infer_folder(str(d / "wavs"), cfg_path, ckpt, str(d / "out_off"), **kw)
    return d, lab, cfg_path, ckpt, bg, kw


def _tsv(path):
    lines = open(path, encoding="utf-8").read().split("\n")
    assert lines[-1] == "" and lines[0].startswith("# ")
    head = lines[0][2:].split("\t")
    return dict(kv.split("=") for kv in head[:4]), head[4], [ln.split("\t") for ln in lines[1:-1]]


def _direct(lab, path, W):
    """The file's FreeScore from bio_viterbi_bigram + decode_posteriors_bigram called directly on the file's concatenated logits, the
    three terms of its path_log_posterior and the path."""
    table = DC.class_table(LABELS)
    z, cf, co, cc = E._file_logits(lab, path)
    lg = torch.from_numpy(z).cuda()
    ids, score, st = DC.bio_viterbi_bigram(lg, [len(z)], table, W, 0.0)
    logz, post, cls, pst = DC.decode_posteriors_bigram(lg, [len(z)], table, W, 0.0, ids)
    assert st.cpu().tolist() == [0] and pst.cpu().tolist() == [0]
    ids = ids.cpu().numpy()
    lse = float(R.prepass(z, 0.0)[0].sum())
    fs = DC.free_score(float(score[0]), float(logz[0]), lse, post.cpu().numpy(), cls.cpu().numpy(), ids, cf, co, cc, lab._table,
                       pp.FRAME_DURATION)
    return fs, (float(score[0]), float(logz[0]), lse), ids, (z, cf, co, cc)


def test_key_on_writes_the_score_files_and_changes_no_lab(world):
    d, lab, cfg_path, ckpt, bg, kw = world
    on, off = d / "out_on", d / "out_off"
    mins = {}
    for name in NAMES:
        stem = name[:-4]
        assert open(on / f"{stem}.lab", "rb").read() == open(off / f"{stem}.lab", "rb").read()
        figures, counts, rows = _tsv(on / f"{stem}.decode_scores.tsv")
        assert list(figures) == ["path_log_posterior", "mean_frame_logprob", "legal_log_mass_per_frame", "min_posterior"]
        assert len(rows) > 0 and counts.startswith(f"runs={len(rows)} ")
        for row in rows:
            got = [float(x) for x in row[3:]]
            assert len(row) == 6 and 0 <= got[1] <= got[0] + 1e-6 and got[2] <= got[0] + 1e-6 <= 1 + 2e-6
        mins[name] = float(figures["min_posterior"])
    review = open(on / "decode_scores.tsv").read().split("\n")
    assert review[0].startswith("# file\tmin_posterior") and review[-1] == "" and len(review) == 2 + len(NAMES)
    listed = [(r.split("\t")[0], float(r.split("\t")[1])) for r in review[1:-1]]
    assert listed == sorted(listed, key=lambda r: (r[1], r[0])) and dict(listed) == pytest.approx(mins)      # the weakest first
    # without the key: the .lab files alone
    assert sorted(os.listdir(off)) == sorted(n[:-4] + ".lab" for n in NAMES)
    assert sorted(os.listdir(on)) == sorted([n[:-4] + ".lab" for n in NAMES] + [n[:-4] + ".decode_scores.tsv" for n in NAMES]
                                            + ["decode_scores.tsv"])


def test_the_scores_are_those_of_direct_calls(world):
    d, lab, cfg_path, ckpt, bg, kw = world
    table = DC.class_table(LABELS)
    W = PH.transition_table(PH.load(bg), table, LABELS, LAM, WEIGHT)
    assert np.isneginf(W).any()
    paths = [str(d / "wavs" / n) for n in NAMES]
    plain = lab.label_files(paths, **kw)
    segs, scores = lab.label_files(paths, bigram_scores=True, **kw)
    assert plain == segs and all(isinstance(sc, DC.FreeScore) for sc in scores)      # the return shape follows the decode_scores rule
    for p, sc in zip(paths, scores):
        fs, terms, ids, _ = _direct(lab, p, W)
        assert len(sc.runs) == len(fs.runs) > 0
        for a, b in zip(sc.runs, fs.runs):
            assert (a.start_s, a.end_s, a.phoneme) == (b.start_s, b.end_s, b.phoneme)
            assert [a.posterior, a.start_posterior, a.min_frame_posterior] == pytest.approx([b.posterior, b.start_posterior,
                                                                                             b.min_frame_posterior], abs=2e-6)
        # path_log_posterior = score + sum lse - logz: three fp32 figures of these sizes, each good to a few units in its last place
        ulp = float(sum(np.spacing(np.float32(abs(x))) for x in terms))
        print(f"{os.path.basename(p)}: path_log_posterior {sc.path_log_posterior:.4f} (direct {fs.path_log_posterior:.4f}), terms {terms}, "
              f"their fp32 spacings together {ulp:.3e}")
        assert sc.path_log_posterior == pytest.approx(fs.path_log_posterior, abs=4 * ulp)
        assert sc.path_log_posterior <= 4 * ulp and fs.path_log_posterior <= 4 * ulp
        assert sc.min_posterior == pytest.approx(fs.min_posterior, abs=2e-6)
        assert sc.mean_frame_logprob == pytest.approx(fs.mean_frame_logprob, abs=1e-4)
        assert sc.legal_log_mass_per_frame == pytest.approx(fs.legal_log_mass_per_frame, abs=1e-4) and sc.legal_log_mass_per_frame <= 1e-4


def test_a_run_crossing_a_seam_is_one_line(world, tmp_path):
    d, lab, cfg_path, ckpt, bg, kw = world
    table = DC.class_table(LABELS)
    p = str(d / "wavs" / "long.wav")
    z, cf, co, cc = E._file_logits(lab, p)
    assert cf[:2] == [1500, 1500] and len(cf) == 3
    kind = lab._table.kind
    found = None
    for lam, wt in ((1.0, 0.7), (2.0, 0.7), (4.0, 0.3), (0.5, 1.0), (8.0, 0.1), (0.0, 1.0), (2.0, 0.0), (1.0, 0.0), (4.0, 0.0), (0.5, 0.0),
                    (8.0, 0.0), (0.0, 0.0)):
        W = PH.transition_table(PH.load(bg), table, LABELS, lam, wt)
        ref, _ = R.viterbi(z, table, W.astype(np.float64))
        if any(kind[ref[s]] == 2 for s in (1500, 3000)):      # I-p opens a chunk: the continuation of the run before
            found = (lam, wt, W, ref)
            break
    assert found is not None, "no run crosses a seam at any of the weights tried (test setup)"
    lam, wt, W, ref = found
    seams = [30.0 * (i + 1) for i, s in enumerate((1500, 3000)) if kind[ref[s]] == 2]
    I.infer_audio(p, cfg_path, ckpt, str(tmp_path / "long.lab"), decode="viterbi", switch_penalty=lam, phoneme_bigram=bg, bigram_weight=wt,
                  bigram_scores=True)
    _, counts, rows = _tsv(tmp_path / "long.decode_scores.tsv")
    assert len(rows) == int((kind[ref] == 1).sum())           # a seam that cut a run in two would add a line
    for t in seams:
        assert sum(1 for r in rows if int(r[0]) < I._lab_int(t) < int(r[1])) == 1
    fs, _, ids, _ = _direct(lab, p, W)
    assert (ids == ref).all() and len(fs.runs) == len(rows)
    assert [float(r[3]) for r in rows] == pytest.approx([r.posterior for r in fs.runs], abs=2e-6)


def test_the_config_key_selects_it_and_decode_scores_is_still_refused(world):
    d, lab, cfg_path, ckpt, bg, kw = world
    p = [str(d / "wavs" / "a.wav")]
    want = lab.label_files(p, bigram_scores=True, **kw)
    assert isinstance(want, tuple) and isinstance(want[1][0], DC.FreeScore)
    lab.config["postprocess"].update(bigram_scores=True, **kw)
    try:
        assert lab.label_files(p) == want
        assert lab.label_files(p, bigram_scores=False) == want[0]
        with pytest.raises(ValueError, match="decode_scores cannot be combined"):
            lab.label_files(p, decode_scores=True)
    finally:
        for k in ("bigram_scores", *kw):
            del lab.config["postprocess"][k]
    with pytest.raises(ValueError, match="decode_scores cannot be combined"):
        lab.label_files(p, decode_scores=True, **kw)
    with pytest.raises(ValueError, match="decode_scores cannot be combined"):
        I.infer_folder(str(d / "wavs"), cfg_path, ckpt, str(d / "never"), decode_scores=True, **kw)
    with pytest.raises(ValueError, match="bigram_scores needs a phoneme_bigram"):
        lab.label_files(p, decode="viterbi", bigram_scores=True)
    assert not os.path.exists(d / "never") or not glob.glob(str(d / "never" / "*"))


def test_a_file_that_falls_back_to_argmax_gets_no_scores(world, tmp_path, capsys):
    """A stub class table that uses one class twice makes wfl_decode_bigram report status 4 for every clip: no fault is provoked."""
    d, lab, cfg_path, ckpt, bg, kw = world
    lab.label_files([str(d / "wavs" / "a.wav")], **kw)                # (the transition table is cached with the real class table)
    capsys.readouterr()
    lab._decode_table = (LABELS.index("O"), [(0, 1)] * 6)
    try:
        I.infer_folder(str(d / "wavs"), cfg_path, ckpt, str(tmp_path / "fb"), bigram_scores=True, **kw)
    finally:
        lab._decode_table = None
    text = capsys.readouterr().out
    assert text.count("viterbi decode not possible (wfl_decode_bigram status 4); using the argmax decode") == len(NAMES)
    assert not glob.glob(str(tmp_path / "fb" / "*.decode_scores.tsv"))
    assert open(tmp_path / "fb" / "decode_scores.tsv").read().count("\n") == 1          # the review list: its header alone
    assert len(glob.glob(str(tmp_path / "fb" / "*.lab"))) == len(NAMES)
