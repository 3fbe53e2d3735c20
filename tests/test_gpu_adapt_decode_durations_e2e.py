"""-m gpu: the free decode's duration EM end to end on the synthetic tiny Whisper checkpoint, label set and 7 s / 65 s files of
tests/test_gpu_adapt_bigram_e2e.py (the fixture is rebuilt here): Labeler.expected_free_durations against the float64 reference
(tests/bio_duration_counts_ref.py) over the forward's own logits under a seeded prior and bigram, the 65 s file being ONE clip across
its 30 s seams; two phonemes under one output name; `python -m wfl_asr_amd.adapt_decode_durations` in a child process and its result
in `infer.py --decode viterbi --decode-duration-prior`; an --init file's forbidden entries; --bigram-output; the EM bound of the
printed figure; and that nothing else changes.

Tolerances: the yardstick rule of tests/test_gpu_decode_duration_counts.py (the float32 restatement's deviation from float64 on the
same inputs, x 4, plus half an fp32 ulp where that exceeds it), per file, the files' allowances added up for the summed outputs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import bio_duration_counts_ref as CR
import synthetic as synth
from cases import tiny_whisper_config
from test_gpu_decode_bigram_posterior import _allowed
from wfl_asr_amd import adapt_bigram as AB
from wfl_asr_amd import audio as A
from wfl_asr_amd import decode as DC
from wfl_asr_amd import durations as DU
from wfl_asr_amd import infer as I
from wfl_asr_amd import native_post as npost
from wfl_asr_amd import phonotactics as PH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHONES = ("p00", "p01", "p02", "p03", "SP", "AP")
LABELS = sorted(["O"] + [f"{t}-{p}" for p in PHONES for t in ("B", "I")])
FILES = ("a.wav", "long.wav")
D = 8


def _seeded_prior(names, rng):
    """Rows that sum to 1 with their tails, a sixth of the entries forbidden, one tail forbidden, one phoneme without a row."""
    rows, tails = [], []
    for i, _ in enumerate(names):
        p = rng.random(D) + 0.05
        p[rng.random(D) < 1 / 6] = 0.0
        p[D - 1] = max(p[D - 1], 0.2)
        p /= p.sum()
        with np.errstate(divide="ignore"):
            rows.append(None if i == 4 else np.log(p))
        tails.append(-np.inf if i == 2 else float(np.log(0.3 + 0.5 * rng.random())))
    return DU.DurationPrior(I.frame_duration, D, list(names), rows, np.array(tails, np.float64))


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp("adapt_dd")
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
    rng = np.random.default_rng(5)
    syms = ["O"] + list(PHONES[::-1])
    lp = -6.0 * rng.random((7, 7))
    mask = rng.random((7, 7)) < 0.2
    mask[:, 0] = False
    lp[mask] = -np.inf
    PH.save(PH.Bigram(syms, lp), str(d / "phoneme_bigram.json"))
    DU.save(_seeded_prior(PHONES, rng), str(d / "phoneme_durations.json"))
    return d, I.Labeler(str(d / "config.yaml"), str(d / "best_model.pt")), str(d / "phoneme_bigram.json"), str(d / "phoneme_durations.json")


def _file_logits(lab, path):
    """The file's chunks through model.label(want_logits=True), one chunk per forward -> z of the valid frames, concatenated."""
    zs = []
    for c in lab._load_chunks(path):
        x = np.zeros((lab.batch_size, lab.chunk_samples), np.float32)
        x[0, :len(c)] = c
        lens = np.zeros(lab.batch_size, np.int32)
        lens[0] = len(c)
        res = lab.model.label(torch.from_numpy(x).cuda(), None, threshold=0.0, lens=lens, average_languages=True, want_logits=True)
        zs.append(res.logits[0, :lab._valid_frames(len(c), res.ids.shape[1])].cpu().numpy())
    return np.concatenate(zs), len(zs)


def _ref(z, table, W, dur, sym_dur):
    r64 = CR.expected_counts(z, table, W.astype(np.float64), dur, sym_dur, None)
    r32 = CR.expected_counts(z, table, W.astype(np.float64), dur, sym_dur, None, dtype=np.float32)
    return dict(logz=r64[0], succ=r64[1], dur=r64[2], yard_logz=abs(r32[0] - r64[0]), yard_succ=float(np.abs(r32[1] - r64[1]).max()),
                yard_dur=float(np.abs(r32[2] - r64[2]).max()))


@pytest.fixture(scope="module")
def reference(setup):
    """Per file, under the seeded bigram (weight 1, penalty 0) and the seeded prior (weight 1): the logits, the float64 results and the
    yardsticks; the tables."""
    d, lab, bigram, prior_path = setup
    table = DC.class_table(LABELS)
    W = PH.transition_table(PH.load(bigram), table, LABELS, 0.0, 1.0)
    prior = DU.load(prior_path)
    dur = DU.table(prior, 1.0)
    sym_dur = DC.duration_symbol_rows(prior, table, LABELS)
    out = {}
    for n in FILES:
        z, n_chunks = _file_logits(lab, str(d / "wavs" / n))
        assert (n_chunks == 3) == (n == "long.wav")
        out[n] = dict(z=z, **_ref(z, table, W, dur, sym_dur))
    return W, prior, dur, sym_dur, out


def _rows_of(dc, prior):
    """[symbols, D + 1] in the class table's order -> [len(prior.phonemes), D + 1] by name."""
    names = AB.symbols_of(LABELS)[1:]
    out = np.zeros((len(prior.phonemes), dc.shape[1]))
    for p, nm in enumerate(names):
        out[prior.phonemes.index(nm)] += dc[p]
    return out


def test_expected_free_durations_equal_the_float64_reference_over_the_forward_s_logits(setup, reference):
    d, lab, _, _ = setup
    W, prior, dur, sym_dur, ref = reference
    paths = [str(d / "wavs" / n) for n in FILES]
    counts, succ, logz, lse, frames, skipped = lab.expected_free_durations(paths, W, prior, verbose=False)
    assert skipped == [] and counts.dtype == succ.dtype == np.float64 and counts.shape == (6, D + 1) and succ.shape == (7, 7)
    assert frames == 350 + 3250
    want_d = sum(_rows_of(ref[n]["dur"], prior) for n in FILES)
    allow_d = sum(_rows_of(_allowed(ref[n]["yard_dur"], ref[n]["dur"]), prior) for n in FILES)
    want_s = sum(ref[n]["succ"] for n in FILES)
    allow_s = sum(_allowed(ref[n]["yard_succ"], ref[n]["succ"]) for n in FILES)
    want_z = sum(ref[n]["logz"] for n in FILES)
    allow_z = sum(float(_allowed(ref[n]["yard_logz"], ref[n]["logz"])) for n in FILES)
    print(f"dur_counts: kernel {np.abs(counts - want_d).max():.3e}, allowed up to {allow_d.max():.3e}; runs {counts[:, :D].sum():.3f} of "
          f"{want_d[:, :D].sum():.3f}")
    print(f"succ: kernel {np.abs(succ - want_s).max():.3e}, allowed up to {allow_s.max():.3e}")
    print(f"logz: kernel {abs(logz - want_z):.3e}, allowed {allow_z:.3e}")
    assert (np.abs(counts - want_d) <= allow_d).all() and (np.abs(succ - want_s) <= allow_s).all() and abs(logz - want_z) <= allow_z
    assert want_d.max() > 0.5 and want_d[:, D].any()
    # what the prior forbids is exactly 0
    for i, r in enumerate(prior.log_prob):
        if r is not None:
            assert (counts[i, :D][np.isneginf(r)] == 0).all()
            if np.isneginf(prior.log_tail[i]):
                assert counts[i, D] == 0
    # one clip across the seams: the reference cut at the 30 s seams (every chunk then starts after a virtual O and ends its last run)
    # gives counts that the same check would refuse
    z = ref["long.wav"]["z"]
    table = DC.class_table(LABELS)
    cut = sum(CR.expected_counts(z[a:a + 1500], table, W.astype(np.float64), dur, sym_dur, None)[2] for a in range(0, len(z), 1500))
    want_cut = _rows_of(cut, prior) + _rows_of(ref["a.wav"]["dur"], prior)
    print(f"cut at the seams: off by {np.abs(counts - want_cut).max():.3e}")
    assert not (np.abs(counts - want_cut) <= allow_d).all(), "the seams make no difference (test setup)"
    # the summed log-sum-exp against the host (tests/test_gpu_adapt_bigram_e2e.py's bound)
    zz = np.concatenate([ref[n]["z"] for n in FILES]).astype(np.float64)
    m = zz.max(axis=1)
    lse_rows = m + np.log(np.exp(zz - m[:, None]).sum(axis=1))
    assert abs(lse - lse_rows.sum()) <= len(zz) * 4 * float(np.spacing(np.float32(np.abs(lse_rows).max())))


def test_two_phonemes_under_one_output_name_land_in_one_row(setup, reference):
    """p01 is written as p00 (the merge map's back-mapping, put into the Labeler's name cache): both symbols read p00's row of the
    prior and their counts add into it."""
    d, lab, _, _ = setup
    W, prior, _, _, ref = reference
    names = [n for n in PHONES if n != "p01"]
    keep = [PHONES.index(n) for n in names]
    merged = DU.DurationPrior(prior.frame_duration, D, names, [prior.log_prob[i] for i in keep], prior.log_tail[keep])
    table_names = list(lab._table.names)
    uniq = [n for n in table_names if n != "p01"]
    remap = np.array([uniq.index("p00" if n == "p01" else n) for n in table_names], np.int32)
    saved = dict(lab._names_cache)
    lab._names_cache[None] = (remap, uniq)
    try:
        path = str(d / "wavs" / "a.wav")
        counts, succ, logz, _, frames, skipped = lab.expected_free_durations([path], W, merged, verbose=False)
    finally:
        lab._names_cache.clear()
        lab._names_cache.update(saved)
    assert skipped == [] and counts.shape == (5, D + 1)
    table = DC.class_table(LABELS)
    syms = AB.symbols_of(LABELS)[1:]
    sym_dur = np.array([-1 if merged.log_prob[names.index("p00" if s == "p01" else s)] is None else names.index("p00" if s == "p01" else s)
                        for s in syms], np.int32)
    r = _ref(ref["a.wav"]["z"], table, W, DU.table(merged, 1.0), sym_dur)
    want, allow = np.zeros((5, D + 1)), np.zeros((5, D + 1))
    for p, s in enumerate(syms):
        want[names.index("p00" if s == "p01" else s)] += r["dur"][p]
        allow[names.index("p00" if s == "p01" else s)] += _allowed(r["yard_dur"], r["dur"][p])
    print(f"merged rows: kernel {np.abs(counts - want).max():.3e}, allowed up to {allow.max():.3e}")
    assert (np.abs(counts - want) <= allow).all()
    both = r["dur"][syms.index("p00")], r["dur"][syms.index("p01")]
    assert both[0].sum() > 1e-3 and both[1].sum() > 1e-3, "one of the two phonemes never runs (test setup)"


def _round_lines(text):
    return [ln for ln in text.splitlines() if re.match(r"round \d+: ", ln)]


def _figure(line):
    return float(re.search(r"(-?\d+\.\d+) nats per frame", line).group(1))


def _lab_bytes(segs):
    return npost.format_lab_tuples(segs)


def test_the_cli_in_a_child_process_its_em_bound_and_its_result_in_infer(setup, reference, tmp_path):
    d, lab, _, prior_path = setup
    _, _, _, _, ref = reference
    paths = [str(d / "wavs" / n) for n in FILES]
    before = [_lab_bytes(s) for s in lab.label_files(paths)]
    before_prior = [_lab_bytes(s) for s in lab.label_files(paths, decode="viterbi", decode_duration_prior=prior_path)]
    out = str(tmp_path / "adapted.json")
    r = subprocess.run([sys.executable, "-m", "wfl_asr_amd.adapt_decode_durations", str(d / "wavs"), "-ckpt", str(d / "best_model.pt"), "-c",
                        str(d / "config.yaml"), "-o", out, "--iterations", "3", "--max-frames", str(D), "--smoothing", "0",
                        "--decode-duration-prior-weight", "1", "--bigram-weight", "1", "--switch-penalty", "0"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    lines = _round_lines(r.stdout)
    assert len(lines) == 3 and all("2 files, 3600 frames" in ln and " runs, " in ln for ln in lines), r.stdout
    figs = [_figure(ln) for ln in lines]
    per_frame = sum(float(_allowed(ref[n]["yard_logz"], ref[n]["logz"])) for n in FILES) / 3600 + 1e-9
    print("nats per frame:", figs, "allowance per frame", per_frame)
    assert all(b >= a - per_frame for a, b in zip(figs, figs[1:])), figs
    assert figs[-1] > figs[0]
    prior = DU.load(out)
    DU.check(prior, lab._names_for(None)[1], I.frame_duration)
    assert prior.max_frames == D and sorted(prior.phonemes) == sorted(PHONES)
    for row, tail in zip(prior.log_prob, prior.log_tail):
        if row is not None:                         # a distribution over d >= 1: sum_{d < D} P(d) + P(D) / (1 - rho) = 1
            assert abs(np.exp(row[:D - 1]).sum() + np.exp(row[D - 1]) / (1 - np.exp(tail)) - 1) <= 1e-9
    assert any(row is not None for row in prior.log_prob)
    os.makedirs(tmp_path / "labs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), str(d / "wavs"), "-ckpt", str(d / "best_model.pt"), "-c",
                        str(d / "config.yaml"), "-o", str(tmp_path / "labs"), "--decode", "viterbi", "--decode-duration-prior", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path / "labs")) == ["a.lab", "long.lab"]
    # with the existing keys, the labels are what they were before the new module ran
    assert [_lab_bytes(s) for s in lab.label_files(paths)] == before and all(len(b) for b in before)
    assert [_lab_bytes(s) for s in lab.label_files(paths, decode="viterbi", decode_duration_prior=prior_path)] == before_prior


def test_what_the_init_file_forbids_stays_null_and_the_bigram_output_loads(setup, tmp_path, capsys):
    from wfl_asr_amd import adapt_decode_durations as AD
    d, lab, bigram, init = setup
    out, bg_out = str(tmp_path / "adapted.json"), str(tmp_path / "bigram.json")
    AD.main([str(d / "wavs" / "a.wav"), "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml"), "-o", out, "--init", init,
             "--iterations", "2", "--smoothing", "0.5", "--prior-count", "1", "--phoneme-bigram", bigram, "--bigram-output", bg_out])
    assert len(_round_lines(capsys.readouterr().out)) == 2
    a, b = DU.load(init), DU.load(out)
    assert a.phonemes == b.phonemes and b.max_frames == D
    shut = 0
    for ra, rb, ta, tb in zip(a.log_prob, b.log_prob, a.log_tail, b.log_tail):
        if ra is None:
            continue
        assert rb is not None and (np.isneginf(ra) == np.isneginf(rb)).all()
        assert np.isneginf(ta) == np.isneginf(tb)
        shut += int(np.isneginf(ra).sum()) + int(np.isneginf(ta))
    assert shut >= 3
    # the bigram that came out loads as --phoneme-bigram does, and keeps what the start forbids
    got = AB.start_bigram(LABELS, bg_out)
    start = AB.start_bigram(LABELS, bigram)
    table = DC.class_table(LABELS)
    DC.check_transitions(PH.transition_table(got, table, LABELS, 0.0, 1.0), len(table.pairs))
    off = ~np.eye(7, dtype=bool) | (np.arange(7)[:, None] > 0)
    assert (np.isneginf(got.log_prob) == np.isneginf(start.log_prob))[off].all()
    assert np.abs(np.exp(got.log_prob).sum(axis=1) - 1).max() <= 1e-12
    assert np.abs(np.exp(got.log_prob) - np.exp(start.log_prob)).max() > 0.02, "the bigram did not move"
