"""-m gpu: the duration prior's re-estimation end to end on the synthetic tiny Whisper checkpoint, label set and 7 s / 65 s files of
tests/test_gpu_adapt_bigram_e2e.py (the fixture is rebuilt here, with seeded `.txt` transcripts of 40 and 300 tokens: two launch
configurations, the long file across two 30 s seams): Labeler.expected_durations against the float64 reference
(tests/duration_prior_counts_ref.py) over the forward's own logits; `python -m wfl_asr_amd.adapt_durations` in a child process and its
result in `infer.py --align viterbi --duration-prior`; an --init file's forbidden entries; the EM bound of the printed figure; and that
nothing else changes.

Tolerances: the yardstick rule of tests/test_gpu_align_duration_prior_counts.py (the float32 restatement's deviation from float64 on
the same inputs, x 4, plus half an fp32 ulp where that exceeds it), per file and per output (the probabilities, the excess, logz), a
token's allowance added to its phoneme's row, the files' allowances added up for the summed outputs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import duration_prior_counts_ref as CR
import synthetic as synth
from cases import tiny_whisper_config
from test_gpu_adapt_bigram_e2e import _file_logits
from test_gpu_align_duration_prior_posterior import _half_ulp
from wfl_asr_amd import adapt_durations as AD
from wfl_asr_amd import align as AL
from wfl_asr_amd import audio as A
from wfl_asr_amd import durations as DU
from wfl_asr_amd import infer as I
from wfl_asr_amd import native_post as npost

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHONES = ("p00", "p01", "p02", "p03", "SP", "AP")
LABELS = sorted(["O"] + [f"{t}-{p}" for p in PHONES for t in ("B", "I")])
FILES = ("a.wav", "long.wav")
TOKENS = {"a.wav": 40, "long.wav": 300}
D = 8


def _transcript(n, rng):
    out = []
    for _ in range(n):
        while True:
            p = PHONES[int(rng.integers(0, 4))]
            if not out or p != out[-1]:
                break
        out.append(p)
    return out


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp("adapt_durations")
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
    rng = np.random.default_rng(77)
    trs = {}
    for n in FILES:
        trs[n] = _transcript(TOKENS[n], rng)
        with open(d / "wavs" / n.replace(".wav", ".txt"), "w") as f:
            f.write(" ".join(trs[n]) + "\n")
    return d, I.Labeler(str(d / "config.yaml"), str(d / "best_model.pt")), trs


def _clip_args(lab, tr, prior):
    remap, names = lab._names_for(None)
    alts, why = AL.token_alternatives(tr, lab._table, remap, names, lab.labels)
    assert alts is not None, why
    return alts, AL.gap_classes(lab.labels, tr), AL.duration_rows(tr, prior)


def _allowed(yard, ref):
    h = _half_ulp(ref)
    return 4 * yard + np.where(yard < h, h, 0.0)


@pytest.fixture(scope="module")
def reference(setup):
    """Per file, under the flat prior at weight 1: the logits, the float64 (logz, dur_post), the per-token allowances, the rows."""
    d, lab, trs = setup
    names = lab._names_for(None)[1]
    prior = DU.flat(names, D, I.frame_duration)
    table = DU.table(prior, 1.0)
    out = {}
    for n in FILES:
        z, n_chunks = _file_logits(lab, str(d / "wavs" / n))
        assert (n_chunks == 3) == (n == "long.wav")
        alts, gaps, rows = _clip_args(lab, trs[n], prior)
        r64 = CR.expected_counts(z, alts, gaps, rows, table)
        r32 = CR.expected_counts(z, alts, gaps, rows, table, dtype=np.float32)
        dev = np.abs(r32["dur_post"] - r64["dur_post"])
        allow = np.empty_like(dev)
        allow[:, :D] = _allowed(float(dev[:, :D].max()), r64["dur_post"][:, :D])
        allow[:, D] = _allowed(float(dev[:, D].max()), r64["dur_post"][:, D])
        out[n] = dict(z=z, alts=alts, gaps=gaps, rows=rows, logz=r64["logz"], dur_post=r64["dur_post"], allow=allow,
                      allow_logz=float(_allowed(abs(r32["logz"] - r64["logz"]), r64["logz"])))
    return prior, table, out


def _per_phoneme(n_rows, rows, per_token):
    out = np.zeros((n_rows, per_token.shape[1]))
    r = np.asarray(rows)
    np.add.at(out, r[r >= 0], per_token[r >= 0])
    return out


def test_expected_durations_equal_the_float64_reference_over_the_forward_s_logits(setup, reference):
    d, lab, trs = setup
    prior, table, ref = reference
    paths = [str(d / "wavs" / n) for n in FILES]
    counts, logz, frames, tokens, skipped = lab.expected_durations(paths, [trs[n] for n in FILES], prior, verbose=False)
    nr = len(prior.phonemes)
    assert skipped == [] and counts.dtype == np.float64 and counts.shape == (nr, D + 1)
    assert frames == 350 + 3250 and tokens == 340
    want = sum(_per_phoneme(nr, ref[n]["rows"], ref[n]["dur_post"]) for n in FILES)
    allowed = sum(_per_phoneme(nr, ref[n]["rows"], ref[n]["allow"]) for n in FILES)
    dev = np.abs(counts - want)
    print(f"counts: kernel {dev.max():.3e}, allowed up to {allowed.max():.3e}; over by {max(float((dev - allowed).max()), 0.0):.3e}; "
          f"runs {counts[:, :D].sum():.3f} of {want[:, :D].sum():.3f}")
    want_z = sum(ref[n]["logz"] for n in FILES)
    allowed_z = sum(ref[n]["allow_logz"] for n in FILES)
    print(f"logz: kernel {abs(logz - want_z):.3e}, allowed {allowed_z:.3e}")
    assert (dev <= allowed).all()
    assert abs(logz - want_z) <= allowed_z
    assert (counts >= 0).all() and abs(want[:, :D].sum() - 340) < 1e-6                # (a run per token in the reference)
    used = [prior.phonemes.index(p) for p in PHONES[:4]]
    assert (counts[used, :D].sum(axis=1) > 10).all() and not np.delete(counts, used, axis=0).any()
    # one clip across the seams: the reference cut at the 30 s seams, each piece with its share of the transcript, gives other counts
    r = ref["long.wav"]
    z, cut, k0 = r["z"], np.zeros_like(want), 0
    for a in range(0, len(z), 1500):
        n = len(z[a:a + 1500]) * 300 // len(z) if a + 1500 < len(z) else 300 - k0
        piece = CR.expected_counts(z[a:a + 1500], r["alts"][k0:k0 + n], r["gaps"], r["rows"][k0:k0 + n], table)
        cut += _per_phoneme(nr, r["rows"][k0:k0 + n], piece["dur_post"])
        k0 += n
    whole = _per_phoneme(nr, r["rows"], r["dur_post"])
    assert k0 == 300 and np.abs(cut - whole).max() > 10 * float(allowed.max()), "the seams make no difference (test setup)"


def _round_lines(text):
    return [ln for ln in text.splitlines() if re.match(r"round \d+: ", ln)]


def _figure(line):
    return float(re.search(r"(-?\d+\.\d+) nats per frame", line).group(1))


def _mass(row, tail):
    p = np.exp(row)
    return p[:-1].sum() + (p[-1] / (1.0 - np.exp(tail)) if p[-1] > 0 else 0.0)


def test_the_cli_in_a_child_process_and_its_result_in_infer(setup, tmp_path):
    d, lab, trs = setup
    paths = [str(d / "wavs" / n) for n in FILES]
    before = [npost.format_lab_tuples(s) for s in lab.label_files(paths)]
    out = str(tmp_path / "phoneme_durations.json")
    r = subprocess.run([sys.executable, "-m", "wfl_asr_amd.adapt_durations", str(d / "wavs"), "-ckpt", str(d / "best_model.pt"), "-c",
                        str(d / "config.yaml"), "-o", out, "--iterations", "2", "--max-frames", str(D)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    lines = _round_lines(r.stdout)
    assert len(lines) == 2 and all("2 files, 3600 frames, 340 tokens" in ln for ln in lines), r.stdout
    prior = DU.load(out)
    names = lab._names_for(None)[1]
    DU.check(prior, names, I.frame_duration)
    assert prior.max_frames == D and prior.phonemes == list(names)
    flat = DU.flat(names, D, I.frame_duration)
    moved = 0.0
    for p, row, tail in zip(prior.phonemes, prior.log_prob, prior.log_tail):
        if p in PHONES[:4]:
            assert row is not None and abs(_mass(row, tail) - 1) < 1e-9, p
            moved = max(moved, float(np.abs(np.exp(row) - np.exp(flat.log_prob[0])).max()))
        else:
            assert row is None, p                                # in no transcript: a null row
    assert moved > 0.05
    os.makedirs(tmp_path / "labs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), str(d / "wavs"), "-ckpt", str(d / "best_model.pt"), "-c",
                        str(d / "config.yaml"), "-o", str(tmp_path / "labs"), "--align", "viterbi", "--duration-prior", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path / "labs")) == ["a.lab", "long.lab"]
    # with no duration-prior key set, the labels are what they were
    assert [npost.format_lab_tuples(s) for s in lab.label_files(paths)] == before and all(len(b) for b in before)


def test_what_the_init_file_forbids_stays_forbidden(setup, tmp_path, capsys):
    d, lab, _ = setup
    names = list(lab._names_for(None)[1])
    init = DU.flat(names, 6, I.frame_duration)
    init.log_prob[names.index("p00")][0] = -np.inf               # never one frame
    init.log_prob[names.index("p02")][3] = -np.inf               # never four
    init.log_tail[names.index("p01")] = -np.inf                  # nothing longer than D
    DU.save(init, str(tmp_path / "init.json"))
    out = str(tmp_path / "adapted.json")
    AD.main([str(d / "wavs"), "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml"), "-o", out, "--init", str(tmp_path / "init.json"),
             "--iterations", "1", "--smoothing", "0.5", "--prior-count", "1"])
    lines = _round_lines(capsys.readouterr().out)
    assert len(lines) == 1 and "2 files" in lines[0]
    a, b = DU.load(str(tmp_path / "init.json")), DU.load(out)
    assert b.max_frames == 6 and b.phonemes == a.phonemes
    shut = 0
    for p, ra, rb, ta, tb in zip(a.phonemes, a.log_prob, b.log_prob, a.log_tail, b.log_tail):
        assert (np.isneginf(ra) == np.isneginf(rb)).all() and np.isneginf(ta) == np.isneginf(tb), p
        shut += int(np.isneginf(ra).sum()) + int(np.isneginf(ta))
        assert abs(_mass(rb, tb) - 1) < 1e-9
    assert shut == 3
    assert any(not np.allclose(ra, rb) for ra, rb in zip(a.log_prob, b.log_prob))


def test_the_printed_figure_does_not_decrease_under_the_em_settings(setup, reference, tmp_path, capsys):
    d, lab, _ = setup
    _, _, ref = reference
    AD.main([str(d / "wavs"), "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml"), "-o", str(tmp_path / "em.json"),
             "--duration-prior-weight", "1", "--smoothing", "0", "--iterations", "3", "--max-frames", str(D)])
    lines = _round_lines(capsys.readouterr().out)
    assert len(lines) == 3
    figs = [_figure(ln) for ln in lines]
    # the logz allowance of the two files by the kernel test's rule, per frame (and the last printed digit)
    per_frame = sum(ref[n]["allow_logz"] for n in FILES) / 3600 + 1e-9
    print("nats per frame:", figs, "allowance per frame", per_frame)
    assert all(b >= a - per_frame for a, b in zip(figs, figs[1:])), figs
    assert figs[-1] > figs[0]
