"""-m gpu: the bigram adaptation end to end on the synthetic tiny Whisper checkpoint, label set and 7 s / 65 s files of
tests/test_gpu_decode_bigram_e2e.py (the fixture is rebuilt here): Labeler.expected_successions against the float64 reference
(tests/bio_bigram_counts_ref.py) over the forward's own logits, the 65 s file being ONE clip across its 30 s seams;
`python -m wfl_asr_amd.adapt_bigram` in a child process and its result in `infer.py --decode viterbi --phoneme-bigram`; an --init
file's forbidden successions; the EM bound of the printed figure; and that nothing else changes.

Tolerances: the yardstick rule of tests/test_gpu_decode_bigram_counts.py (the float32 restatement's deviation from float64 on the same
inputs, x 4, plus half an fp32 ulp where that exceeds it), per file, the files' allowances added up for the summed outputs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import bio_bigram_counts_ref as BC
import synthetic as synth
from cases import tiny_whisper_config
from test_gpu_decode_bigram_posterior import _allowed
from wfl_asr_amd import adapt_bigram as AB
from wfl_asr_amd import audio as A
from wfl_asr_amd import decode as DC
from wfl_asr_amd import infer as I
from wfl_asr_amd import native_post as npost
from wfl_asr_amd import phonotactics as PH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHONES = ("p00", "p01", "p02", "p03", "SP", "AP")
LABELS = sorted(["O"] + [f"{t}-{p}" for p in PHONES for t in ("B", "I")])
FILES = ("a.wav", "long.wav")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp("adapt")
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
    # a bigram file in an order of its own, a fifth of the successions forbidden (never a way into O)
    rng = np.random.default_rng(5)
    syms = ["O"] + list(PHONES[::-1])
    lp = -6.0 * rng.random((7, 7))
    mask = rng.random((7, 7)) < 0.2
    mask[:, 0] = False
    lp[mask] = -np.inf
    PH.save(PH.Bigram(syms, lp), str(d / "phoneme_bigram.json"))
    return d, I.Labeler(str(d / "config.yaml"), str(d / "best_model.pt")), str(d / "phoneme_bigram.json")


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


@pytest.fixture(scope="module")
def reference(setup):
    """Per file, under the uniform start table at weight 1, penalty 0: the logits, the float64 (logz, counts), the yardsticks; and the
    table."""
    d, lab, _ = setup
    table = DC.class_table(LABELS)
    W = PH.transition_table(AB.start_bigram(LABELS), table, LABELS, 0.0, 1.0)
    out = {}
    for n in FILES:
        z, n_chunks = _file_logits(lab, str(d / "wavs" / n))
        assert (n_chunks == 3) == (n == "long.wav")
        r64 = BC.expected_counts(z, table, W.astype(np.float64), None)
        r32 = BC.expected_counts(z, table, W.astype(np.float64), None, dtype=np.float32)
        out[n] = dict(z=z, logz=r64[0], counts=r64[1], yard_logz=abs(r32[0] - r64[0]), yard_counts=float(np.abs(r32[1] - r64[1]).max()))
    return W, out


def test_expected_successions_equal_the_float64_reference_over_the_forward_s_logits(setup, reference):
    d, lab, _ = setup
    W, ref = reference
    paths = [str(d / "wavs" / n) for n in FILES]
    counts, logz, lse, frames, skipped = lab.expected_successions(paths, W, verbose=False)
    assert skipped == [] and counts.dtype == np.float64 and counts.shape == (7, 7)
    want = sum(ref[n]["counts"] for n in FILES)
    allowed = sum(_allowed(ref[n]["yard_counts"], ref[n]["counts"]) for n in FILES)
    dev = np.abs(counts - want)
    print(f"counts: kernel {dev.max():.3e}, float32 restatement {sum(ref[n]['yard_counts'] for n in FILES):.3e} (the two files' added), "
          f"allowed up to {allowed.max():.3e}; total {counts.sum():.3f} of {want.sum():.3f}")
    want_z = sum(ref[n]["logz"] for n in FILES)
    allowed_z = sum(float(_allowed(ref[n]["yard_logz"], ref[n]["logz"])) for n in FILES)
    print(f"logz: kernel {abs(logz - want_z):.3e}, allowed {allowed_z:.3e}")
    assert (dev <= allowed).all()
    assert abs(logz - want_z) <= allowed_z
    assert counts[0, 0] == 0 and (counts >= 0).all() and want.max() > 0.5
    # one clip across the seams: the reference cut at the 30 s seams gives other counts (every chunk starts after a virtual O)
    z = ref["long.wav"]["z"]
    cut = sum(BC.expected_counts(z[a:a + 1500], DC.class_table(LABELS), W.astype(np.float64), None)[1] for a in range(0, len(z), 1500))
    assert np.abs(cut - ref["long.wav"]["counts"]).max() > 10 * float(allowed.max()), "the seams make no difference (test setup)"
    # frames and the summed log-sum-exp against the host.  The device takes each frame's log-sum-exp in fp32 (C = 13 classes: a few
    # roundings of values near |lse|) and sums in double: 4 fp32 ulps of the largest |lse| per frame, errors taken not to cancel
    n_host = sum(len(ref[n]["z"]) for n in FILES)
    assert frames == n_host == 350 + 3250
    zz = np.concatenate([ref[n]["z"] for n in FILES]).astype(np.float64)
    m = zz.max(axis=1)
    lse_rows = m + np.log(np.exp(zz - m[:, None]).sum(axis=1))
    bound = n_host * 4 * float(np.spacing(np.float32(np.abs(lse_rows).max())))
    print(f"sum lse: device {lse:.6f} host {lse_rows.sum():.6f}, differ by {abs(lse - lse_rows.sum()):.3e}, bound {bound:.3e}")
    assert abs(lse - lse_rows.sum()) <= bound


def _round_lines(text):
    return [ln for ln in text.splitlines() if re.match(r"round \d+: ", ln)]


def _figure(line):
    return float(re.search(r"(-?\d+\.\d+) nats per frame", line).group(1))


def _lab_bytes(segs):
    return npost.format_lab_tuples(segs)


def test_the_cli_in_a_child_process_and_its_result_in_infer(setup, tmp_path):
    d, lab, _ = setup
    paths = [str(d / "wavs" / n) for n in FILES]
    before = [_lab_bytes(s) for s in lab.label_files(paths)]
    out = str(tmp_path / "adapted.json")
    r = subprocess.run([sys.executable, "-m", "wfl_asr_amd.adapt_bigram", str(d / "wavs"), "-ckpt", str(d / "best_model.pt"), "-c",
                        str(d / "config.yaml"), "-o", out, "--iterations", "2"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    lines = _round_lines(r.stdout)
    assert len(lines) == 2 and all("2 files, 3600 frames" in ln for ln in lines), r.stdout
    bg = PH.load(out)
    assert bg.symbols == AB.symbols_of(LABELS)
    p = np.exp(bg.log_prob)
    assert np.abs(p.sum(axis=1) - 1).max() <= 1e-12 and p[0, 0] == 0
    table = DC.class_table(LABELS)
    DC.check_transitions(PH.transition_table(bg, table, LABELS, 0.5, 1.0), len(table.pairs))
    # the table moved away from the uniform start
    assert np.abs(p - np.exp(AB.start_bigram(LABELS).log_prob)).max() > 0.05
    os.makedirs(tmp_path / "labs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), str(d / "wavs"), "-ckpt", str(d / "best_model.pt"), "-c",
                        str(d / "config.yaml"), "-o", str(tmp_path / "labs"), "--decode", "viterbi", "--phoneme-bigram", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path / "labs")) == ["a.lab", "long.lab"]
    # with no bigram key set, the labels are what they were
    assert [_lab_bytes(s) for s in lab.label_files(paths)] == before and all(len(b) for b in before)


def test_what_the_init_file_forbids_stays_forbidden(setup, tmp_path, capsys):
    d, lab, init = setup
    out = str(tmp_path / "adapted.json")
    AB.main([str(d / "wavs"), "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml"), "-o", out, "--init", init,
             "--iterations", "1", "--smoothing", "0.5", "--prior-count", "1"])
    assert len(_round_lines(capsys.readouterr().out)) == 1
    a, b = PH.load(init), PH.load(out)
    shut = 0
    for i, s in enumerate(a.symbols):
        for j, q in enumerate(a.symbols):
            if (i, j) != (0, 0) and np.isneginf(a.log_prob[i, j]):
                shut += 1
                assert np.isneginf(b.log_prob[b.symbols.index(s), b.symbols.index(q)]), (s, q)
            elif (i, j) != (0, 0):
                assert np.isfinite(b.log_prob[b.symbols.index(s), b.symbols.index(q)]), (s, q)
    assert shut >= 3
    assert np.abs(np.exp(b.log_prob).sum(axis=1) - 1).max() <= 1e-12


def test_the_printed_figure_does_not_decrease_under_the_em_settings(setup, reference, tmp_path, capsys):
    d, lab, _ = setup
    _, ref = reference
    AB.main([str(d / "wavs"), "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml"), "-o", str(tmp_path / "em.json"),
             "--bigram-weight", "1", "--switch-penalty", "0", "--smoothing", "0", "--iterations", "3"])
    lines = _round_lines(capsys.readouterr().out)
    assert len(lines) == 3
    figs = [_figure(ln) for ln in lines]
    # the logz allowance of the two files by the kernel test's rule, per frame (and the last printed digit)
    per_frame = sum(float(_allowed(ref[n]["yard_logz"], ref[n]["logz"])) for n in FILES) / 3600 + 1e-9
    print("nats per frame:", figs, "allowance per frame", per_frame)
    assert all(b >= a - per_frame for a, b in zip(figs, figs[1:])), figs
    assert figs[-1] > figs[0] and all(f <= 0 for f in figs)
