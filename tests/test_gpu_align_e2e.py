"""-m gpu: `align="viterbi"` end to end on synthetic tiny checkpoints (Whisper geometry of 30 s windows, and WavLM with ragged clips):
one time-ordered segment per transcript token, the same segments as the numpy float64 DP over the forward's own logits, one search
across a long file's chunks, files without a transcript unchanged, the CLI flag."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import synthetic as synth
import viterbi_ref as V
from cases import tiny_wavlm_config, tiny_whisper_config
from wfl_asr_amd import align as AL
from wfl_asr_amd import audio as A
from wfl_asr_amd import infer as I
from wfl_asr_amd import postprocess as pp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = sorted(["O"] + [f"{t}-{p}" for p in ("p00", "p01", "p02", "p03", "SP", "AP") for t in ("B", "I")])


def _setup(d, cfg, seed):
    cfg["output"]["save_dir"] = str(d / "save")
    cfg["postprocess"] = {"median_filter": 3, "merge_segments": "right", "confidence_threshold": 0.3}
    os.makedirs(d / "save")
    with open(d / "save" / "phonemes.txt", "w") as f:
        f.write("\n".join(LABELS) + "\n")
    with open(d / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, len(LABELS), seed=seed).items()}
    torch.save(sd, d / "best_model.pt")
    os.makedirs(d / "wavs")
    return I.Labeler(str(d / "config.yaml"), str(d / "best_model.pt"))


@pytest.fixture(scope="module")
def whisper(tmp_path_factory):
    d = tmp_path_factory.mktemp("va")
    cfg = tiny_whisper_config(enable_bilstm=False)
    cfg["model"]["encoder_arch"]["max_positions"] = 1500
    lab = _setup(d, cfg, 41)
    A.write_wav(str(d / "wavs" / "a.wav"), synth.make_clip(800, 16000 * 7, seed=41) * 0.9, 16000)
    A.write_wav(str(d / "wavs" / "long.wav"), synth.make_clip(801, 16000 * 65, seed=41) * 0.8, 16000)
    A.write_wav(str(d / "wavs" / "plain.wav"), synth.make_clip(802, 16000 * 4, seed=41) * 0.7, 16000)
    return d, lab


def _write_tr(path, tokens):
    with open(path.replace(".wav", ".txt"), "w") as f:
        f.write(" ".join(tokens))


def _core(segs):
    return [s for s in segs if s[2] not in ("SP", "AP")]


def _check_segments(core, tr, total_s):
    assert [s[2] for s in core] == tr
    for i, (a, b, _) in enumerate(core):
        assert a <= b <= total_s + 1e-6
        if i:
            assert core[i - 1][1] <= a + 1e-9 and core[i - 1][0] < a


def _host_reference(lab, path, tr):
    """The same clip through model.label(want_logits=True) and the numpy float64 DP, assembled by the host helpers."""
    chunks = lab._load_chunks(path)
    assert len(chunks) == 1
    x = np.zeros((lab.batch_size, lab.chunk_samples), np.float32)
    x[0, :len(chunks[0])] = chunks[0]
    lens = np.zeros(lab.batch_size, np.int32)
    lens[0] = len(chunks[0])
    res = lab.model.label(torch.from_numpy(x).cuda(), None, threshold=0.3, lens=lens, average_languages=True, want_logits=True)
    T = res.ids.shape[1]
    tv = lab._valid_frames(len(chunks[0]), T)
    z = res.logits[0, :tv].cpu().numpy()
    offs = res.offsets[0, :tv].cpu().numpy()
    remap, names = lab._names_for(None)
    alts, why = AL.token_alternatives(tr, lab._table, remap, names, LABELS)
    assert why is None
    states, _ = V.viterbi(z, alts, AL.gap_classes(LABELS, tr))
    ids, tok = V.outputs(states, z, alts, LABELS.index("O"))
    return AL.path_segments(ids, tok, [tv], [offs], [0.0], lab._table, alts, tr, pp.FRAME_DURATION)


def test_viterbi_fixes_what_greedy_gets_wrong_and_equals_the_host_dp(whisper):
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    free = lab.label_files([path], confidence_threshold=0.3, align="greedy")[0]
    names = [s[2] for s in free if s[2] not in ("SP", "AP")]
    # a transcript the greedy match gets wrong: the decoded order reversed (its times would run backwards), tokens inserted
    tr = [t for t in reversed(names) if t in ("p00", "p01", "p02", "p03")][:40] + ["p03", "p00", "p03"]
    assert len(set(names)) >= 2, "the free decode has too few segments (test setup)"
    _write_tr(path, tr)
    try:
        greedy = lab.label_files([path], confidence_threshold=0.3, align="greedy")[0]
        got = lab.label_files([path], confidence_threshold=0.3, align="viterbi")[0]
    finally:
        os.remove(path.replace(".wav", ".txt"))
    g = _core(greedy)
    assert [s[2] for s in g] != tr or any(g[i][0] > g[i + 1][0] for i in range(len(g) - 1)), "greedy was right here (test setup)"
    core = _core(got)
    _check_segments(core, tr, 7.0)
    ref = _host_reference(lab, path, tr)
    assert core == ref


def test_long_file_one_search_across_chunks_and_files_without_transcript_unchanged(whisper, capsys):
    d, lab = whisper
    long_p, plain_p, a_p = (str(d / "wavs" / n) for n in ("long.wav", "plain.wav", "a.wav"))
    rng = np.random.default_rng(2)
    tr = [str(x) for x in rng.choice(["p00", "p01", "p02", "p03"], size=120)]
    _write_tr(long_p, tr)
    _write_tr(a_p, ["p00", "zz", "p01"])             # a token that matches no phoneme: greedy for this file, with a message
    try:
        greedy = lab.label_files([long_p, plain_p, a_p], confidence_threshold=0.3, align="greedy")
        capsys.readouterr()
        got = lab.label_files([long_p, plain_p, a_p], confidence_threshold=0.3, align="viterbi")
        out = capsys.readouterr().out
    finally:
        os.remove(long_p.replace(".wav", ".txt"))
        os.remove(a_p.replace(".wav", ".txt"))
    core = _core(got[0])
    _check_segments(core, tr, 65.0)
    assert any(s[0] < 30.0 for s in core) and any(s[1] > 60.0 for s in core)      # the path spans both seams
    assert got[1] == greedy[1]                                                      # no transcript: the greedy path, bit for bit
    assert "'zz'" in out and got[2] == greedy[2]


def test_empty_transcript_and_infeasible_fall_back(whisper, capsys):
    d, lab = whisper
    p = str(d / "wavs" / "plain.wav")
    _write_tr(p, [])
    try:
        assert lab.label_files([p], align="viterbi")[0] == []
        _write_tr(p, ["p00"] * 400)                      # 4 s = 200 frames: fewer frames than tokens
        greedy = lab.label_files([p], confidence_threshold=0.3, align="greedy")[0]
        capsys.readouterr()
        got = lab.label_files([p], confidence_threshold=0.3, align="viterbi")[0]
        assert "400 tokens for 200 frames" in capsys.readouterr().out and got == greedy
    finally:
        os.remove(p.replace(".wav", ".txt"))


def test_cli_align_viterbi_writes_the_lab(whisper, tmp_path):
    d, _ = whisper
    p = str(d / "wavs" / "a.wav")
    _write_tr(p, ["p00", "p01", "p02"])
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), p, "-ckpt", str(d / "best_model.pt"), "-c",
                            str(d / "config.yaml"), "-o", str(tmp_path / "a.lab"), "--align", "viterbi"],
                           capture_output=True, text=True, timeout=300)
    finally:
        os.remove(p.replace(".wav", ".txt"))
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "a.lab").read().split("\n")
    assert [ln.split()[2] for ln in lines if ln and ln.split()[2] not in ("SP", "AP")] == ["p00", "p01", "p02"]


def test_wavlm_ragged_clips(tmp_path):
    lab = _setup(tmp_path, tiny_wavlm_config(False), 43)
    paths, trs = [], []
    for i, sec in enumerate((2.3, 3.7, 1.1)):
        p = str(tmp_path / "wavs" / f"w{i}.wav")
        A.write_wav(p, synth.make_clip(900 + i, int(16000 * sec), seed=43) * 0.8, 16000)
        tr = ["p00", "p01", "p02", "p03", "p01"][:2 + i]
        _write_tr(p, tr)
        paths.append(p)
        trs.append(tr)
    got = lab.label_files(paths, confidence_threshold=0.0, align="viterbi")
    for segs, tr, sec in zip(got, trs, (2.3, 3.7, 1.1)):
        _check_segments(_core(segs), tr, sec)
    alone = lab.label_files(paths[1:2], confidence_threshold=0.0, align="viterbi")[0]
    assert alone == got[1]
