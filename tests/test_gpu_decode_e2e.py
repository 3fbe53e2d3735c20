"""-m gpu: `decode="viterbi"` end to end on synthetic tiny checkpoints (Whisper geometry of 30 s windows, and WavLM with ragged
clips): legal tag strings, the same segments as the numpy float64 recurrence over the forward's own logits, one search across a long
file's chunks with seam-crossing runs as single segments, the greedy transcript match over the new segments, the median-filter
notice, the fallback and the CLI flags; `decode="argmax"` and no option at all stay what they were."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import bio_viterbi_ref as R
import synthetic as synth
from cases import tiny_wavlm_config, tiny_whisper_config
from wfl_asr_amd import audio as A
from wfl_asr_amd import decode as DC
from wfl_asr_amd import infer as I
from wfl_asr_amd import native_post as npost
from wfl_asr_amd import postprocess as pp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = sorted(["O"] + [f"{t}-{p}" for p in ("p00", "p01", "p02", "p03", "SP", "AP") for t in ("B", "I")])
NOTICE = "median_filter is not applied"


def _setup(d, cfg, seed, merge="none"):
    cfg["output"]["save_dir"] = str(d / "save")
    cfg["postprocess"] = {"median_filter": 3, "merge_segments": merge, "confidence_threshold": 0.3}
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
    d = tmp_path_factory.mktemp("vd")
    cfg = tiny_whisper_config(enable_bilstm=False)
    cfg["model"]["encoder_arch"]["max_positions"] = 1500
    lab = _setup(d, cfg, 41)
    A.write_wav(str(d / "wavs" / "a.wav"), synth.make_clip(800, 16000 * 7, seed=41) * 0.9, 16000)
    A.write_wav(str(d / "wavs" / "long.wav"), synth.make_clip(801, 16000 * 65, seed=41) * 0.8, 16000)
    A.write_wav(str(d / "wavs" / "plain.wav"), synth.make_clip(802, 16000 * 4, seed=41) * 0.7, 16000)
    return d, lab


def _file_logits(lab, path, threshold):
    """The file's chunks through model.label(want_logits=True), one chunk per forward -> (z [frames, C] float64-able numpy of the valid
    frames, frames per chunk, offsets per chunk, clock per chunk)."""
    chunks = lab._load_chunks(path)
    zs, cf, co, cc, clock = [], [], [], [], 0.0
    for c in chunks:
        x = np.zeros((lab.batch_size, lab.chunk_samples), np.float32)
        x[0, :len(c)] = c
        lens = np.zeros(lab.batch_size, np.int32)
        lens[0] = len(c)
        res = lab.model.label(torch.from_numpy(x).cuda(), None, threshold=threshold, lens=lens, average_languages=True, want_logits=True)
        tv = lab._valid_frames(len(c), res.ids.shape[1])
        zs.append(res.logits[0, :tv].cpu().numpy())
        cf.append(tv)
        co.append(res.offsets[0, :tv].cpu().numpy())
        cc.append(clock)
        clock += len(c) / lab.sr
    return np.concatenate(zs), cf, co, cc


def _host_segments(lab, ids, cf, co, cc):
    s, e, ph = DC.path_segments_free(ids, cf, co, cc, lab._table, pp.FRAME_DURATION)
    remap, names = lab._names_for(None)
    ph = remap[ph] if ph.size else ph
    mode = lab.config["postprocess"]["merge_segments"]
    if mode != "none" and s.size:
        s, e, ph = npost.merge_segments(s, e, ph, mode)
    return npost.to_tuples(s, e, ph, names)


def _lab_bytes(segs):
    return npost.format_lab_tuples(segs)


def test_argmax_and_no_option_are_the_same_lab_bytes(whisper, capsys):
    d, lab = whisper
    paths = [str(d / "wavs" / n) for n in ("a.wav", "long.wav", "plain.wav")]
    plain = lab.label_files(paths, confidence_threshold=0.3)
    out = capsys.readouterr().out
    explicit = lab.label_files(paths, confidence_threshold=0.3, decode="argmax", switch_penalty=3.0)
    assert [_lab_bytes(s) for s in plain] == [_lab_bytes(s) for s in explicit]
    assert NOTICE not in out and all(len(s) for s in plain)


@pytest.mark.parametrize("lam", [0.0, 2.0])
def test_viterbi_is_legal_and_equals_the_host_recurrence(whisper, lam):
    d, lab = whisper
    table = DC.class_table(LABELS)
    paths = [str(d / "wavs" / n) for n in ("a.wav", "plain.wav", "long.wav")]
    got = lab.label_files(paths, confidence_threshold=0.0, decode="viterbi", switch_penalty=lam)
    for p, segs in zip(paths, got):
        z, cf, co, cc = _file_logits(lab, p, 0.0)
        ref, _ = R.viterbi(z, table, lam)
        ids, _, st = DC.bio_viterbi(torch.from_numpy(z).cuda(), [len(z)], table, lam, 0.0)
        ids = ids.cpu().numpy()
        assert st.cpu().tolist() == [0] and R.legal(ids, table)
        assert (ids == ref).all()
        assert segs == _host_segments(lab, ref, cf, co, cc)
        assert len(segs) == int((lab._table.kind[ref] == 1).sum())        # merge_segments none: one segment per opened phoneme run
        for j in range(len(segs) - 1):
            assert segs[j][0] <= segs[j][1] <= segs[j + 1][0] + 1e-9
    # with the confidence threshold of the config: still a legal tag string behind every file
    for p in paths:
        z, cf, _, _ = _file_logits(lab, p, 0.3)
        ids, _, st = DC.bio_viterbi(torch.from_numpy(z).cuda(), [len(z)], table, lam, 0.3)
        assert st.cpu().tolist() == [0] and R.legal(ids.cpu().numpy(), table)


def test_a_run_across_a_chunk_seam_is_one_segment(whisper):
    d, lab = whisper
    table = DC.class_table(LABELS)
    p = str(d / "wavs" / "long.wav")
    z, cf, co, cc = _file_logits(lab, p, 0.0)
    assert cf[:2] == [1500, 1500] and len(cf) == 3
    kind = lab._table.kind
    lam = None
    for cand in (2.0, 1.0, 4.0, 0.5, 8.0, 0.0):
        ref, _ = R.viterbi(z, table, cand)
        if any(kind[ref[s]] == 2 for s in (1500, 3000)):      # I-p opens a chunk: legal only as the continuation of the run before
            lam = cand
            break
    assert lam is not None, "no run crosses a seam at any of the penalties tried (test setup)"
    seams = [30.0 * (i + 1) for i, s in enumerate((1500, 3000)) if kind[ref[s]] == 2]
    got = lab.label_files([p], confidence_threshold=0.0, decode="viterbi", switch_penalty=lam)[0]
    assert len(got) == int((kind[ref] == 1).sum())            # a seam that cut a run in two would add a segment
    for t in seams:
        assert sum(1 for a, b, _ in got if a < t < b) == 1


def test_a_transcript_under_align_greedy_is_matched_over_the_new_segments(whisper):
    d, lab = whisper
    p = str(d / "wavs" / "a.wav")
    free = lab.label_files([p], confidence_threshold=0.3, decode="viterbi", switch_penalty=2.0)[0]
    names = [s[2] for s in free if s[2] not in ("SP", "AP")]
    assert len(names) >= 3, "the decode has too few segments (test setup)"
    tr = names[1:-1:2] or names[:1]
    with open(p.replace(".wav", ".txt"), "w") as f:
        f.write(" ".join(tr))
    try:
        got = lab.label_files([p], confidence_threshold=0.3, align="greedy", decode="viterbi", switch_penalty=2.0, verbose=False)[0]
        argmax = lab.label_files([p], confidence_threshold=0.3, align="greedy", verbose=False)[0]
        want = pp.align_phoneme_list(free, tr)
        assert [s for s in got if s[2] not in ("SP", "AP")] == [s for s in want if s[2] not in ("SP", "AP")]
        assert got == lab._match_forced(p, free, False)
        assert [s[2] for s in got if s[2] not in ("SP", "AP")] == tr
        assert got != argmax                                   # (the segments under the match are the new ones)
    finally:
        os.remove(p.replace(".wav", ".txt"))


def test_median_filter_prints_the_notice_and_changes_nothing_else(whisper, capsys):
    d, lab = whisper
    paths = [str(d / "wavs" / n) for n in ("a.wav", "plain.wav")]
    capsys.readouterr()
    with_mf = lab.label_files(paths, confidence_threshold=0.3, decode="viterbi", switch_penalty=1.0)
    out = capsys.readouterr().out
    assert out.count(NOTICE) == 1
    lab.config["postprocess"]["median_filter"] = 1
    try:
        without = lab.label_files(paths, confidence_threshold=0.3, decode="viterbi", switch_penalty=1.0)
        assert NOTICE not in capsys.readouterr().out
    finally:
        lab.config["postprocess"]["median_filter"] = 3
    assert with_mf == without


def test_config_keys_select_the_decode(whisper):
    d, lab = whisper
    p = str(d / "wavs" / "plain.wav")
    want = lab.label_files([p], confidence_threshold=0.3, decode="viterbi", switch_penalty=2.0)
    lab.config["postprocess"].update(decode="viterbi", switch_penalty=2.0)
    try:
        assert lab.label_files([p], confidence_threshold=0.3) == want
        assert lab.label_files([p], confidence_threshold=0.3, decode="argmax") != want
    finally:
        del lab.config["postprocess"]["decode"], lab.config["postprocess"]["switch_penalty"]


def test_a_non_zero_status_falls_back_to_argmax_with_a_message(whisper, capsys):
    """A stub class table that uses one class twice makes wfl_decode report status 4 for every clip: no fault is provoked."""
    d, lab = whisper
    paths = [str(d / "wavs" / n) for n in ("a.wav", "plain.wav")]
    argmax = lab.label_files(paths, confidence_threshold=0.3)
    capsys.readouterr()
    lab._decode_table = (LABELS.index("O"), [(0, 1), (0, 1)])
    try:
        got = lab.label_files(paths, confidence_threshold=0.3, decode="viterbi", switch_penalty=2.0)
    finally:
        lab._decode_table = None
    out = capsys.readouterr().out
    assert out.count("viterbi decode not possible (wfl_decode status 4); using the argmax decode") == 2
    assert got == argmax


def test_cli_flags_reach_the_labeler(whisper, tmp_path):
    d, lab = whisper
    p = str(d / "wavs" / "a.wav")
    want = lab.label_files([p], confidence_threshold=0.3, decode="viterbi", switch_penalty=2.5)[0]
    plain = lab.label_files([p], confidence_threshold=0.3)[0]
    assert _lab_bytes(want) != _lab_bytes(plain)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), p, "-ckpt", str(d / "best_model.pt"), "-c",
                        str(d / "config.yaml"), "-o", str(tmp_path / "a.lab"), "--decode", "viterbi", "--switch-penalty", "2.5"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert NOTICE in r.stdout
    assert open(tmp_path / "a.lab", "rb").read() == _lab_bytes(want)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), p, "-ckpt", str(d / "best_model.pt"), "-c",
                        str(d / "config.yaml"), "-o", str(tmp_path / "b.lab"), "-dec", "argmax"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "b.lab", "rb").read() == _lab_bytes(plain)


def test_wavlm_ragged_clips(tmp_path):
    lab = _setup(tmp_path, tiny_wavlm_config(False), 43, merge="right")
    paths = []
    for i, sec in enumerate((2.3, 3.7, 1.1)):
        p = str(tmp_path / "wavs" / f"w{i}.wav")
        A.write_wav(p, synth.make_clip(900 + i, int(16000 * sec), seed=43) * 0.8, 16000)
        paths.append(p)
    got = lab.label_files(paths, confidence_threshold=0.0, decode="viterbi", switch_penalty=1.0)
    assert all(len(s) for s in got)
    for segs, sec in zip(got, (2.3, 3.7, 1.1)):
        for j, (a, b, _) in enumerate(segs):
            assert 0.0 <= a <= b <= sec + 0.05
            if j:
                assert segs[j - 1][1] <= a + 1e-9
    alone = lab.label_files(paths[1:2], confidence_threshold=0.0, decode="viterbi", switch_penalty=1.0)[0]
    assert alone == got[1]
