"""-m gpu: `postprocess.phoneme_bigram` end to end on a synthetic tiny Whisper checkpoint (30 s windows), in the manner of
tests/test_gpu_decode_e2e.py: the segments of a file decoded with a bigram file equal those the float64 recurrence
(tests/bio_bigram_ref.py) and path_segments_free give over the forward's own logits, for a short file and for one longer than 30 s;
weight 0 is the plain grammar search byte for byte; without the keys nothing changes; the fallback; the CLI flags."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import bio_bigram_ref as R
import bio_viterbi_ref as V
import synthetic as synth
from cases import tiny_whisper_config
from wfl_asr_amd import audio as A
from wfl_asr_amd import decode as DC
from wfl_asr_amd import infer as I
from wfl_asr_amd import native_post as npost
from wfl_asr_amd import phonotactics as PH
from wfl_asr_amd import postprocess as pp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHONES = ("p00", "p01", "p02", "p03", "SP", "AP")
LABELS = sorted(["O"] + [f"{t}-{p}" for p in PHONES for t in ("B", "I")])
LAM, WEIGHT = 1.0, 0.7


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp("bg")
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
    """The file's chunks through model.label(want_logits=True), one chunk per forward -> (z of the valid frames, frames per chunk,
    offsets per chunk, clock per chunk)."""
    chunks = lab._load_chunks(path)
    zs, cf, co, cc, clock = [], [], [], [], 0.0
    for c in chunks:
        x = np.zeros((lab.batch_size, lab.chunk_samples), np.float32)
        x[0, :len(c)] = c
        lens = np.zeros(lab.batch_size, np.int32)
        lens[0] = len(c)
        res = lab.model.label(torch.from_numpy(x).cuda(), None, threshold=0.0, lens=lens, average_languages=True, want_logits=True)
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
    return npost.to_tuples(s, e, ph, names)


def _lab_bytes(segs):
    return npost.format_lab_tuples(segs)


@pytest.fixture(scope="module")
def logits(setup):
    d, lab, _ = setup
    return {n: _file_logits(lab, str(d / "wavs" / n)) for n in ("a.wav", "long.wav")}


def test_a_bigram_file_gives_the_float64_recurrence_s_lab(setup, logits):
    d, lab, bg = setup
    table = DC.class_table(LABELS)
    W = PH.transition_table(PH.load(bg), table, LABELS, LAM, WEIGHT)
    assert np.isneginf(W).any()
    paths = [str(d / "wavs" / n) for n in ("a.wav", "long.wav")]
    got = lab.label_files(paths, decode="viterbi", switch_penalty=LAM, phoneme_bigram=bg, bigram_weight=WEIGHT)
    plain = lab.label_files(paths, decode="viterbi", switch_penalty=LAM)
    for n, segs, flat in zip(("a.wav", "long.wav"), got, plain):
        z, cf, co, cc = logits[n]
        assert (len(cf) == 3) == (n == "long.wav")
        ref, _ = R.viterbi(z, table, W.astype(np.float64))
        assert R.forbidden_successions(ref, table, W) == 0
        want = _host_segments(lab, ref, cf, co, cc)
        assert len(want) and _lab_bytes(segs) == _lab_bytes(want)
        assert _lab_bytes(segs) != _lab_bytes(flat)                 # (the prior moved something)


def test_weight_zero_is_the_plain_search_byte_for_byte(setup):
    d, lab, bg = setup
    paths = [str(d / "wavs" / n) for n in ("a.wav", "long.wav")]
    plain = lab.label_files(paths, decode="viterbi", switch_penalty=2.0)
    zero = lab.label_files(paths, decode="viterbi", switch_penalty=2.0, phoneme_bigram=bg, bigram_weight=0.0)
    assert [_lab_bytes(s) for s in zero] == [_lab_bytes(s) for s in plain] and all(len(s) for s in plain)


def test_without_the_keys_nothing_changes(setup, logits):
    d, lab, bg = setup
    p = str(d / "wavs" / "a.wav")
    z, cf, co, cc = logits["a.wav"]
    table = DC.class_table(LABELS)
    ref, _ = V.viterbi(z, table, 2.0)
    assert _lab_bytes(lab.label_files([p], decode="viterbi", switch_penalty=2.0)[0]) == _lab_bytes(_host_segments(lab, ref, cf, co, cc))
    assert lab.label_files([p]) == lab.label_files([p], decode="argmax")
    # the config keys select the bigram as the arguments do
    want = lab.label_files([p], decode="viterbi", switch_penalty=LAM, phoneme_bigram=bg, bigram_weight=WEIGHT)
    lab.config["postprocess"].update(decode="viterbi", switch_penalty=LAM, phoneme_bigram=bg, bigram_weight=WEIGHT)
    try:
        assert lab.label_files([p]) == want
        with pytest.raises(ValueError, match="decode_scores cannot be combined"):
            lab.label_files([p], decode_scores=True)
        with pytest.raises(ValueError, match="need decode='viterbi'"):
            lab.label_files([p], decode="argmax")
    finally:
        for k in ("decode", "switch_penalty", "phoneme_bigram", "bigram_weight"):
            del lab.config["postprocess"][k]


def test_a_bigram_that_does_not_fit_the_label_set_is_named(setup, tmp_path):
    d, lab, _ = setup
    p = str(d / "wavs" / "a.wav")
    f = tmp_path / "short.json"
    PH.save(PH.Bigram(["O", "p00", "xx"], np.zeros((3, 3))), str(f))
    with pytest.raises(ValueError, match="lacks phonemes of the label set: AP, SP, p01"):
        lab.label_files([p], decode="viterbi", phoneme_bigram=str(f))


def test_a_non_zero_status_falls_back_to_argmax_with_a_message(setup, capsys):
    """A stub class table that uses one class twice makes wfl_decode_bigram report status 4: no fault is provoked."""
    d, lab, bg = setup
    p = str(d / "wavs" / "a.wav")
    argmax = lab.label_files([p])
    lab.label_files([p], decode="viterbi", phoneme_bigram=bg)         # (the transition table is cached with the real class table)
    capsys.readouterr()
    lab._decode_table = (LABELS.index("O"), [(0, 1)] * 6)
    try:
        got = lab.label_files([p], decode="viterbi", phoneme_bigram=bg)
    finally:
        lab._decode_table = None
    out = capsys.readouterr().out
    assert out.count("viterbi decode not possible (wfl_decode_bigram status 4); using the argmax decode") == 1
    assert got == argmax


def test_cli_flags_reach_the_labeler(setup, tmp_path):
    d, lab, bg = setup
    p = str(d / "wavs" / "a.wav")
    want = lab.label_files([p], decode="viterbi", switch_penalty=LAM, phoneme_bigram=bg, bigram_weight=WEIGHT)[0]
    plain = lab.label_files([p], decode="viterbi", switch_penalty=LAM)[0]
    assert _lab_bytes(want) != _lab_bytes(plain)
    base = [sys.executable, os.path.join(ROOT, "infer.py"), p, "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml")]
    r = subprocess.run(base + ["-o", str(tmp_path / "a.lab"), "--decode", "viterbi", "--switch-penalty", str(LAM), "--phoneme-bigram", bg,
                               "--bigram-weight", str(WEIGHT)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "a.lab", "rb").read() == _lab_bytes(want)
    r = subprocess.run(base + ["-o", str(tmp_path / "b.lab"), "--phoneme-bigram", bg], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "need decode='viterbi'" in r.stderr and not os.path.exists(tmp_path / "b.lab")
