"""-m gpu: `encoder_type: none` at any sample rate and frame duration (/root/reference/model.py:85-90: MelSpectrogram(data.sample_rate,
n_fft=400, hop_length=int(frame_duration * sample_rate), n_mels); infer.py:218-220 resamples every file to data.sample_rate).  Hops
160 and 320 run their Toeplitz kernels, every other hop the general one (csrc/logmel.hip, HOP = 0); the mel bank spans
0 .. sample_rate // 2.  Held against the oracle's restatement of torchaudio (PARITY UNPINNED, as tests/test_gpu_none.py says)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from oracle import wfl_oracle as O
from wfl_asr_amd import audio as A
from wfl_asr_amd import infer as I
from wfl_asr_amd import postprocess as pp
import synthetic as synth
from wfl_asr_amd.archs import resolve_encoder_arch
from wfl_asr_amd.tagger import BIOPhonemeTagger

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLESS = dict(enable_bilstm=False, num_conformer_layers=0, enable_dilated_conv=False)


def _cfg(sr, frame_duration, n_mels=80, **kw):
    cfg = synth.base_config("none", **kw)
    cfg["data"].update(sample_rate=sr, frame_duration=frame_duration, n_mels=n_mels)
    return cfg


def _state_dict(cfg, n_labels, seed):
    """The synthetic head checkpoint: it depends on n_mels alone, so it is drawn from the same config at 16 kHz / 20 ms."""
    return synth.make_state_dict(dict(cfg, data=dict(cfg["data"], sample_rate=16000, frame_duration=0.02)), n_labels, seed=seed)


def _build(cfg, n_phonemes, seed):
    labels = synth.make_labels(n_phonemes)
    sd_np = _state_dict(cfg, len(labels), seed)
    m = BIOPhonemeTagger(cfg, labels, any_rate=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    m.to("cuda").eval()
    return m, labels, sd_np


@pytest.mark.parametrize("sr,frame,n_mels", [(44100, 0.02, 80), (44100, 0.01, 128), (24000, 0.02, 80), (22050, 0.01, 64),
                                             (16000, 0.005, 80), (8000, 0.02, 40)])
def test_mel_power_matches_oracle_at_any_rate(sr, frame, n_mels):
    """[B, 1 + L // hop, n_mels] fp32 mel power against torchaudio's definition, for hops above n_fft (882), below the Toeplitz
    kernels' range (80), and hop 160 at 8 kHz (the existing kernel with the 0 .. 4 kHz bank).  Empty triangles come out as 0."""
    hop = int(frame * sr)
    m, labels, _ = _build(_cfg(sr, frame, n_mels, **HEADLESS), 5, seed=81)
    fb = O.mel_filter_bank_htk(n_mels, 201, sr)
    empty = torch.from_numpy(fb.sum(0) == 0)
    for L in (sr * 3 + 123, 203):
        assert L % hop
        wav = synth.make_batch(960, 3, L, sr=sr, seed=81)
        out = m.label(torch.from_numpy(wav).cuda(), [0, 1, 0], threshold=0.5, want_hidden=True)
        ref = O.mel_spectrogram_power(torch.from_numpy(wav), sr, 400, hop, n_mels).transpose(1, 2)
        assert tuple(out.hidden.shape) == tuple(ref.shape) == (3, 1 + L // hop, n_mels) and m.num_frames(L) == 1 + L // hop
        got = out.hidden.cpu()
        assert torch.isfinite(got).all()
        err = (got - ref).abs()
        assert err.max() <= 2e-5 * ref.max(), (L, float(err.max()), float(ref.max()))
        assert (err / (ref.abs() + 1e-3 * ref.max())).max() <= 5e-4
        assert (got[:, :, empty] == 0).all()
        assert int(out.status.item()) == 0


@pytest.mark.parametrize("sr,frame", [(44100, 0.02), (16000, 0.005)])
def test_ragged_batch_equals_clips_alone(sr, frame):
    """hop 882 and 80, default head: every clip of a mixed-length batch (lens) equals the clip labelled alone, bit for bit."""
    hop = int(frame * sr)
    m, labels, _ = _build(_cfg(sr, frame), 8, seed=82)
    lens = [sr * 4 + 17, sr * 2 + 301, 5000, sr * 4 + 16, 230]
    L = max(lens)
    wav = synth.make_batch(970, len(lens), L, sr=sr, seed=82) * 0.05
    for i, n in enumerate(lens):
        wav[i, n:] = 0.0
    lang = np.array([0, 1, 1, 0, 1], np.int64)
    x = torch.from_numpy(wav).cuda()
    batch = m.label(x, lang, threshold=0.4, lens=np.array(lens, np.int32), want_logits=True, want_hidden=True)
    assert int(batch.status.item()) == 0
    for i, n in enumerate(lens):
        T = 1 + n // hop
        one = m.label(x[i:i + 1, :n].contiguous(), lang[i:i + 1], threshold=0.4, want_logits=True, want_hidden=True)
        assert one.hidden.shape[1] == T and int(one.status.item()) == 0
        assert torch.equal(batch.hidden[i, :T], one.hidden[0]), i
        assert torch.equal(batch.logits[i, :T], one.logits[0]), i
        assert torch.equal(batch.ids[i, :T], one.ids[0]), i
        assert (batch.hidden[i, T:] == 0).all()


_CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_none_rates as t
out = {{}}
for frame in (0.01, 0.02):
    m, _, _ = t._build(t._cfg(16000, frame, **t.HEADLESS), 5, seed=83)
    wav = torch.from_numpy(t.synth.make_batch(980, 3, 16000 * 5 + 77, seed=83)).cuda()
    lens = np.array([16000 * 5 + 77, 16000 * 3 + 5, 1111], np.int32)
    out[f"plain{{frame}}"] = m.label(wav, [0, 1, 0], threshold=0.5, want_hidden=True).hidden.cpu().numpy()
    out[f"ragged{{frame}}"] = m.label(wav, [0, 1, 0], threshold=0.5, lens=lens, want_hidden=True).hidden.cpu().numpy()
np.savez({path!r}, **out)
"""


def test_general_kernel_equals_the_specialised_ones(tmp_path):
    """WFL_MEL_GENERAL=1 (read once per process) runs the general kernel at hop 160 and 320: the same sums in the same order as the
    Toeplitz instantiations, so the mel power is bit-identical, plain and ragged."""
    res = {}
    for flag in ("0", "1"):
        path = str(tmp_path / f"mel{flag}.npz")
        env = dict(os.environ, WFL_MEL_GENERAL=flag)
        code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-4000:]
        res[flag] = dict(np.load(path))
    assert sorted(res["0"]) == sorted(res["1"]) and len(res["0"]) == 4
    for k in res["0"]:
        assert np.array_equal(res["0"][k], res["1"][k]), k
        assert res["0"][k].any()


def test_full_head_at_44k_vs_oracle():
    """The reference's default head behind the 44.1 kHz / 20 ms front-end (hop 882), bounds of test_full_head_at_mel_width_vs_oracle."""
    cfg = _cfg(44100, 0.02)
    m, labels, sd_np = _build(cfg, 20, seed=84)
    L = 44100 * 9 + 77
    wav = synth.make_batch(990, 3, L, sr=44100, seed=84) * 0.05
    lang = np.array([1, 0, 1], np.int64)
    out = m.label(torch.from_numpy(wav).cuda(), lang, threshold=0.4, want_logits=True)
    enc, arch = resolve_encoder_arch(cfg["model"], cfg["data"], any_rate=True)
    assert enc == "none" and arch.hop == 882 and arch.sample_rate == 44100
    lg, of = O.forward(torch.from_numpy(wav), torch.from_numpy(lang), O.to_torch_state_dict(sd_np), enc, arch,
                       synth.head_config(cfg["model"]))
    assert tuple(out.logits.shape) == tuple(lg.shape) == (3, 1 + L // 882, len(labels))
    ids, maxp, arg, margin = O.tags_from_logits(lg, m.label2id["O"], 0.4)
    err = (out.logits.cpu() - lg).abs()
    scale = float(lg.std())
    assert err.max() <= 0.06 * scale and err.mean() <= 0.010 * scale
    assert (out.offsets.cpu() - of).abs().max() <= 0.03
    safe = (margin > 0.06 * scale) & ((maxp - 0.4).abs() > 0.06)
    assert float(safe.float().mean()) > 0.6
    assert torch.equal(out.ids.cpu()[safe].long(), ids[safe])
    assert int(out.status.item()) == 0
    m.check(3, L)


def _manual(lab, path, lang_id, thr):
    """The reference's loop at the Labeler's rate, one label() call per 30 s chunk of the native host loader (infer.py:237-325)."""
    out, clock = [], 0.0
    for c in A.load_items(path, lab.sr):
        res = lab.model.label(torch.from_numpy(np.ascontiguousarray(c))[None].cuda(), [lang_id], threshold=thr)
        ids = pp.median_filter_ids(res.ids[0].cpu().numpy(), int(lab.config["postprocess"]["median_filter"]))
        segs = pp.decode_bio_tags([lab.model.id2label[int(i)] for i in ids], offsets=res.offsets[0].cpu().numpy())
        out.extend((s + clock, e + clock, ph) for s, e, ph in segs)
        clock += len(c) / lab.sr
    return pp.merge_adjacent_segments(out, "right")


def test_labeler_at_44k(tmp_path, monkeypatch):
    """A `none` model trained at 44.1 kHz labels a folder of 44.1 kHz and 16 kHz files and a 75 s file (three 30 s chunks of 1 323 000
    samples): the same .lab with and without the GPU ingest switch, every chunk's tags equal label() on the host loader's chunk
    bit for bit, 1 + len // 882 frames per chunk.  Whisper and WavLM configs at 44.1 kHz are still refused."""
    d = tmp_path
    cfg = _cfg(44100, 0.02)
    cfg["output"]["save_dir"] = str(d / "save")
    cfg["postprocess"] = {"median_filter": 3, "merge_segments": "right", "confidence_threshold": 0.3}
    os.makedirs(cfg["output"]["save_dir"])
    labels = synth.make_labels(6)
    with open(d / "save" / "phonemes.txt", "w") as f:
        f.write("\n".join(labels) + "\n")
    with open(d / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    torch.save({k: torch.from_numpy(v) for k, v in _state_dict(cfg, len(labels), 85).items()}, d / "best_model.pt")
    os.makedirs(d / "wavs")
    files = {}
    for i, secs in enumerate((5, 3, 7)):
        files[f"hi{i}"] = 44100
        A.write_wav(str(d / "wavs" / f"hi{i}.wav"), synth.make_clip(1000 + i, 44100 * secs, sr=44100, seed=85) * 0.7, 44100)
    for i, secs in enumerate((4, 6)):
        files[f"lo{i}"] = 16000
        A.write_wav(str(d / "wavs" / f"lo{i}.wav"), synth.make_clip(1010 + i, 16000 * secs, seed=85) * 0.7, 16000)
    files["long"] = 44100
    A.write_wav(str(d / "wavs" / "long.wav"), synth.make_clip(1020, 44100 * 75, sr=44100, seed=85) * 0.7, 44100)
    cp, ck = str(d / "config.yaml"), str(d / "best_model.pt")
    texts = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("WFL_GPU_INGEST", flag)
        I.infer_folder(str(d / "wavs"), cp, ck, output_dir=str(d / f"labs{flag}"), device="cuda", lang_id=1, confidence_threshold=0.3)
        texts[flag] = {n: open(d / f"labs{flag}" / f"{n}.lab").read() for n in files}
    assert texts["1"] == texts["0"]
    lab = I._labeler(cp, ck, "cuda")
    assert lab.sr == 44100 and lab.chunk_samples == 1323000
    for n in files:
        segs = _manual(lab, str(d / "wavs" / f"{n}.wav"), 1, 0.3)
        assert texts["0"][n] == "".join(f"{int(s * 1e7)} {int(e * 1e7)} {ph}\n" for s, e, ph in segs), n
        assert segs, n
    for n, rate in files.items():
        if rate != 44100:
            continue
        path = str(d / "wavs" / f"{n}.wav")
        host = A.chunk_clip(A.load_clip(path, 44100), 44100)
        items = A.load_items(path, 44100)                      # what label_files forwards
        assert len(items) == len(host) == (3 if n == "long" else 1)
        got = lab._forward_items(items, 1, 0.3)
        for c, it, (ids, offs) in zip(host, items, got):
            assert np.array_equal(it, c) and len(ids) == 1 + len(c) // 882
            ref = lab.model.label(torch.from_numpy(np.ascontiguousarray(c))[None].cuda(), [1], threshold=0.3)
            assert np.array_equal(ids, ref.ids[0].cpu().numpy()), n
            assert np.array_equal(offs, ref.offsets[0].cpu().numpy()), n
    for enc in ("whisper", "wavlm"):
        other = synth.base_config(enc)
        other["data"]["sample_rate"] = 44100
        with pytest.raises(ValueError, match="16 kHz"):
            I.Labeler(other, {}, device="cuda")
