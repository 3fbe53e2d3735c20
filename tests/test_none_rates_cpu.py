"""CPU: `encoder_type: none` at any sample rate and frame duration (/root/reference/model.py:85-90 builds the MelSpectrogram from
data.sample_rate with hop_length = int(frame_duration * sample_rate)).  Config resolution, and the C-ABI geometry through the ctypes
binding (wfl_create runs without a GPU)."""
import ctypes

import pytest

from wfl_asr_amd import _lib
import synthetic as synth
from wfl_asr_amd.archs import resolve_encoder_arch
from wfl_asr_amd.tagger import BIOPhonemeTagger


def _cfg(sample_rate, frame_duration, n_mels=80, **kw):
    cfg = synth.base_config("none", **kw)
    cfg["data"].update(sample_rate=sample_rate, frame_duration=frame_duration, n_mels=n_mels)
    return cfg


@pytest.mark.parametrize("sr,frame,hop", [(44100, 0.02, 882), (44100, 0.01, 441), (22050, 0.01, 220), (24000, 0.02, 480),
                                          (8000, 0.01, 80), (16000, 0.005, 80)])
def test_hop_follows_rate_and_frame_duration(sr, frame, hop):
    cfg = _cfg(sr, frame)
    enc, arch = resolve_encoder_arch(cfg["model"], cfg["data"], any_rate=True)
    assert enc == "none" and arch.hop == hop == int(frame * sr) and arch.sample_rate == sr and arch.n_fft == 400
    if sr != 16000:
        with pytest.raises(ValueError, match="16 kHz"):                     # (without any_rate: the original 16 kHz contract)
            resolve_encoder_arch(cfg["model"], cfg["data"])


def test_hop_zero_is_refused():
    cfg = _cfg(16000, 0.00001)
    with pytest.raises(ValueError, match="frame_duration"):
        resolve_encoder_arch(cfg["model"], cfg["data"], any_rate=True)
    cfg["data"]["sample_rate"] = 0
    with pytest.raises(ValueError, match="sample_rate"):
        resolve_encoder_arch(cfg["model"], cfg["data"], any_rate=True)


def _none_arch(hop, sr, n_mels=80):
    a = _lib.WflArch()
    a.abi_version = _lib.ABI_VERSION
    a.encoder_type = 2
    a.d_model = a.n_mels = n_mels
    a.num_classes, a.o_id = 5, 4
    a.mel_hop, a.mel_sample_rate = hop, sr
    return a


def test_create_at_44k_through_the_binding():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.WflArch) == 256
    assert _lib.WflArch.mel_sample_rate.offset == 256 - 6 * 4          # (taken from the reserved words: ABI 2 unchanged)
    h = ctypes.c_void_p(0)
    assert lib.wfl_create(ctypes.byref(_none_arch(882, 44100)), ctypes.byref(h)) == 0 and h.value, lib.wfl_last_error()
    try:
        for L in (201, 882, 883, 44100 * 7 + 13, 1323000):
            assert lib.wfl_num_frames(h, L) == 1 + L // 882
        assert lib.wfl_num_frames(h, 1323000) == 1501
        for L in (0, 1, 200):
            assert lib.wfl_num_frames(h, L) == 0
        assert lib.wfl_workspace_bytes(h, 4, 1323000) > 0
    finally:
        lib.wfl_destroy(h)


def test_create_validates_hop_and_rate():
    lib = _lib.load()
    h = ctypes.c_void_p(0)
    for hop, sr in ((80, 8000), (1, 16000), (200, 16000), (4800, 192000), (220, 22050), (441, 11025), (160, 0), (320, 0)):
        assert lib.wfl_create(ctypes.byref(_none_arch(hop, sr)), ctypes.byref(h)) == 0, (hop, sr, lib.wfl_last_error())
        lib.wfl_destroy(h)
    assert lib.wfl_create(ctypes.byref(_none_arch(0, 16000)), ctypes.byref(h)) != 0
    assert b"mel_hop" in lib.wfl_last_error()
    for hop in (200, 80, 882):                                              # no rate named: 16 kHz, hop 160 / 320, as before the field
        assert lib.wfl_create(ctypes.byref(_none_arch(hop, 0)), ctypes.byref(h)) != 0
        assert b"hop 160 and 320" in lib.wfl_last_error()
    for sr in (7999, 192001, -16000):
        assert lib.wfl_create(ctypes.byref(_none_arch(320, sr)), ctypes.byref(h)) != 0
        assert b"mel_sample_rate" in lib.wfl_last_error()


def test_tagger_carries_the_rate():
    labels = synth.make_labels(3)
    m = BIOPhonemeTagger(_cfg(44100, 0.02), labels, any_rate=True)
    assert m.num_frames(1323000) == 1501 and m.num_frames(200) == 0
    m = BIOPhonemeTagger(_cfg(16000, 0.005), labels, any_rate=True)
    assert m.num_frames(16000 * 3 + 7) == 1 + (16000 * 3 + 7) // 80
    with pytest.raises(_lib.WflError, match="hop 160 and 320"):
        BIOPhonemeTagger(_cfg(16000, 0.005), labels)                        # (without any_rate: the original contract)
