#!/usr/bin/env python3
"""Diagnostic (not product): `encoder_type: none` forward steps at two front-end geometries in ONE process, so that a
`rocprofv3 --kernel-trace --stats` run lists both mel kernels side by side:
  16 clips x 30 s at 44.1 kHz, frame 0.02 s -> hop 882 (the general kernel, logmel_power_kernel<0, true>)
  16 clips x 30 s at 16 kHz,   frame 0.02 s -> hop 320 (the Toeplitz kernel, logmel_power_kernel<320, true>)
Both give 1501 frames per clip, so the head's work is the same.  Prints one JSON line per geometry: the whole forward step
(device events around `steps` back-to-back label() calls after `warmup` calls)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import synthetic as synth
from wfl_asr_amd.tagger import BIOPhonemeTagger


def step_time(sr, frame, batch, steps, warmup, headless):
    cfg = synth.base_config("none")
    cfg["data"].update(sample_rate=sr, frame_duration=frame, n_mels=80)
    if headless:
        cfg["model"].update(enable_bilstm=False, num_conformer_layers=0, enable_dilated_conv=False)
    labels = synth.make_labels(40)
    m = BIOPhonemeTagger(cfg, labels, any_rate=True)
    sd_cfg = dict(cfg, data=dict(cfg["data"], sample_rate=16000, frame_duration=0.02))      # (the head checkpoint depends on n_mels alone)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(sd_cfg, len(labels), seed=7).items()})
    m.to("cuda").eval()
    L = 30 * sr
    x = torch.from_numpy(synth.make_batch(0, batch, L, sr=sr, seed=7) * 0.05).cuda()
    lang = np.zeros(batch, np.int64)
    for _ in range(warmup):
        out = m.label(x, lang, threshold=0.5)
    torch.cuda.synchronize()
    assert int(out.status.item()) == 0
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        m.label(x, lang, threshold=0.5)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / steps
    return dict(sample_rate=sr, frame_duration=frame, hop=int(frame * sr), frames=m.num_frames(L), batch=batch, head="none" if headless
                else "default", step_ms=round(ms, 4), audio_s_per_s=round(batch * 30.0 / (ms / 1e3), 1),
                mel_general=os.environ.get("WFL_MEL_GENERAL", "0"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--headless", action="store_true", help="no BiLSTM / Conformer / dilated stack: the step is the front-end + classifier")
    args = ap.parse_args()
    for sr, frame in ((44100, 0.02), (16000, 0.02)):
        print(json.dumps(step_time(sr, frame, args.batch, args.steps, args.warmup, args.headless)), flush=True)


if __name__ == "__main__":
    main()
