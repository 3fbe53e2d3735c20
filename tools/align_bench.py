#!/usr/bin/env python3
"""Diagnostic (not product): the cost of `align="viterbi"`.

  --op    one wfl_align launch for 16 and 64 clips x 1500 frames x N = 300 tokens, C = 141 (seeded random logits, resident): the
          median of --reps launches timed with device events (run it under `rocprofv3 --kernel-trace --stats` for the kernel alone)
  --e2e   Labeler.label_files over a folder of 30 s 16 kHz files (BASELINE config 2 model, synthetic weights), the same files with
          a transcript each (align="viterbi") and without one, alternated, --rounds times each; prints audio-s/s of both"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import yaml

import synthetic as synth
from wfl_asr_amd import align as AL
from wfl_asr_amd import audio as A
from wfl_asr_amd import infer as I


def op_bench(reps):
    rng = np.random.default_rng(0)
    C, T, N = 141, 1500, 300
    out = {}
    for nb in (16, 64):
        z = torch.from_numpy(rng.standard_normal((nb * T, C)).astype(np.float32) * 3).cuda()
        toks = [[[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 70, N)] for _ in range(nb)]
        gaps = [[0, 139, 140]] * nb
        for _ in range(3):
            AL.viterbi_align(z, [T] * nb, toks, gaps, 0)
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ids, tok, score, st = AL.viterbi_align(z, [T] * nb, toks, gaps, 0)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        assert int(st.max()) == 0
        out[f"clips{nb}_ms_median"] = float(np.median(ms))
        out[f"clips{nb}_ms_min"] = float(np.min(ms))
    print(json.dumps({"align_launch": out, "T": T, "N": N, "C": C, "reps": reps}))


def e2e_bench(files, rounds):
    d = tempfile.mkdtemp(prefix="wfl_align_")
    try:
        cfg = synth.baseline_config(1)
        cfg["output"] = {"save_dir": os.path.join(d, "save")}
        cfg["postprocess"] = {"median_filter": 3, "merge_segments": "right", "confidence_threshold": 0.5}
        cfg.setdefault("data", {})["sample_rate"] = 16000
        os.makedirs(cfg["output"]["save_dir"])
        labels = synth.make_labels(70)
        with open(os.path.join(cfg["output"]["save_dir"], "phonemes.txt"), "w") as f:
            f.write("\n".join(labels) + "\n")
        sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, len(labels), seed=1, cls_gain=6.0).items()}
        lab = I.Labeler(cfg, sd)
        plain, withtr = os.path.join(d, "plain"), os.path.join(d, "tr")
        os.makedirs(plain)
        os.makedirs(withtr)
        rng = np.random.default_rng(1)
        base = [synth.make_clip(5000 + i, 480000, seed=1) * 0.8 for i in range(8)]
        phs = sorted({t[2:] for t in labels if t != "O"})
        for i in range(files):
            for folder in (plain, withtr):
                A.write_wav(os.path.join(folder, f"{i:04d}.wav"), base[i % 8], 16000)
            with open(os.path.join(withtr, f"{i:04d}.txt"), "w") as f:
                f.write(" ".join(rng.choice(phs, size=300)))
        lists = {k: sorted(os.path.join(f, n) for n in os.listdir(f) if n.endswith(".wav")) for k, f in (("greedy", plain),
                                                                                                      ("viterbi", withtr))}
        for k in lists:                                        # warm-up (allocations, kernels)
            lab.label_files(lists[k][:4], confidence_threshold=0.5, verbose=False, align=k)
        rates = {"greedy": [], "viterbi": []}
        for _ in range(rounds):
            for k in ("greedy", "viterbi"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lab.label_files(lists[k], confidence_threshold=0.5, verbose=False, align=k)
                torch.cuda.synchronize()
                rates[k].append(files * 30.0 / (time.perf_counter() - t0))
        print(json.dumps({"e2e_audio_s_per_s": {k: [round(r, 1) for r in v] for k, v in rates.items()},
                          "median": {k: round(float(np.median(v)), 1) for k, v in rates.items()}, "files": files,
                          "note": "greedy = the folder without transcripts, viterbi = the same files with a 300-token transcript each"}))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.op:
        op_bench(a.reps)
    if a.e2e:
        e2e_bench(a.files, a.rounds)


if __name__ == "__main__":
    main()
