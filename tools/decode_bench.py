#!/usr/bin/env python3
"""Diagnostic (not product): the cost of `decode="viterbi"`.

  --op    one wfl_decode call (pre-pass + chain kernels) for 16 and 64 clips x 1500 frames and for one 15 000-frame clip, C = 141,
          70 phonemes (seeded random logits, resident), lambda 2, threshold 0.5: the median of --reps calls timed with device events
          (run it under `rocprofv3 --kernel-trace --stats` for the kernels alone)
  --e2e   Labeler.label_files over a folder of 30 s 16 kHz files without transcripts (BASELINE config 2 model, synthetic weights),
          decode="argmax" and decode="viterbi" alternated, --rounds times each: audio-s/s of both
  --summarise TRACE.csv   a rocprofv3 kernel trace -> the per-kernel summary (kernel, workgroups, calls, avg / min / max us) on --stats-out
The results of --op / --e2e go to --out (profiles/decode_bench.json), merged into what the file already holds."""
import argparse
import csv
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np


def _timed(fn, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms))}


def op_bench(reps):
    import torch
    import synthetic as synth
    from wfl_asr_amd import decode as DC
    rng = np.random.default_rng(0)
    C = 141
    table = DC.class_table(synth.make_labels(70))
    out = {"C": C, "phonemes": len(table.pairs), "switch_penalty": 2.0, "threshold": 0.5, "reps": reps}
    for name, nb, T in (("clips16_T1500", 16, 1500), ("clips64_T1500", 64, 1500), ("clips1_T15000", 1, 15000)):
        z = torch.from_numpy(rng.standard_normal((nb * T, C)).astype(np.float32) * 3).cuda()
        st = DC.bio_viterbi(z, [T] * nb, table, 2.0, 0.5)[2]
        assert int(st.max()) == 0
        out[name] = _timed(lambda: DC.bio_viterbi(z, [T] * nb, table, 2.0, 0.5), reps)
        out[name]["workspace_bytes"] = DC.workspace_bytes([T] * nb, len(table.pairs))
    return out


def e2e_bench(files, rounds):
    import torch
    import synthetic as synth
    from wfl_asr_amd import audio as A
    from wfl_asr_amd import infer as I
    d = tempfile.mkdtemp(prefix="wfl_decode_")
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
        folder = os.path.join(d, "plain")
        os.makedirs(folder)
        base = [synth.make_clip(5000 + i, 480000, seed=1) * 0.8 for i in range(8)]
        for i in range(files):
            A.write_wav(os.path.join(folder, f"{i:04d}.wav"), base[i % 8], 16000)
        paths = sorted(os.path.join(folder, n) for n in os.listdir(folder))
        legs = {"argmax": dict(decode="argmax"), "viterbi": dict(decode="viterbi", switch_penalty=2.0)}
        nseg = {}
        for k, kw in legs.items():                             # warm-up (allocations, kernels)
            lab.label_files(paths[:4], confidence_threshold=0.5, verbose=False, **kw)
        rates = {k: [] for k in legs}
        for _ in range(rounds):
            for k, kw in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = lab.label_files(paths, confidence_threshold=0.5, verbose=False, **kw)
                torch.cuda.synchronize()
                rates[k].append(files * 30.0 / (time.perf_counter() - t0))
                nseg[k] = float(np.mean([len(g) for g in got]))
        return {"e2e_audio_s_per_s": {k: [round(r, 1) for r in v] for k, v in rates.items()},
                "median": {k: round(float(np.median(v)), 1) for k, v in rates.items()}, "segments_per_file": nseg, "files": files,
                "note": "a folder of 30 s files without transcripts; argmax = the default free decode, viterbi = decode='viterbi', "
                        "switch_penalty 2"}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def summarise(trace, dst):
    """rocprofv3's kernel trace -> kernel, workgroups, calls, avg_us, min_us, max_us (the layout of profiles/align_kernel_stats.csv)."""
    groups = {}
    with open(trace, newline="") as f:
        for r in csv.DictReader(f):
            def prod(stem):
                if stem in r:
                    return int(r[stem])
                return int(r[stem + "_X"]) * int(r[stem + "_Y"]) * int(r[stem + "_Z"])
            wgs = prod("Grid_Size") // max(prod("Workgroup_Size"), 1)
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            groups.setdefault((r["Kernel_Name"], wgs), []).append(us)
    rows = sorted(groups.items(), key=lambda kv: -sum(kv[1]))
    with open(dst, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["kernel", "workgroups", "calls", "avg_us", "min_us", "max_us"])
        for (name, wgs), v in rows:
            w.writerow([name, wgs, len(v), round(float(np.mean(v)), 1), round(min(v), 1), round(max(v), 1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--summarise", metavar="TRACE.csv")
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "decode_kernel_stats.csv"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_bench.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.stats_out)
    if not (a.op or a.e2e):
        return
    import torch
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res["tool"] = "tools/decode_bench.py --op --reps 50; --e2e --files 64 --rounds 3"
    res["gpu"] = torch.cuda.get_device_name(0)
    if a.op:
        res["bio_viterbi_call_device_events"] = op_bench(a.reps)
        print(json.dumps(res["bio_viterbi_call_device_events"]))
    if a.e2e:
        res["e2e"] = e2e_bench(a.files, a.rounds)
        print(json.dumps(res["e2e"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
