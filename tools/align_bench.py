#!/usr/bin/env python3
"""Diagnostic (not product): the cost of `align="viterbi"`.

  --op    one wfl_align launch for 16 and 64 clips x 1500 frames x N = 300 tokens, C = 141 (seeded random logits, resident): the
          median of --reps launches timed with device events (run it under `rocprofv3 --kernel-trace --stats` for the kernel alone)
  --posterior   the same shape through viterbi_align and then alignment_posteriors (wfl_align_posterior), both timed in the same run;
          the ratio of the two calls.  With --check also the kernel's maximum deviations from the float64 reference on the shapes
          of tests/test_gpu_align_posterior.py, beside the float32 restatement's.  With --e2e the end-to-end rate of viterbi with
          and without align_scores.  The result goes to --out (profiles/align_posterior_bench.json)
  --windowed    the --op shape through wfl_align, through wfl_align_windowed with open windows and with windows of +-5 frames around
          the unwindowed path's starts, and the same three through the posterior entries; the ratios to the unwindowed calls.  The
          result goes to --out (profiles/align_windowed_bench.json)
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


def _timed(fn, reps):
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


def posterior_bench(reps):
    rng = np.random.default_rng(0)
    C, T, N = 141, 1500, 300
    out = {"T": T, "N": N, "C": C, "reps": reps}
    for nb in (16, 64):
        z = torch.from_numpy(rng.standard_normal((nb * T, C)).astype(np.float32) * 3).cuda()
        toks = [[[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 70, N)] for _ in range(nb)]
        gaps = [[0, 139, 140]] * nb
        args = (z, [T] * nb, toks, gaps, 0)
        tok = AL.viterbi_align(*args)[1]
        vit = _timed(lambda: AL.viterbi_align(*args), reps)
        post = _timed(lambda: AL.alignment_posteriors(*args, tok), reps)
        st = AL.alignment_posteriors(*args, tok)[4]
        assert int(st.max()) == 0
        out[f"clips{nb}"] = {"viterbi_align": vit, "alignment_posteriors": post,
                             "ratio_posterior_to_viterbi": post["ms_median"] / vit["ms_median"],
                             "workspace_bytes": AL.posterior_workspace_bytes([T] * nb, [N] * nb)}
    return out


def windowed_bench(reps, shapes=((1500, 300, (16, 64)),)):
    """shapes: (T, N, clip counts); the first is the --op shape, whose results stay at the top level of the result."""
    out = {}
    for T, N, counts in shapes:
        res = _windowed_shape(reps, T, N, counts)
        if not out:
            out = res
        else:
            out.setdefault("other_configurations", {})[f"T{T}_N{N}"] = res
    return out


def _windowed_shape(reps, T, N, counts):
    rng = np.random.default_rng(0)
    C = 141
    out = {"T": T, "N": N, "C": C, "reps": reps}
    for nb in counts:
        z = torch.from_numpy(rng.standard_normal((nb * T, C)).astype(np.float32) * 3).cuda()
        toks = [[[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 70, N)] for _ in range(nb)]
        gaps = [[0, 139, 140]] * nb
        args = (z, [T] * nb, toks, gaps, 0)
        tok = AL.viterbi_align(*args)[1]
        h = tok.cpu().numpy().reshape(nb, T)
        near = []                                     # +-5 frames around every token's start on the unwindowed path
        for b in range(nb):
            opens = np.nonzero((h[b] >= 0) & (np.concatenate([[-1], h[b][:-1]]) != h[b]))[0]
            assert len(opens) == N
            near.append([(int(t) - 5, int(t) + 5) for t in opens])
        packs = {"unwindowed": AL.pack_clips(*args[:4]), "open_windows": AL.pack_clips(*args[:4], windows=[None] * nb),
                 "windows_pm5": AL.pack_clips(*args[:4], windows=near)}
        res = {}
        for name, pk in packs.items():
            st = AL.viterbi_align(*args, packed=pk)[3]
            pst = AL.alignment_posteriors(*args, tok, packed=pk)[4]
            assert int(st.max()) == 0 and int(pst.max()) == 0
            res[name] = {"viterbi_align": _timed(lambda: AL.viterbi_align(*args, packed=pk), reps),
                         "alignment_posteriors": _timed(lambda: AL.alignment_posteriors(*args, tok, packed=pk), reps)}
        for name in ("open_windows", "windows_pm5"):
            for call in ("viterbi_align", "alignment_posteriors"):
                res[name][call]["ratio_to_unwindowed"] = res[name][call]["ms_median"] / res["unwindowed"][call]["ms_median"]
        out[f"clips{nb}"] = res
    return out


def posterior_check():
    """The kernel's and the float32 restatement's maximum deviations from float64 on the operator test's own clips (its builders)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_align_posterior as tp
    out = {}
    for name, clips, scattered in [("ragged", tp.ragged_clips(), True), ("multi_wave_2500_1000", tp.multi_wave_clips(2500, 1000), False),
                                   ("multi_wave_4400_4096", tp.multi_wave_clips(4400, 4096), False), ("cap_15000_4096", tp.cap_clips(), False),
                                   ("T_equals_N", tp.t_equals_n_clips(), False), ("batch_of_16", tp.batch16_clips(), False)]:
        out[name] = tp._check_case(name, clips, tp._run(clips, scattered=scattered))
    return out


def e2e_bench(files, rounds, scores=False):
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
        legs = {"greedy": ("greedy", "greedy", None), "viterbi": ("viterbi", "viterbi", None)}
        if scores:
            legs["viterbi_scores"] = ("viterbi", "viterbi", True)
        for folder, mode, sc in legs.values():                 # warm-up (allocations, kernels)
            lab.label_files(lists[folder][:4], confidence_threshold=0.5, verbose=False, align=mode, align_scores=sc)
        rates = {k: [] for k in legs}
        for _ in range(rounds):
            for k, (folder, mode, sc) in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lab.label_files(lists[folder], confidence_threshold=0.5, verbose=False, align=mode, align_scores=sc)
                torch.cuda.synchronize()
                rates[k].append(files * 30.0 / (time.perf_counter() - t0))
        res = {"e2e_audio_s_per_s": {k: [round(r, 1) for r in v] for k, v in rates.items()},
               "median": {k: round(float(np.median(v)), 1) for k, v in rates.items()}, "files": files,
               "note": "greedy = the folder without transcripts, viterbi = the same files with a 300-token transcript each"
                       + (", viterbi_scores = viterbi with align_scores" if scores else "")}
        print(json.dumps(res))
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--posterior", action="store_true")
    ap.add_argument("--windowed", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None, help="default: profiles/align_posterior_bench.json (--posterior), "
                                                 "profiles/align_windowed_bench.json (--windowed)")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.op:
        op_bench(a.reps)
    if a.windowed:
        res = {"tool": "tools/align_bench.py " + " ".join(sys.argv[1:]), "gpu": torch.cuda.get_device_name(0),
               # beside the --op shape (N = 300: 256 threads x 2 slots), the two posterior configurations whose windowed form costs
               # registers: 256 x 4 (N = 600) and 512 x 9 (N = 2100)
               "calls_device_events": windowed_bench(a.reps, ((1500, 300, (16, 64)), (1500, 600, (16,)), (3000, 2100, (16,))))}
        out = a.out or os.path.join(ROOT, "profiles", "align_windowed_bench.json")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res["calls_device_events"]))
    if a.posterior:
        res = {"tool": "tools/align_bench.py " + " ".join(sys.argv[1:]), "gpu": torch.cuda.get_device_name(0),
               "calls_device_events": posterior_bench(a.reps)}
        if a.check:
            res["max_deviation_from_float64"] = posterior_check()
        if a.e2e:
            res["e2e"] = e2e_bench(a.files, a.rounds, scores=True)
        out = a.out or os.path.join(ROOT, "profiles", "align_posterior_bench.json")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res["calls_device_events"]))
    elif a.e2e:
        e2e_bench(a.files, a.rounds)


if __name__ == "__main__":
    main()
