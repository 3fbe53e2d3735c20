#!/usr/bin/env python3
"""Diagnostic (not product): the cost of `align_edits`.

One wfl_align_edits call beside one wfl_align_posterior call on the same batches -- 16 and 64 clips x 1500 frames x N = 300 tokens,
C = 141 (seeded random logits, resident, the batch packed once), the shape of tools/align_bench.py -- for tables of 0, 6, 64 and 70
substitutes (70: every phoneme of that label set; 0: the sweeps and the deletion column alone): the median of --reps calls timed
with device events, the ratio to the posterior call, and the workspace of both.  With --windowed the same with windows of +-5 frames
around the unwindowed path's starts (phase 2 skips the frames a window excludes).  The result goes to --out
(profiles/align_edits_bench.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from wfl_asr_amd import align as AL


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


def edits_bench(reps, windowed, tables=(0, 6, 64, 70), counts=(16, 64)):
    rng = np.random.default_rng(0)
    C, T, N = 141, 1500, 300
    pairs = [(2 * p - 1, 2 * p) for p in range(1, 71)]
    out = {"T": T, "N": N, "C": C, "reps": reps}
    for nb in counts:
        z = torch.from_numpy(rng.standard_normal((nb * T, C)).astype(np.float32) * 3).cuda()
        toks = [[[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 70, N)] for _ in range(nb)]
        gaps = [[0, 139, 140]] * nb
        args = (z, [T] * nb, toks, gaps, 0)
        tok = AL.viterbi_align(*args)[1]
        packs = {"unwindowed": AL.pack_clips(*args[:4])}
        if windowed:
            h = tok.cpu().numpy().reshape(nb, T)
            near = []                                     # +-5 frames around every token's start on the unwindowed path
            for b in range(nb):
                opens = np.nonzero((h[b] >= 0) & (np.concatenate([[-1], h[b][:-1]]) != h[b]))[0]
                assert len(opens) == N
                near.append([(int(t) - 5, int(t) + 5) for t in opens])
            packs["windows_pm5"] = AL.pack_clips(*args[:4], windows=near)
        res = {}
        for name, pk in packs.items():
            assert int(AL.alignment_posteriors(*args, tok, packed=pk)[4].max()) == 0
            post = _timed(lambda: AL.alignment_posteriors(*args, tok, packed=pk), reps)
            r = {"alignment_posteriors": post, "posterior_workspace_bytes": AL.posterior_workspace_bytes([T] * nb, [N] * nb),
                 "edits_workspace_bytes": AL.edits_workspace_bytes([T] * nb, [N] * nb)}
            for P in tables:
                assert int(AL.edit_scores(*args, pairs[:P], packed=pk)[2].max()) == 0
                t = _timed(lambda: AL.edit_scores(*args, pairs[:P], packed=pk), reps)
                t["ratio_to_posterior"] = t["ms_median"] / post["ms_median"]
                r[f"edit_scores_P{P}"] = t
            res[name] = r
        out[f"clips{nb}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windowed", action="store_true")
    ap.add_argument("--out", default=None, help="default: profiles/align_edits_bench.json")
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    res = {"tool": "tools/align_edits_bench.py " + " ".join(sys.argv[1:]), "gpu": torch.cuda.get_device_name(0),
           "calls_device_events": edits_bench(a.reps, a.windowed)}
    out = a.out or os.path.join(ROOT, "profiles", "align_edits_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["calls_device_events"]))


if __name__ == "__main__":
    main()
