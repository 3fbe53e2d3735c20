#!/usr/bin/env python3
"""Diagnostic (not product): what the minimum-duration chain costs the alignment kernel.

One wfl_align call (the yardstick) beside wfl_align_min_duration calls with every D_k = 1, 3 and 5, and with D_k = 8 for every second
token (1 for the others), on the same batches -- 16 and 64 clips x 1500 frames x N = 300 tokens, C = 141 (seeded random logits,
resident, each batch packed once), the shapes of tools/align_bench.py --op.  (Every D_k = 8 would need 2400 frames: at this shape it
has no path, and a clip without a path skips its backtrace.  5 is the deepest duration all 300 tokens can have in 1500 frames.)
The calls alternate inside one process, --rounds times, reps calls each (50 in all by default), timed with device events; per call
the median over all its timings, the spread of the rounds' medians and the ratio to wfl_align.  The result goes to --out
(profiles/align_min_duration_bench.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from wfl_asr_amd import align as AL


def _times(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def _summary(rounds):
    med = [float(np.median(r)) for r in rounds]
    return {"ms_median": float(np.median(np.concatenate(rounds))), "ms_min": float(np.min(np.concatenate(rounds))),
            "round_medians_ms": med}


def min_duration_bench(reps, rounds, counts=(16, 64)):
    rng = np.random.default_rng(0)
    C, T, N = 141, 1500, 300
    out = {"T": T, "N": N, "C": C, "reps": reps, "rounds": rounds}
    depths = {"D1": [1] * N, "D3": [3] * N, "D5": [5] * N, "D8_every_second": [8, 1] * (N // 2)}
    for nb in counts:
        z = torch.from_numpy(rng.standard_normal((nb * T, C)).astype(np.float32) * 3).cuda()
        toks = [[[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 70, N)] for _ in range(nb)]
        gaps = [[0, 139, 140]] * nb
        args = (z, [T] * nb, toks, gaps, 0)
        packs = {"wfl_align": AL.pack_clips(*args[:4])}
        for name, d in depths.items():
            packs["min_duration_" + name] = AL.pack_clips(*args[:4], min_frames=[d] * nb)
        calls = {k: (lambda pk=pk: AL.viterbi_align(*args, packed=pk)) for k, pk in packs.items()}
        for fn in calls.values():
            assert int(fn()[3].max()) == 0
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(rounds):                            # alternating: a drift of the clock reaches all of them alike
            for k, fn in calls.items():
                ms[k].append(_times(fn, reps))
        res = {k: _summary(v) for k, v in ms.items()}
        for name in depths:
            res[name + "_to_wfl_align"] = res["min_duration_" + name]["ms_median"] / res["wfl_align"]["ms_median"]
        out[f"clips{nb}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/align_min_duration_bench.json")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    res = {"tool": "tools/align_min_duration_bench.py " + " ".join(sys.argv[1:]), "gpu": torch.cuda.get_device_name(0),
           "calls_device_events": min_duration_bench(a.reps, a.rounds)}
    out = a.out or os.path.join(ROOT, "profiles", "align_min_duration_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["calls_device_events"]))


if __name__ == "__main__":
    main()
