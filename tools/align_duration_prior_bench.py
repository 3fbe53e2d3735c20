#!/usr/bin/env python3
"""Diagnostic (not product): what the explicit-duration search costs beside the plain alignment kernel.

--op: one wfl_align call (the yardstick) beside wfl_align_duration_prior calls at D = 8 and D = 32 on the same batches -- 16 and 64
clips x 1500 frames x N = 300 tokens, C = 141 (seeded random logits, resident, each batch packed once), the shapes of
tools/align_bench.py --op.  The table is a discretised gamma histogram per phoneme (mean 3 to 8 frames) with a geometric tail, every
entry finite, one row per phoneme.  At N = 300 the history ring of the D run scores lives in LDS at every D; a second shape, 16
clips x 1500 frames x N = 1100, shows the ring in LDS (D = 8) beside the ring in the clip's workspace (D = 32), each against wfl_align
at that shape.  The calls alternate inside one process, --rounds times, reps / rounds calls each, timed with device events; per call
the median and the minimum over all its timings, the rounds' medians and the ratio to wfl_align.  The result goes to --out
(profiles/align_duration_prior_bench.json)."""
import argparse
import json
import math
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


def gamma_table(n_rows, D, rng):
    """Per row a gamma-shaped duration histogram (shape 2 .. 4, mean 3 .. 8 frames) over d = 1 .. D and the geometric tail of its
    last two entries -> float32 [n_rows][D + 1], every entry finite."""
    t = np.zeros((n_rows, D + 1))
    d = np.arange(1, D + 2, dtype=np.float64)
    for r in range(n_rows):
        k, mean = rng.uniform(2, 4), rng.uniform(3, 8)
        logp = (k - 1) * np.log(d) - d * k / mean
        logp -= math.log(np.exp(logp).sum())
        t[r, :D] = logp[:D]
        t[r, D] = min(logp[D] - logp[D - 1], -1e-3)
    return t.astype(np.float32)


def op_bench(reps, rounds, shapes=((16, 300), (64, 300), (16, 1100)), depths=(8, 32)):
    rng = np.random.default_rng(0)
    C, T = 141, 1500
    out = {"T": T, "C": C, "reps": reps, "rounds": rounds}
    per_round = max(1, reps // rounds)
    for nb, N in shapes:
        z = torch.from_numpy(rng.standard_normal((nb * T, C)).astype(np.float32) * 3).cuda()
        phon = [rng.integers(1, 70, N) for _ in range(nb)]
        toks = [[[(int(2 * p - 1), int(2 * p))] for p in ph] for ph in phon]
        gaps = [[0, 139, 140]] * nb
        args = (z, [T] * nb, toks, gaps, 0)
        packed = AL.pack_clips(*args[:4])
        rows = AL.upload_durations([[int(p) - 1 for p in ph] for ph in phon], packed.N, z.device)
        calls = {"wfl_align": lambda: AL.viterbi_align(*args, packed=packed)}
        for D in depths:
            tab = torch.from_numpy(gamma_table(69, D, rng)).cuda()
            calls[f"duration_prior_D{D}"] = lambda tab=tab: AL.viterbi_align_duration_prior(*args, rows, tab, packed=packed)
        for fn in calls.values():
            assert int(fn()[3].max()) == 0
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(rounds):                            # alternating: a drift of the clock reaches all of them alike
            for k, fn in calls.items():
                ms[k].append(_times(fn, per_round))
        res = {k: _summary(v) for k, v in ms.items()}
        for D in depths:
            res[f"D{D}_to_wfl_align"] = res[f"duration_prior_D{D}"]["ms_median"] / res["wfl_align"]["ms_median"]
            res[f"D{D}_workspace_bytes"] = AL.duration_prior_workspace_bytes([T] * nb, [N] * nb, D)
        res["wfl_align_workspace_bytes"] = AL.workspace_bytes([T] * nb, [N] * nb)
        out[f"clips{nb}_N{N}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", action="store_true", help="the operator-level comparison (the only mode)")
    ap.add_argument("--out", default=None, help="default: profiles/align_duration_prior_bench.json")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    res = {"tool": "tools/align_duration_prior_bench.py " + " ".join(sys.argv[1:]), "gpu": torch.cuda.get_device_name(0),
           "calls_device_events": op_bench(a.reps, a.rounds)}
    out = a.out or os.path.join(ROOT, "profiles", "align_duration_prior_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["calls_device_events"]))


if __name__ == "__main__":
    main()
