#!/usr/bin/env python3
"""Diagnostic (not product): what the E-step of the duration prior's re-estimation costs.

--op: wfl_align_duration_prior_counts beside wfl_align_duration_prior_posterior (whose instantiations are the code they were) on the
same inputs in the same process, on the shapes of tools/align_duration_prior_posterior_bench.py -- 16 clips x 1500 frames (30 s) x
N = 300 tokens at D = 8 and D = 32 -- plus one clip of 4096 tokens (6000 frames, D = 8): C = 141, seeded random logits, resident, each
batch packed once, the same gamma-histogram tables.  The posterior's `tok` is its search's own output at that D; the counts take
none.  The calls alternate inside one process, --rounds times, reps / rounds calls each after a warm-up, timed with device events; per
call the median and the minimum over all its timings, the rounds' medians, and the ratio counts / posterior.  The result goes to --out
(profiles/align_duration_prior_counts_bench.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from align_duration_prior_bench import _summary, _times, gamma_table
from wfl_asr_amd import align as AL


def op_bench(reps, rounds, shapes=((16, 1500, 300, (8, 32)), (1, 6000, 4096, (8,)))):
    rng = np.random.default_rng(0)
    C = 141
    out = {"C": C, "reps": reps, "rounds": rounds}
    per_round = max(1, reps // rounds)
    for nb, T, N, depths in shapes:
        z = torch.from_numpy(rng.standard_normal((nb * T, C)).astype(np.float32) * 3).cuda()
        phon = [rng.integers(1, 70, N) for _ in range(nb)]
        toks = [[[(int(2 * p - 1), int(2 * p))] for p in ph] for ph in phon]
        gaps = [[0, 139, 140]] * nb
        args = (z, [T] * nb, toks, gaps, 0)
        packed = AL.pack_clips(*args[:4])
        rows = AL.upload_durations([[int(p) - 1 for p in ph] for ph in phon], packed.N, z.device)
        calls = {}
        for D in depths:
            tab = torch.from_numpy(gamma_table(69, D, rng)).cuda()
            tok = AL.viterbi_align_duration_prior(*args, rows, tab, packed=packed)[1]
            calls[f"duration_prior_posterior_D{D}"] = (lambda tab=tab, tok=tok:
                                                       AL.duration_prior_posteriors(*args, rows, tab, tok, packed=packed))
            calls[f"duration_prior_counts_D{D}"] = lambda tab=tab: AL.duration_prior_expected_counts(*args, rows, tab, packed=packed)
        for fn in calls.values():
            assert int(fn()[-1].max()) == 0               # (status is the last output of both)
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(rounds):                            # alternating: a drift of the clock reaches both alike
            for k, fn in calls.items():
                ms[k].append(_times(fn, per_round))
        res = {k: _summary(v) for k, v in ms.items()}
        for D in depths:
            res[f"D{D}_counts_to_posterior"] = (res[f"duration_prior_counts_D{D}"]["ms_median"]
                                                / res[f"duration_prior_posterior_D{D}"]["ms_median"])
            res[f"D{D}_counts_workspace_bytes"] = AL.duration_prior_counts_workspace_bytes([T] * nb, [N] * nb, D)
            res[f"D{D}_posterior_workspace_bytes"] = AL.duration_prior_posterior_workspace_bytes([T] * nb, [N] * nb, D)
        out[f"clips{nb}_T{T}_N{N}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", action="store_true", help="the operator-level comparison (the only mode)")
    ap.add_argument("--out", default=None, help="default: profiles/align_duration_prior_counts_bench.json")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    # (the record names what shaped the measurement, not where the file went)
    res = {"tool": f"tools/align_duration_prior_counts_bench.py --op --reps {a.reps} --rounds {a.rounds}", "gpu": torch.cuda.get_device_name(0),
           "calls_device_events": op_bench(a.reps, a.rounds)}
    out = a.out or os.path.join(ROOT, "profiles", "align_duration_prior_counts_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["calls_device_events"]))


if __name__ == "__main__":
    main()
