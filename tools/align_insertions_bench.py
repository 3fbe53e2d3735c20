#!/usr/bin/env python3
"""Diagnostic (not product): the cost of `align_insertions`.

One wfl_align_insertions call beside one wfl_align_edits call and one wfl_align_posterior call on the same batches -- 16 and 64 clips x
1500 frames x N = 300 tokens, C = 141 (seeded random logits, resident, the batch packed once), the shapes of
tools/align_edits_bench.py -- for tables of 0, 1 and 70 substitutes (70: every phoneme of that label set; 0: the sweeps alone).  The
three calls alternate inside one process, --rounds times --reps calls each, timed with device events; per call the median over all
its timings, the spread of the rounds' medians, the ratio of the insertions to the edits call, and the workspaces.  The result goes
to --out (profiles/align_insertions_bench.json)."""
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


def insertions_bench(reps, rounds, tables=(0, 1, 70), counts=(16, 64)):
    rng = np.random.default_rng(0)
    C, T, N = 141, 1500, 300
    pairs = [(2 * p - 1, 2 * p) for p in range(1, 71)]
    out = {"T": T, "N": N, "C": C, "reps": reps, "rounds": rounds}
    for nb in counts:
        z = torch.from_numpy(rng.standard_normal((nb * T, C)).astype(np.float32) * 3).cuda()
        toks = [[[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 70, N)] for _ in range(nb)]
        gaps = [[0, 139, 140]] * nb
        args = (z, [T] * nb, toks, gaps, 0)
        tok = AL.viterbi_align(*args)[1]
        pk = AL.pack_clips(*args[:4])
        assert int(AL.alignment_posteriors(*args, tok, packed=pk)[4].max()) == 0
        res = {"posterior_workspace_bytes": AL.posterior_workspace_bytes([T] * nb, [N] * nb),
               "edits_workspace_bytes": AL.edits_workspace_bytes([T] * nb, [N] * nb),
               "insertions_workspace_bytes": AL.insertions_workspace_bytes([T] * nb, [N] * nb)}
        for P in tables:
            calls = {"alignment_posteriors": lambda: AL.alignment_posteriors(*args, tok, packed=pk),
                     "edit_scores": lambda: AL.edit_scores(*args, pairs[:P], packed=pk),
                     "insertion_scores": lambda: AL.insertion_scores(*args, pairs[:P], packed=pk)}
            assert int(calls["edit_scores"]()[2].max()) == 0 and int(calls["insertion_scores"]()[2].max()) == 0
            for fn in calls.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in calls}
            for _ in range(rounds):                        # alternating: a drift of the clock reaches all three alike
                for k, fn in calls.items():
                    ms[k].append(_times(fn, reps))
            r = {k: _summary(v) for k, v in ms.items()}
            r["insertions_to_edits"] = r["insertion_scores"]["ms_median"] / r["edit_scores"]["ms_median"]
            r["insertions_to_posterior"] = r["insertion_scores"]["ms_median"] / r["alignment_posteriors"]["ms_median"]
            res[f"P{P}"] = r
        out[f"clips{nb}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/align_insertions_bench.json")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    res = {"tool": "tools/align_insertions_bench.py " + " ".join(sys.argv[1:]), "gpu": torch.cuda.get_device_name(0),
           "calls_device_events": insertions_bench(a.reps, a.rounds)}
    out = a.out or os.path.join(ROOT, "profiles", "align_insertions_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["calls_device_events"]))


if __name__ == "__main__":
    main()
