#!/usr/bin/env python3
"""Diagnostic (not product): the cost of the duration-prior decode's expected run lengths beside its posteriors and beside the
bigram's expected successions.

tools/decode_duration_posterior_bench.py's inputs: the SAME seeded random logits (resident) and the same random table in [-8, 0],
threshold 0.5, 16 clips x 1500 frames at P = 70 phonemes (C = 141), where the run history and the sums live in LDS, and at P = 191
(C = 383), where they live in the workspace; the duration table random in [-6, 0] with a fifth of the entries -inf, one row per phoneme,
D = 8 and D = 32.  Timed on those logits: wfl_decode_bigram_counts, and per D wfl_decode_duration_posterior on wfl_decode_duration's ids
and wfl_decode_duration_counts.  One process, --warmup untimed calls, then the median of --reps calls timed with device events
(tools/decode_bench.py's timing).  The result goes to --out (profiles/decode_duration_counts_bench.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np

from decode_bench import _timed


def bench(reps, warmup):
    import torch
    import synthetic as synth
    from wfl_asr_amd import decode as DC
    rng = np.random.default_rng(0)
    out = {"threshold": 0.5, "reps": reps, "warmup": warmup}
    nb, T = 16, 1500
    for P in (70, 191):
        table = DC.class_table(synth.make_labels(P))
        C = 2 * P + 1
        assert len(table.pairs) == P
        W = (-8.0 * rng.random((P + 1, P + 1))).astype(np.float32)
        z = torch.from_numpy(rng.standard_normal((nb * T, C)).astype(np.float32) * 3).cuda()
        sd = np.arange(P, dtype=np.int32)
        DC.bio_viterbi_bigram(z, [T] * nb, table, W, 0.5)       # (keeps the random stream that of the posterior bench)
        calls = {"wfl_decode_bigram_counts": (lambda: DC.bigram_expected_counts(z, [T] * nb, table, W, 0.5),
                                              DC.bigram_counts_workspace_bytes([T] * nb, P))}
        for D in (8, 32):
            dur = -6.0 * rng.random((P, D + 1))
            dur[rng.random(dur.shape) < 0.2] = -np.inf
            dur = dur.astype(np.float32)
            ids = DC.bio_viterbi_duration(z, [T] * nb, table, W, dur, sd, 0.5)[0]
            calls[f"wfl_decode_duration_posterior_D{D}"] = (
                lambda dur=dur, ids=ids: DC.decode_posteriors_duration(z, [T] * nb, table, W, dur, sd, 0.5, ids),
                DC.duration_posterior_workspace_bytes([T] * nb, P, D))
            calls[f"wfl_decode_duration_counts_D{D}"] = (lambda dur=dur: DC.duration_expected_counts(z, [T] * nb, table, W, dur, sd, 0.5),
                                                         DC.duration_counts_workspace_bytes([T] * nb, P, D))
        res = {"C": C, "phonemes": P, "clips": nb, "frames": T}
        for name, (fn, ws) in calls.items():
            for _ in range(warmup):
                assert int(fn()[-1].max()) == 0          # (status is the last result of every entry)
            res[name] = _timed(fn, reps)
            res[name]["workspace_bytes"] = ws
        for D in (8, 32):
            cnt = res[f"wfl_decode_duration_counts_D{D}"]["ms_median"]
            res[f"counts_D{D}_over_posterior"] = round(cnt / res[f"wfl_decode_duration_posterior_D{D}"]["ms_median"], 3)
            res[f"counts_D{D}_over_bigram_counts"] = round(cnt / res["wfl_decode_bigram_counts"]["ms_median"], 3)
        out[f"P{P}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_duration_counts_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    res = {"tool": f"tools/decode_duration_counts_bench.py --reps {a.reps} --warmup {a.warmup}", "gpu": torch.cuda.get_device_name(0),
           "timing": "whole Python call (uploads of the class table, the transition table and the duration table included), device events, "
                     "median",
           "calls": bench(a.reps, a.warmup)}
    print(json.dumps(res["calls"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
