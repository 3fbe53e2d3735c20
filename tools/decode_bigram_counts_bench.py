#!/usr/bin/env python3
"""Diagnostic (not product): the cost of the expected successions (wfl_decode_bigram_counts) beside the posteriors of the same grammar.

One wfl_decode_bigram_counts call and one wfl_decode_bigram_posterior call (on wfl_decode_bigram's ids) on the SAME seeded random
logits (resident), threshold 0.5: the inputs of tools/decode_bigram_posterior_bench.py -- 64 clips x 1500 frames and one 15 000-frame
clip, at P = 70 (C = 141) and P = 191 (C = 383) phonemes, a random table in [-8, 0].  The median of --reps calls timed with device
events (tools/decode_bench.py's timing), from the one-clip case the time per frame of the two serial chains, and the ratio of the two
entries.  The result goes to --out (profiles/decode_bigram_counts_bench.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np

from decode_bench import _timed

KEYS = ("wfl_decode_bigram_posterior", "wfl_decode_bigram_counts")


def bench(reps):
    import torch
    import synthetic as synth
    from wfl_asr_amd import decode as DC
    rng = np.random.default_rng(0)
    out = {"threshold": 0.5, "reps": reps}
    for P in (70, 191):
        table = DC.class_table(synth.make_labels(P))
        C = 2 * P + 1
        assert len(table.pairs) == P
        W = (-8.0 * rng.random((P + 1, P + 1))).astype(np.float32)
        res = {"C": C, "phonemes": P}
        for name, nb, T in (("clips64_T1500", 64, 1500), ("clips1_T15000", 1, 15000)):
            z = torch.from_numpy(rng.standard_normal((nb * T, C)).astype(np.float32) * 3).cuda()
            ids, _, st = DC.bio_viterbi_bigram(z, [T] * nb, table, W, 0.5)
            assert int(st.max()) == 0
            assert int(DC.decode_posteriors_bigram(z, [T] * nb, table, W, 0.5, ids)[3].max()) == 0
            assert int(DC.bigram_expected_counts(z, [T] * nb, table, W, 0.5)[2].max()) == 0
            res[name] = {"wfl_decode_bigram_posterior": _timed(lambda: DC.decode_posteriors_bigram(z, [T] * nb, table, W, 0.5, ids), reps),
                         "wfl_decode_bigram_counts": _timed(lambda: DC.bigram_expected_counts(z, [T] * nb, table, W, 0.5), reps),
                         "workspace_bytes": {"wfl_decode_bigram_posterior": DC.bigram_posterior_workspace_bytes([T] * nb, P),
                                             "wfl_decode_bigram_counts": DC.bigram_counts_workspace_bytes([T] * nb, P)}}
            r = res[name]
            r["counts_over_posterior"] = round(r["wfl_decode_bigram_counts"]["ms_median"] / r["wfl_decode_bigram_posterior"]["ms_median"], 3)
            if nb == 1:
                for k in KEYS:
                    r[k]["us_per_frame"] = round(r[k]["ms_median"] * 1e3 / T, 4)
        out[f"P{P}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_bigram_counts_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    res = {"tool": f"tools/decode_bigram_counts_bench.py --reps {a.reps}", "gpu": torch.cuda.get_device_name(0),
           "timing": "whole Python call (uploads of the class table / transition table included), device events, median",
           "calls": bench(a.reps)}
    print(json.dumps(res["calls"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
