#!/usr/bin/env python3
"""Diagnostic (not product): what `decode_scores` costs beside the search it scores.

One wfl_decode call, and one wfl_decode call followed by wfl_decode_posterior on its ids, for the shapes of profiles/decode_bench.json
(16 and 64 clips x 1500 frames and one 15 000-frame clip, C = 141, 70 phonemes, seeded random logits, resident, lambda 2, threshold
0.5): the median of --reps calls timed with device events after warm-up, and the ratio of the two.  --commit labels the result with
the commit it was measured on.  The result goes to --out (profiles/decode_posterior_bench.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

from decode_bench import _timed


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
        frames = [T] * nb

        def search():
            return DC.bio_viterbi(z, frames, table, 2.0, 0.5)

        def both():
            ids = search()[0]
            return DC.decode_posteriors(z, frames, table, 2.0, 0.5, ids)
        assert int(search()[2].max()) == 0 and int(both()[3].max()) == 0
        a, b = _timed(search, reps), _timed(both, reps)
        out[name] = {"decode": a, "decode_then_posterior": b, "ratio_of_medians": round(b["ms_median"] / a["ms_median"], 3),
                     "posterior_workspace_bytes": DC.posterior_workspace_bytes(frames, len(table.pairs))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_posterior_bench.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--commit", default="", help="the commit the library was built from (recorded in the result)")
    a = ap.parse_args()
    import torch
    res = {"tool": "tools/decode_posterior_bench.py --reps %d" % a.reps, "gpu": torch.cuda.get_device_name(0), "measured_on": a.commit,
           "calls_device_events": op_bench(a.reps)}
    print(json.dumps(res["calls_device_events"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
