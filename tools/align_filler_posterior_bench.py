#!/usr/bin/env python3
"""Diagnostic (not product): what the filler emission and the end moments of wfl_align_filler_posterior cost the forward-backward
kernel.

One wfl_align_posterior call (the yardstick) beside wfl_align_filler_posterior calls with no flag set, with one token in twenty
flagged and with every third token flagged (filler penalty 1 nat), on the same batch -- 16 clips x 1500 frames x N = 300 tokens,
C = 141 (seeded random logits, resident, the batch packed once, the flags uploaded once), the shapes of
tools/align_optional_posterior_bench.py.  Every call scores the `tok` of its own search: wfl_align's for the yardstick,
wfl_align_filler's with the same flags for the others.  The calls alternate inside one process, --rounds times, reps calls each after
three warm-up calls, timed with device events; per call the median over all its timings, the spread of the rounds' medians and the
ratio to wfl_align_posterior.  There is no pass / fail ratio: the figures are reported.  The result goes to --out
(profiles/align_filler_posterior_bench.json)."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

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
            "round_medians_ms": med, "round_spread": (max(med) - min(med)) / float(np.median(med))}


def bench(reps, rounds, counts=(16,), phi=1.0):
    rng = np.random.default_rng(0)
    C, T, N = 141, 1500, 300
    out = {"T": T, "N": N, "C": C, "reps": reps, "rounds": rounds, "filler_penalty": phi}
    flags = {"no_flag": [False] * N, "one_in_twenty": [k % 20 == 7 for k in range(N)], "every_third": [k % 3 == 1 for k in range(N)]}
    for nb in counts:
        z = torch.from_numpy(rng.standard_normal((nb * T, C)).astype(np.float32) * 3).cuda()
        toks = [[[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 70, N)] for _ in range(nb)]
        gaps = [[0, 139, 140]] * nb
        args = (z, [T] * nb, toks, gaps, 0)
        pk = AL.pack_clips(*args[:4])
        _, tok, _, st = AL.viterbi_align(*args, packed=pk)
        assert int(st.max()) == 0
        calls = {"wfl_align_posterior": lambda tok=tok: AL.alignment_posteriors(*args, tok, packed=pk)}
        info = {}
        for name, f in flags.items():
            d_f = AL.upload_filler([f] * nb, pk.N, z.device)
            _, tok_f, _, st = AL.viterbi_align_filler(*args, d_f, phi, packed=pk)
            assert int(st.max()) == 0
            calls["filler_" + name] = lambda d_f=d_f, tok_f=tok_f: AL.filler_posteriors(*args, d_f, tok_f, phi, packed=pk)
            fl = torch.tensor(f, device=z.device)              # (tok is the token's index inside its clip)
            frames = (tok_f >= 0) & fl[tok_f.clamp(min=0).long()]
            info["filler_" + name] = {"filler_frame_fraction": float(frames.float().mean())}
        for k, fn in calls.items():
            res = fn()
            assert int(res[-1].max()) == 0
            if k in info:
                info[k]["mean_end_sd_frames"] = float(res[5][:nb * N].mean())
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(rounds):                            # alternating: a drift of the clock reaches all of them alike
            for k, fn in calls.items():
                ms[k].append(_times(fn, reps))
        res = {k: _summary(v) for k, v in ms.items()}
        for k, extra in info.items():
            res[k].update(extra)
            res[k[len("filler_"):] + "_to_wfl_align_posterior"] = res[k]["ms_median"] / res["wfl_align_posterior"]["ms_median"]
        out[f"clips{nb}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/align_filler_posterior_bench.json")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    res = {"tool": f"tools/align_filler_posterior_bench.py --reps {a.reps} --rounds {a.rounds}", "gpu": torch.cuda.get_device_name(0),   # (no path)
           "calls_device_events": bench(a.reps, a.rounds)}
    out = a.out or os.path.join(HERE, "profiles", "align_filler_posterior_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
