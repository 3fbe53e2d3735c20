#!/usr/bin/env python3
"""Diagnostic (not product): what the filler emission of wfl_align_filler costs the alignment kernel.

One wfl_align call (the yardstick) beside wfl_align_filler calls with no flag set, with one token in twenty a filler and with every
third token a filler (filler penalty 1 nat), on the same batch -- 16 clips x 1500 frames x N = 300 tokens, C = 141 (seeded random
logits, resident, the batch packed once), the shapes of tools/align_optional_bench.py.  The calls alternate inside one process,
--rounds times, reps calls each (50 in all by default), timed with device events; per call the median over all its timings, the
spread of the rounds' medians and the ratio to wfl_align.  The result goes to --out (profiles/align_filler_bench.json).

wfl_align across commits: --tree DIR runs the same batch with the package of another checkout of this repository (built there; it
need not know wfl_align_filler) and times wfl_align alone; --against FILE (repeatable) then takes such runs' results into the
record, beside this tree's own wfl_align, with the ratio of the medians.  Run the trees in turn in one session."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tree():
    for i, a in enumerate(sys.argv):
        if a == "--tree" and i + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[i + 1])
        if a.startswith("--tree="):
            return os.path.abspath(a[len("--tree="):])
    return HERE


ROOT = _tree()
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
            "round_medians_ms": med, "round_spread": (max(med) - min(med)) / float(np.median(med))}


def filler_bench(reps, rounds, counts=(16,), phi=1.0):
    rng = np.random.default_rng(0)
    C, T, N = 141, 1500, 300
    out = {"T": T, "N": N, "C": C, "reps": reps, "rounds": rounds, "filler_penalty": phi}
    with_filler = hasattr(AL, "viterbi_align_filler")
    flags = {"no_flag": [False] * N, "one_in_twenty": [k % 20 == 10 for k in range(N)], "every_third": [k % 3 == 1 for k in range(N)]}
    for nb in counts:
        z = torch.from_numpy(rng.standard_normal((nb * T, C)).astype(np.float32) * 3).cuda()
        toks = [[[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 70, N)] for _ in range(nb)]
        gaps = [[0, 139, 140]] * nb
        args = (z, [T] * nb, toks, gaps, 0)
        pk = AL.pack_clips(*args[:4])
        calls = {"wfl_align": lambda: AL.viterbi_align(*args, packed=pk)}
        if with_filler:
            for name, f in flags.items():                  # (a flagged token keeps its row of the token table: one valid pair, never read)
                d_f = AL.upload_filler([f] * nb, pk.N, z.device)        # (packed and uploaded once, as the token tables are)
                calls["filler_" + name] = lambda d_f=d_f: AL.viterbi_align_filler(*args, d_f, phi, packed=pk)
        frames = {}
        for k, fn in calls.items():
            res = fn()
            assert int(res[3].max()) == 0
            if k.startswith("filler_"):                    # the share of the frames the path gives to fillers
                tok = res[1].cpu().numpy().reshape(nb, T)
                f = np.array(flags[k[len("filler_"):]])
                frames[k] = float((f[np.maximum(tok, 0)] & (tok >= 0)).mean())
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(rounds):                            # alternating: a drift of the clock reaches all of them alike
            for k, fn in calls.items():
                ms[k].append(_times(fn, reps))
        res = {k: _summary(v) for k, v in ms.items()}
        for k, frac in frames.items():
            res[k]["filler_frame_fraction"] = frac
            res[k[len("filler_"):] + "_to_wfl_align"] = res[k]["ms_median"] / res["wfl_align"]["ms_median"]
        out[f"clips{nb}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/align_filler_bench.json")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tree", default=None, help="another checkout of this repository, built: time its wfl_align alone")
    ap.add_argument("--against", action="append", default=[], help="the result file of a --tree run, taken into the record (repeatable)")
    a = ap.parse_args()
    res = {"tool": "tools/align_filler_bench.py " + " ".join(sys.argv[1:]), "gpu": torch.cuda.get_device_name(0),
           "calls_device_events": filler_bench(a.reps, a.rounds)}
    if a.against:
        others = []
        for path in a.against:
            with open(path) as f:
                others.append(json.load(f)["calls_device_events"])
        cmp = {}
        for key in ("clips16",):
            mine = res["calls_device_events"][key]["wfl_align"]
            theirs = [o[key]["wfl_align"] for o in others]
            other = float(np.median([t["ms_median"] for t in theirs]))
            spread = max([mine["round_spread"]] + [t["round_spread"] for t in theirs])
            cmp[key] = {"other_tree_runs": theirs, "this_tree": mine, "this_to_other_median": mine["ms_median"] / other,
                        # what must hold: this tree's median within the other's plus the larger of the records' round spreads
                        "allowed_ratio": 1.0 + spread, "within_spread": bool(mine["ms_median"] <= other * (1.0 + spread))}
        res["wfl_align_against_other_tree"] = cmp
    out = a.out or os.path.join(HERE, "profiles", "align_filler_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
