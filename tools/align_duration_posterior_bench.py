#!/usr/bin/env python3
"""Diagnostic (not product): what the minimum-duration chain costs the posterior kernel.

One wfl_align_posterior call (the yardstick, on the path of wfl_align) beside wfl_align_min_duration_posterior calls with every
D_k = 1, 3 and 5, and with D_k = 8 for every second token (1 for the others), each on the path wfl_align_min_duration gave for the
same durations, on the same batches -- 16 and 64 clips x 1500 frames x N = 300 tokens, C = 141 (seeded random logits, resident, each
batch packed once), the shapes of tools/align_min_duration_bench.py.  (Every D_k = 8 would need 2400 frames: at this shape it has no
path.)  The calls alternate inside one process, --rounds times, reps calls each (50 in all by default), timed with device events; per
call the median over all its timings, the spread of the rounds' medians, the ratio to wfl_align_posterior and the workspace bytes.
The result goes to --out (profiles/align_duration_posterior_bench.json).

--plain-only times wfl_align_posterior alone and touches nothing newer: the same file run inside a checkout of an earlier commit gives
that commit's figure for the same batches, and several such runs beside runs of this commit give the run-to-run spread
(--merge-runs folds their outputs into the profile)."""
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


def duration_posterior_bench(reps, rounds, counts=(16, 64), plain_only=False):
    rng = np.random.default_rng(0)
    C, T, N = 141, 1500, 300
    out = {"T": T, "N": N, "C": C, "reps": reps, "rounds": rounds}
    depths = {} if plain_only else {"D1": [1] * N, "D3": [3] * N, "D5": [5] * N, "D8_every_second": [8, 1] * (N // 2)}
    for nb in counts:
        z = torch.from_numpy(rng.standard_normal((nb * T, C)).astype(np.float32) * 3).cuda()
        toks = [[[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 70, N)] for _ in range(nb)]
        gaps = [[0, 139, 140]] * nb
        args = (z, [T] * nb, toks, gaps, 0)
        plain = AL.pack_clips(*args[:4])
        tok = AL.viterbi_align(*args, packed=plain)[1]
        calls = {"wfl_align_posterior": lambda: AL.alignment_posteriors(*args, tok, packed=plain)}
        res = {"workspace_bytes": {"wfl_align_posterior": AL.posterior_workspace_bytes([T] * nb, [N] * nb)}}
        for name, d in depths.items():
            pk = AL.pack_clips(*args[:4], min_frames=[d] * nb)
            _, dtok, _, st = AL.viterbi_align(*args, packed=pk)
            assert int(st.max()) == 0
            calls["duration_posterior_" + name] = lambda pk=pk, dtok=dtok: AL.duration_posteriors(*args, dtok, packed=pk)
        if depths:
            res["workspace_bytes"]["wfl_align_min_duration_posterior"] = AL.duration_posterior_workspace_bytes([T] * nb, [N] * nb)
        for fn in calls.values():
            assert int(fn()[4].max()) == 0
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(rounds):                            # alternating: a drift of the clock reaches all of them alike
            for k, fn in calls.items():
                ms[k].append(_times(fn, reps))
        res.update({k: _summary(v) for k, v in ms.items()})
        for name in depths:
            res[name + "_to_wfl_align_posterior"] = res["duration_posterior_" + name]["ms_median"] / res["wfl_align_posterior"]["ms_median"]
        out[f"clips{nb}"] = res
    return out


def merge_runs(profile, parent_runs, this_runs):
    """Fold the --plain-only outputs of runs of the parent commit and of this commit (taken alternately in one session) into the
    profile: per batch the runs' medians of wfl_align_posterior, the parent's run-to-run spread, whether this commit's runs lie inside
    it, and the duration entry's ratios against the parent's median."""
    out = {}
    for key in [k for k in profile["calls_device_events"] if k.startswith("clips")]:
        par = [r["calls_device_events"][key]["wfl_align_posterior"]["ms_median"] for r in parent_runs]
        new = [r["calls_device_events"][key]["wfl_align_posterior"]["ms_median"] for r in this_runs]
        pm = float(np.median(par))
        e = {"parent_runs_ms": par, "this_commit_runs_ms": new, "parent_median_ms": pm,
             "parent_spread": (max(par) - min(par)) / pm, "this_commit_median_to_parent": float(np.median(new)) / pm,
             "this_commit_inside_parent_range": bool(min(par) <= float(np.median(new)) <= max(par))}
        for name, v in profile["calls_device_events"][key].items():
            if name.startswith("duration_posterior_"):
                e[name[len("duration_posterior_"):] + "_to_parent_wfl_align_posterior"] = v["ms_median"] / pm
        out[key] = e
    profile["against_parent_commit"] = out
    return profile


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/align_duration_posterior_bench.json")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true", help="time wfl_align_posterior alone (runs in an earlier checkout as well)")
    ap.add_argument("--merge-runs", nargs=2, metavar=("PARENT_GLOB", "THIS_GLOB"), default=None,
                    help="no timing: fold --plain-only outputs of the parent commit and of this one into the profile at --out")
    a = ap.parse_args()
    out = a.out or os.path.join(ROOT, "profiles", "align_duration_posterior_bench.json")
    if a.merge_runs:
        import glob
        load = lambda pat: [json.load(open(p)) for p in sorted(glob.glob(pat))]     # noqa: E731
        res = merge_runs(json.load(open(out)), load(a.merge_runs[0]), load(a.merge_runs[1]))
    else:
        res = {"tool": "tools/align_duration_posterior_bench.py " + " ".join(sys.argv[1:]), "gpu": torch.cuda.get_device_name(0),
               "calls_device_events": duration_posterior_bench(a.reps, a.rounds, plain_only=a.plain_only)}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res.get("against_parent_commit") if a.merge_runs else res["calls_device_events"]))


if __name__ == "__main__":
    main()
