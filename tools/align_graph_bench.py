#!/usr/bin/env python3
"""Diagnostic (not product): what the predecessor gather of wfl_align_graph costs the alignment kernel.

One wfl_align call (the yardstick, from the same build) beside two wfl_align_graph calls on the same batch -- 16 clips x 1500 frames x
300 tokens, C = 141 (seeded random logits, resident, each batch packed once), as profiles/align_bench.json was taken: the transcripts as
chain graphs (the same lattice, state for state), and the same transcripts with a 2-variant group in place of every tenth token (330
slots).  The calls alternate inside one process, --rounds times, reps calls each (50 in all by default), timed with device events; per
call the median over all its timings, the spread of the rounds' medians and the ratio to wfl_align.  The result goes to --out
(profiles/align_graph_bench.json)."""
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


def _pair(p):
    return [(int(2 * p - 1), int(2 * p))]


def graph_bench(reps, rounds, nb=16):
    rng = np.random.default_rng(0)
    C, T, N = 141, 1500, 300
    z = torch.from_numpy(rng.standard_normal((nb * T, C)).astype(np.float32) * 3).cuda()
    phon = [rng.integers(1, 70, N) for _ in range(nb)]
    toks = [[_pair(p) for p in ph] for ph in phon]
    gaps = [[0, 139, 140]] * nb
    chain = AL.chain_graph(N)
    # a 2-variant group in place of every tenth token: the token as written, or another phoneme
    graphs, slot_cls = [], []
    for ph in phon:
        elements, cls = [], []
        for k, p in enumerate(ph):
            if k % 10 == 5:
                elements.append(((f"t{k}",), (f"u{k}",)))
                cls += [_pair(p), _pair(1 + (int(p) + 34) % 69)]
            else:
                elements.append(f"t{k}")
                cls.append(_pair(p))
        graphs.append(AL.compile_graph(elements))
        slot_cls.append(cls)
    n_slots = len(graphs[0].slots)
    pk = AL.pack_clips(z, [T] * nb, toks, gaps)
    pk_chain = AL.pack_graph(z, [T] * nb, toks, [chain[0]] * nb, [chain[1]] * nb, gaps)
    pk_groups = AL.pack_graph(z, [T] * nb, slot_cls, [g.preds for g in graphs], [g.final for g in graphs], gaps)
    calls = {"wfl_align": lambda: AL.viterbi_align(z, [T] * nb, toks, gaps, 0, packed=pk),
             "graph_chain": lambda: AL.viterbi_align_graph(z, [T] * nb, None, None, None, None, 0, packed=pk_chain),
             "graph_groups": lambda: AL.viterbi_align_graph(z, [T] * nb, None, None, None, None, 0, packed=pk_groups)}
    first = {k: fn() for k, fn in calls.items()}
    assert all(int(r[3].max()) == 0 for r in first.values())
    assert torch.equal(first["wfl_align"][0], first["graph_chain"][0]) and torch.equal(first["wfl_align"][1], first["graph_chain"][1])
    gain = (first["graph_groups"][2] - first["wfl_align"][2]).cpu().numpy()
    assert (gain >= -1e-3 * T).all()
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(rounds):                                # alternating: a drift of the clock reaches all of them alike
        for k, fn in calls.items():
            ms[k].append(_times(fn, reps))
    res = {k: _summary(v) for k, v in ms.items()}
    res["graph_chain_to_wfl_align"] = res["graph_chain"]["ms_median"] / res["wfl_align"]["ms_median"]
    res["graph_groups_to_wfl_align"] = res["graph_groups"]["ms_median"] / res["wfl_align"]["ms_median"]
    res["mean_gain_nats"] = float(gain.mean())
    return {"T": T, "N": N, "C": C, "clips": nb, "slots_with_groups": n_slots, "groups": len(graphs[0].groups), "reps": reps,
            "rounds": rounds, f"clips{nb}": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/align_graph_bench.json")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    res = {"tool": "tools/align_graph_bench.py " + " ".join(sys.argv[1:]), "gpu": torch.cuda.get_device_name(0),
           "calls_device_events": graph_bench(a.reps, a.rounds)}
    out = a.out or os.path.join(HERE, "profiles", "align_graph_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
