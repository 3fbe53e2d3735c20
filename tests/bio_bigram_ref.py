"""float64 numpy restatement of the BIO-grammar Viterbi decode with a phone-bigram prior that wfl_decode_bigram computes
(include/wfl_asr.h), for the tests.  `plant` and `prepass` are tests/bio_viterbi_ref.py's.

Symbols: 0 is O, 1 + p is phoneme p of the table.  States, legality, forced frames and the virtual O frame before frame 0 are
bio_viterbi_ref's; the path maximises  sum_t z[t][c_t] + sum over opened runs W[previous symbol][opened symbol]:  a run is opened by
every B-q frame and by every O frame whose predecessor is not O; the previous symbol of a frame in B-p or I-p is p, of a frame in O it
is O; W[O][O] is never read.  With end[O] = d[O], end[p] = max(d[B-p], d[I-p]):
    B-q : z + max_s (end[s] + W[s][q])     O : z + max(d[O], max_{p != O} (end[p] + W[p][O]))     I-q : z + max(d[I-q], d[B-q])
The lowest predecessor symbol wins a tie, I-p wins a tie against B-p, the end state is the best symbol of the last frame.
`table` is (o_id, [(B class, I class or -1), ...]); W a [P + 1, P + 1] array, entries finite or -inf; `forced` a bool per frame.
"""
from __future__ import annotations

import numpy as np

from bio_viterbi_ref import NEG, _split, legal, plant, prepass  # noqa: F401  (re-exported for the tests)


def _symbols(table):
    """class -> symbol (O 0, B-p and I-p 1 + p; -1: never chosen), class -> kind (0 O, 1 B, 2 I, 3 never chosen)."""
    o, B, I = _split(table)
    sym, kind = {o: 0}, {o: 0}
    for p, (b, i) in enumerate(zip(B, I)):
        sym[int(b)], kind[int(b)] = p + 1, 1
        if i >= 0:
            sym[int(i)], kind[int(i)] = p + 1, 2
    return sym, kind


def viterbi(z, table, W, forced=None):
    """-> (ids [T] int32, objective)."""
    o, B, I = _split(table)
    z = np.asarray(z, np.float64)
    W = np.asarray(W, np.float64)
    T, P = z.shape[0], len(B)
    assert W.shape == (P + 1, P + 1)
    if T == 0:
        return np.zeros(0, np.int32), 0.0
    hasI = I >= 0
    Is = np.where(hasI, I, o)
    dO, dB, dI = 0.0, np.full(P, NEG), np.full(P, NEG)
    A = np.zeros((T, P + 1), np.int64)        # the winning predecessor symbol per opened symbol
    OB = np.zeros(T, bool)
    IB = np.zeros((T, P), bool)
    forced = np.zeros(T, bool) if forced is None else np.asarray(forced, bool)
    for t in range(T):
        end = np.concatenate([[dO], np.maximum(dB, dI)])
        cand = end[:, None] + W                # [previous][opened]
        cand[0, 0] = NEG                       # O after O is no opened run
        arg = cand.argmax(axis=0)              # (the first maximum: the lowest symbol)
        best = cand[arg, np.arange(P + 1)]
        ob = not (dO >= best[0])
        ib = ~(dI >= dB) | ~hasI
        eB = z[t, B].copy()
        eI = np.where(hasI, z[t, Is], NEG)
        if forced[t]:
            eB[:] = NEG
            eI[:] = NEG
        dI = np.where(ib, dB, dI) + eI
        dB = best[1:] + eB
        dO = z[t, o] + (best[0] if ob else dO)
        A[t], OB[t], IB[t] = arg, ob, ib
    end = np.concatenate([[dO], np.maximum(dB, dI)])
    q = int(end.argmax())
    isI = bool(q and hasI[q - 1] and dI[q - 1] >= dB[q - 1])
    obj = float(end[q])
    ids = np.empty(T, np.int32)
    for t in range(T - 1, -1, -1):
        ids[t] = o if q == 0 else (I[q - 1] if isI else B[q - 1])
        s = -1
        if q == 0:
            if OB[t]:
                s = int(A[t, 0])
        elif isI:
            if IB[t, q - 1]:
                isI = False
        else:
            s = int(A[t, q])
        if s >= 0:
            q = s
            isI = bool(q and not IB[t, q - 1])
    return ids, obj


def objective(ids, z, table, W, forced=None):
    """float64 objective of a LEGAL path: the logits on it plus W per opened run; -inf when a forced frame is not O or a succession
    is forbidden."""
    o = int(table[0])
    sym, kind = _symbols(table)
    z = np.asarray(z, np.float64)
    W = np.asarray(W, np.float64)
    tot, prev = 0.0, 0
    for t, c in enumerate(int(c) for c in ids):
        if forced is not None and forced[t] and c != o:
            return NEG
        tot += z[t, c]
        if kind[c] == 1 or (kind[c] == 0 and prev != 0):
            tot += W[prev, sym[c]]
        prev = sym[c]
    return float(tot)


def score(ids, z, table, W, forced=None):
    """What wfl_decode_bigram reports: the objective minus the frames' log-sum-exp (float64)."""
    return objective(ids, z, table, W, forced) - float(prepass(z, 0.0)[0].sum())


def forbidden_successions(ids, table, W):
    """How many opened runs of the path take a -inf entry of W."""
    sym, kind = _symbols(table)
    n, prev = 0, 0
    for c in (int(c) for c in ids):
        if (kind[c] == 1 or (kind[c] == 0 and prev != 0)) and np.isneginf(W[prev, sym[c]]):
            n += 1
        prev = sym[c]
    return n


def brute_force(z, table, W, forced=None):
    """Every class string over ALL C classes enumerated (tiny T and C only) -> (ids, the best objective among the legal ones)."""
    o, B, I = _split(table)
    sym, kind = _symbols(table)
    z = np.asarray(z, np.float64)
    W = np.asarray(W, np.float64)
    T, C = z.shape
    step = np.full((C + 1, C), NEG)             # [previous class; row C: the virtual O frame][class]: the transition's weight
    for prev in list(range(C)) + [C]:
        if prev < C and prev not in sym:
            continue
        ps = 0 if prev == C else sym[prev]
        for c in range(C):
            k = kind.get(c, 3)
            if k == 0:
                step[prev, c] = W[ps, 0] if ps != 0 else 0.0
            elif k == 1:
                step[prev, c] = W[ps, sym[c]]
            elif k == 2 and prev < C and sym[prev] == sym[c] and kind[prev] in (1, 2):
                step[prev, c] = 0.0
    paths = np.stack(np.meshgrid(*[np.arange(C)] * T, indexing="ij"), -1).reshape(-1, T)
    tot = z[0, paths[:, 0]] + step[C, paths[:, 0]]
    for t in range(1, T):
        tot = tot + z[t, paths[:, t]] + step[paths[:, t - 1], paths[:, t]]
    if forced is not None:
        for t in range(T):
            if forced[t]:
                tot = np.where(paths[:, t] == o, tot, NEG)
    k = int(np.argmax(tot))
    return paths[k].astype(np.int32), float(tot[k])
