"""float64 numpy restatement of the BIO-grammar Viterbi decode with a phone-bigram prior and a duration prior per phoneme that
wfl_decode_duration computes (include/wfl_asr.h), for the tests.  `plant`, `prepass` and `legal` are tests/bio_viterbi_ref.py's, the
symbols tests/bio_bigram_ref.py's.

Symbols, states, legality, forced frames, the virtual O frame and the table W are bio_bigram_ref's.  A run of phoneme q is one B-q
frame and then zero or more I-q frames; B-q after B-q / I-q opens a new run.  The path maximises
    sum_t z[t][c_t] + sum over opened runs W[previous symbol][opened symbol] + sum over phoneme runs L_q(d)
with L_q(d) = dur[r][d - 1] for d <= D, dur[r][D - 1] + (d - D) dur[r][D] beyond, r = sym_dur[q - 1], and L = 0 for r = -1.  O runs
carry no prior; the run in progress at the last frame ends there.  Frame by frame (frame t - 1 on the right):
    In_q(t)  = max_s (end_s(t-1) + W[s][q])                              the lowest s on a tie
    R_q^1(t) = In_q(t) + zB_t(q);    R_q^j(t) = R_q^{j-1}(t-1) + zI_t(q)   2 <= j <= D
    Y_q(t)   = max(Y_q(t-1), R_q^D(t-1) + L_q(D)) + zI_t(q) + tail_q      Y first on a tie
    end_q(t) = max(max_j R_q^j(t) + L_q(j), Y_q(t))                       the shortest j first, Y last on a tie
    O        : z + max(d[O], max_{p != O} (end_p(t-1) + W[p][O]))
`table` is (o_id, [(B class, I class or -1), ...]); W a [P + 1, P + 1] array; dur a [rows, D + 1] array, entries finite or -inf;
sym_dur [P] ints; `forced` a bool per frame.
"""
from __future__ import annotations

import numpy as np

from bio_bigram_ref import _symbols
from bio_viterbi_ref import NEG, _split, legal, plant, prepass  # noqa: F401  (re-exported for the tests)


def _rows(dur, sym_dur, P):
    """-> (L [P, D] float64, tail [P]) per phoneme; zeros for a phoneme without prior."""
    dur = np.asarray(dur, np.float64)
    D = dur.shape[1] - 1
    L, tail = np.zeros((P, D)), np.zeros(P)
    for p, r in enumerate(int(r) for r in sym_dur):
        if r >= 0:
            L[p], tail[p] = dur[r, :D], dur[r, D]
    return L, tail


def run_score(L, tail, p, d):
    """L_p(d), d >= 1."""
    D = L.shape[1]
    if d <= D:
        return float(L[p, d - 1])
    return float(L[p, D - 1] + (d - D) * tail[p])      # (-inf only ever adds: a finite multiple of -inf, or -inf + -inf)


def viterbi(z, table, W, dur, sym_dur, forced=None):
    """-> (ids [T] int32, objective)."""
    o, B, I = _split(table)
    z = np.asarray(z, np.float64)
    W = np.asarray(W, np.float64)
    T, P = z.shape[0], len(B)
    assert W.shape == (P + 1, P + 1) and len(sym_dur) == P
    if T == 0:
        return np.zeros(0, np.int32), 0.0
    L, tail = _rows(dur, sym_dur, P)
    D = L.shape[1]
    hasI = I >= 0
    Is = np.where(hasI, I, o)
    forced = np.zeros(T, bool) if forced is None else np.asarray(forced, bool)
    dO = 0.0
    R = np.full((P, D), NEG)                   # R[:, j - 1] = R^j
    Y = np.full(P, NEG)
    end = np.concatenate([[0.0], np.full(P, NEG)])
    A = np.zeros((T, P + 1), np.int64)         # the winning predecessor symbol per opened symbol
    OB = np.zeros(T, bool)
    DW = np.zeros((T, P), np.int64)            # end's winning duration, D + 1 for Y
    YB = np.zeros((T, P), bool)                # Y entered (True) or stayed
    with np.errstate(invalid="ignore"):
        for t in range(T):
            cand = end[:, None] + W
            cand[0, 0] = NEG                   # O after O is no opened run
            arg = cand.argmax(axis=0)          # (the first maximum: the lowest symbol)
            best = cand[arg, np.arange(P + 1)]
            ob = not (dO >= best[0])
            eB = z[t, B].copy()
            eI = np.where(hasI, z[t, Is], NEG)
            if forced[t]:
                eB[:] = NEG
                eI[:] = NEG
            yc = R[:, D - 1] + L[:, D - 1]
            yb = yc > Y
            Y = (np.where(yb, yc, Y) + eI) + tail
            Rn = np.empty_like(R)
            Rn[:, 0] = best[1:] + eB
            Rn[:, 1:] = R[:, :-1] + eI[:, None]
            R = Rn
            x = R + L
            dw = x.argmax(axis=1)              # (the first maximum: the shortest duration)
            xe = x[np.arange(P), dw]
            take_y = Y > xe
            dO = z[t, o] + (best[0] if ob else dO)
            end = np.concatenate([[dO], np.where(take_y, Y, xe)])
            A[t], OB[t], DW[t], YB[t] = arg, ob, np.where(take_y, D + 1, dw + 1), yb
    q = int(end.argmax())
    obj = float(end[q])
    ids = np.empty(T, np.int32)
    t = T - 1
    while t >= 0:
        if q == 0:
            ids[t] = o
            if OB[t]:
                q = int(A[t, 0])
            t -= 1
            continue
        p = q - 1
        d = int(DW[t, p])
        if d > D:                               # the tail: follow Y to the frame it was entered at
            while not YB[t, p]:
                ids[t] = I[p]
                t -= 1
            ids[t] = I[p]
            t -= 1
            d = D
        for _ in range(d - 1):
            ids[t] = I[p]
            t -= 1
        ids[t] = B[p]
        q = int(A[t, q])
        t -= 1
    return ids, obj


def run_lengths(ids, table):
    """The phoneme runs of a LEGAL path -> [(symbol, first frame, frames)]."""
    sym, kind = _symbols(table)
    runs = []
    for t, c in enumerate(int(c) for c in ids):
        if kind[c] == 1:
            runs.append([sym[c], t, 1])
        elif kind[c] == 2:
            runs[-1][2] += 1
    return [tuple(r) for r in runs]


def objective(ids, z, table, W, dur, sym_dur, forced=None):
    """float64 objective of a LEGAL path: the logits on it, W per opened run and L per phoneme run; -inf when a forced frame is not O,
    a succession is forbidden or a run has a forbidden duration."""
    o = int(table[0])
    sym, kind = _symbols(table)
    z = np.asarray(z, np.float64)
    W = np.asarray(W, np.float64)
    L, tail = _rows(dur, sym_dur, len(table[1]))
    tot, prev = 0.0, 0
    for t, c in enumerate(int(c) for c in ids):
        if forced is not None and forced[t] and c != o:
            return NEG
        tot += z[t, c]
        if kind[c] == 1 or (kind[c] == 0 and prev != 0):
            tot += W[prev, sym[c]]
        prev = sym[c]
    for s, _, d in run_lengths(ids, table):
        tot += run_score(L, tail, s - 1, d)
    return float(tot)


def score(ids, z, table, W, dur, sym_dur, forced=None):
    """What wfl_decode_duration reports: the objective minus the frames' log-sum-exp (float64)."""
    return objective(ids, z, table, W, dur, sym_dur, forced) - float(prepass(z, 0.0)[0].sum())


def forbidden_durations(ids, table, dur, sym_dur):
    """How many phoneme runs of the path have a length whose L is -inf."""
    L, tail = _rows(dur, sym_dur, len(table[1]))
    return sum(1 for s, _, d in run_lengths(ids, table) if np.isneginf(run_score(L, tail, s - 1, d)))


def brute_force(z, table, W, dur, sym_dur, forced=None):
    """Every class string over ALL C classes enumerated (tiny T and C only) -> (ids, the best objective among the legal ones)."""
    o, B, I = _split(table)
    sym, kind = _symbols(table)
    z = np.asarray(z, np.float64)
    W = np.asarray(W, np.float64)
    T, C = z.shape
    P = len(B)
    L, tail = _rows(dur, sym_dur, P)
    Lfull = np.zeros((P + 1, T + 1))            # [symbol][frames]; O and "no run" (0 frames) score 0
    for p in range(P):
        for d in range(1, T + 1):
            Lfull[p + 1, d] = run_score(L, tail, p, d)
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
    ksym = np.array([sym.get(c, 0) for c in range(C)])
    kkind = np.array([kind.get(c, 3) for c in range(C)])
    paths = np.stack(np.meshgrid(*[np.arange(C)] * T, indexing="ij"), -1).reshape(-1, T)
    M = len(paths)
    tot = np.zeros(M)
    cur, rl = np.zeros(M, np.int64), np.zeros(M, np.int64)      # the open run's symbol (0: none) and its frames so far
    prev = np.full(M, C)
    for t in range(T):
        c = paths[:, t]
        tot = tot + z[t, c] + step[prev, c]
        closes = kkind[c] != 2                  # O, B and a never-chosen class close the open run; I continues it
        tot = tot + np.where(closes, Lfull[cur, rl], 0.0)
        opens = kkind[c] == 1
        cur = np.where(opens, ksym[c], np.where(closes, 0, cur))
        rl = np.where(opens, 1, np.where(closes, 0, rl + 1))
        prev = c
    tot = tot + Lfull[cur, np.minimum(rl, T)]
    if forced is not None:
        for t in range(T):
            if forced[t]:
                tot = np.where(paths[:, t] == o, tot, NEG)
    k = int(np.argmax(tot))
    return paths[k].astype(np.int32), float(tot[k])
