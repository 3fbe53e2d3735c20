"""float64 numpy restatement of the BIO-grammar Viterbi decode that wfl_decode computes (include/wfl_asr.h), for the tests.

States are the classes: O, B-p, I-p of the table's phonemes; every other class is never chosen.  A legal path has every I-p directly
preceded by B-p or I-p; the clip starts after a virtual O frame.  The path maximises sum_t z[t][c_t] - lambda * (runs opened): a run
is opened by every B-p frame and by every O frame whose predecessor is not O.  With d the previous frame's scores, a = argmax d (the
lowest class id wins a tie), best = d[a]:
    O   : z + (d[O] >= best - lambda ? d[O] : best - lambda)        B-p : z + best - lambda
    I-p : z + (d[I-p] >= d[B-p] ? d[I-p] : d[B-p])                  end: argmax of the last frame, lowest id on a tie
`table` is (o_id, [(B class, I class or -1), ...]) throughout; `forced` a bool per frame (such a frame can only be O).
"""
from __future__ import annotations

import numpy as np

NEG = -np.inf


def _split(table):
    o, pairs = table
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    return int(o), pairs[:, 0], pairs[:, 1]


def prepass(z, threshold, dtype=np.float64):
    """-> (lse [T], forced [T] bool, max probability [T]) in `dtype` arithmetic (float32: what the kernel's pre-pass computes)."""
    z = np.asarray(z, dtype)
    if z.shape[0] == 0:
        return np.zeros(0, dtype), np.zeros(0, bool), np.zeros(0, dtype)
    m = z.max(axis=1)
    se = np.exp(z - m[:, None]).sum(axis=1, dtype=dtype)
    pmax = (dtype(1) / se).astype(dtype)
    forced = (pmax < dtype(threshold)) if threshold > 0 else np.zeros(len(z), bool)
    return (m + np.log(se)).astype(dtype), forced, pmax


def viterbi(z, table, lam, forced=None, dtype=np.float64):
    """-> (ids [T] int32, objective).  dtype=np.float32 restates the kernel's arithmetic: fp32 state scores, `best` subtracted every
    16 frames and carried in a double."""
    o, B, I = _split(table)
    z = np.asarray(z, dtype)
    T, P = z.shape[0], len(B)
    if T == 0:
        return np.zeros(0, np.int32), 0.0
    f32 = dtype == np.float32
    hasI = I >= 0
    Is = np.where(hasI, I, o)
    cls = np.concatenate([[o], B, I[hasI]])
    lam = dtype(lam)
    dO, dB, dI = dtype(0), np.full(P, NEG, dtype), np.full(P, NEG, dtype)
    A = np.zeros(T, np.int64)
    OB = np.zeros(T, bool)
    IB = np.zeros((T, P), bool)
    acc = 0.0
    forced = np.zeros(T, bool) if forced is None else np.asarray(forced, bool)

    def argbest():
        vals = np.concatenate([[dO], dB, dI[hasI]])
        best = vals.max()
        return best, int(cls[vals == best].min())

    for t in range(T):
        best, a = argbest()
        if f32 and t and t % 16 == 0:
            acc += float(best)
            dO, dB, dI = dtype(dO - best), dB - best, dI - best
            best = dtype(0)
        sw = dtype(best - lam)
        ob = not (dO >= sw)
        ib = ~(dI >= dB)
        eB = z[t, B].copy()
        eI = np.where(hasI, z[t, Is], NEG).astype(dtype)
        if forced[t]:
            eB[:] = NEG
            eI[:] = NEG
        dI = (np.where(ib, dB, dI) + eI).astype(dtype)
        dB = (sw + eB).astype(dtype)
        dO = dtype(z[t, o] + (sw if ob else dO))
        A[t], OB[t], IB[t] = a, ob, ib
    best, s = argbest()
    pair_of = {int(b): (p, 1) for p, b in enumerate(B)}
    pair_of.update({int(i): (p, 2) for p, i in enumerate(I) if i >= 0})
    ids = np.empty(T, np.int32)
    for t in range(T - 1, -1, -1):
        ids[t] = s
        if s == o:
            s = int(A[t]) if OB[t] else o
        else:
            p, kind = pair_of[s]
            s = int(A[t]) if kind == 1 else (int(B[p]) if IB[t, p] else s)
    return ids, float(best) + acc


def legal(ids, table):
    o, B, I = _split(table)
    b_of_i = {int(i): int(b) for b, i in zip(B, I) if i >= 0}
    bs = set(int(b) for b in B)
    prev = o
    for c in (int(c) for c in ids):
        if c == o or c in bs:
            pass
        elif c in b_of_i:
            if prev != c and prev != b_of_i[c]:
                return False
        else:
            return False                        # a class that is never chosen
        prev = c
    return True


def objective(ids, z, table, lam, forced=None):
    """float64 objective of a path (legal or not): the logits on it minus lambda per opened run; -inf when a forced frame is not O."""
    o, B, _ = _split(table)
    z = np.asarray(z, np.float64)
    bs = set(int(b) for b in B)
    tot, prev = 0.0, o
    for t, c in enumerate(int(c) for c in ids):
        if forced is not None and forced[t] and c != o:
            return NEG
        tot += z[t, c]
        if c in bs or (c == o and prev != o):
            tot -= lam
        prev = c
    return float(tot)


def score(ids, z, table, lam, forced=None):
    """What wfl_decode reports: the objective minus the frames' log-sum-exp (float64)."""
    return objective(ids, z, table, lam, forced) - float(prepass(z, 0.0)[0].sum())


def brute_force(z, table, lam, forced=None):
    """Every class string over ALL C classes enumerated (tiny T and C only) -> the best objective among the legal ones."""
    o, B, I = _split(table)
    z = np.asarray(z, np.float64)
    T, C = z.shape
    ok = np.zeros((C, C), bool)                 # ok[prev, cur]
    opens = np.zeros((C, C))
    ok[:, o] = True
    opens[:, o] = 1.0
    opens[o, o] = 0.0
    for b, i in zip(B, I):
        ok[:, b] = True
        opens[:, b] = 1.0
        if i >= 0:
            ok[b, i] = ok[i, i] = True
    paths = np.stack(np.meshgrid(*[np.arange(C)] * T, indexing="ij"), -1).reshape(-1, T)
    good = ok[o, paths[:, 0]]
    tot = z[0, paths[:, 0]] - lam * opens[o, paths[:, 0]]
    for t in range(1, T):
        good &= ok[paths[:, t - 1], paths[:, t]]
        tot = tot + z[t, paths[:, t]] - lam * opens[paths[:, t - 1], paths[:, t]]
    if forced is not None:
        for t in range(T):
            if forced[t]:
                good &= paths[:, t] == o
    tot = np.where(good, tot, NEG)
    k = int(np.argmax(tot))
    return paths[k].astype(np.int32), float(tot[k])


def plant(T, C, table, rng, margin=12.0, scale=1.0, min_run=5, max_run=25):
    """Random logits with a legal path planted by `margin` on its classes: (z float32, planted ids).  Runs of min_run..max_run frames:
    O, or a phoneme (B-p then I-p; a phoneme without I-p gets one frame), never O after O."""
    o, B, I = _split(table)
    z = rng.standard_normal((T, C)) * scale
    ids = np.empty(T, np.int32)
    t, prev_o = 0, False
    while t < T:
        n = int(rng.integers(min_run, max_run + 1))
        if not prev_o and rng.random() < 0.25:
            ids[t:t + n] = o
            prev_o = True
        else:
            p = int(rng.integers(len(B)))
            if I[p] < 0:
                n = 1
            ids[t] = B[p]
            ids[t + 1:t + n] = I[p]
            prev_o = False
        t += n
    z[np.arange(T), ids] += margin
    return z.astype(np.float32), ids
