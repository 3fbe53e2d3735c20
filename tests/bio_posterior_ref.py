"""numpy forward-backward over the BIO grammar of wfl_decode, the restatement of what wfl_decode_posterior computes (include/wfl_asr.h),
for the tests.  Grammar, virtual start, forced frames and `table` as in bio_viterbi_ref.

    weight of a legal path = exp(sum_t z[t][c_t] - lambda * runs opened)     (a run is opened by every B-p frame and by every O frame
                                                                              whose predecessor is not O)
    logZ = log sum over all legal paths,      gamma_t(c) = exp(alpha_t(c) + beta_t(c) - logZ)
    post[t]     = gamma_t(B-p) + gamma_t(I-p) for ids[t] in {B-p, I-p},  gamma_t(O) for ids[t] == O
    cls_post[t] = gamma_t(ids[t])

Everything here is in the log domain.  `dtype=np.float64` is the reference.  `dtype=np.float32` keeps the alpha / beta recurrences in
fp32 and subtracts the maximum state every `renorm` frames (offsets in float64), as tests/posterior_ref.py does for the alignment
lattice: its distance from the float64 run on the same inputs is the yardstick for what fp32 rounding costs.  In both, alpha + beta -
logZ is formed in float64.
"""
from __future__ import annotations

import numpy as np

from bio_viterbi_ref import _split

NEG = -np.inf


def _lae(dt, *xs):
    """log(sum exp x) elementwise in dtype dt, m + log(sum exp(x - m)); -inf in, -inf out."""
    xs = [np.asarray(x, dt) for x in xs]
    m = xs[0]
    for x in xs[1:]:
        m = np.maximum(m, x)
    ms = np.where(np.isfinite(m), m, dt(0)).astype(dt)
    s = np.zeros_like(ms)
    with np.errstate(invalid="ignore"):
        for x in xs:
            s = (s + np.exp((x - ms).astype(dt)).astype(dt)).astype(dt)
    with np.errstate(divide="ignore"):
        return (ms + np.log(s).astype(dt)).astype(dt)


def _lse_all(dt, v):
    """log(sum exp v) of a vector -> scalar of dtype dt (-inf for an empty or all -inf vector)."""
    v = np.asarray(v, dt)
    if v.size == 0:
        return dt(NEG)
    m = v.max()
    if not np.isfinite(m):
        return dt(NEG)
    return dt(m + np.log(np.exp((v - m).astype(dt)).astype(dt).sum(dtype=dt)))


def path_is_legal(ids, table, forced=None):
    """A class per frame that the grammar accepts: only classes of the table, every I-p directly after B-p or I-p (the clip follows a
    virtual O frame), and O on every forced frame."""
    o, B, I = _split(table)
    b_of_i = {int(i): int(b) for b, i in zip(B, I) if i >= 0}
    bs = set(int(b) for b in B)
    prev = o
    for t, c in enumerate(int(c) for c in ids):
        if forced is not None and forced[t] and c != o:
            return False
        if c == o or c in bs:
            pass
        elif c in b_of_i:
            if prev != c and prev != b_of_i[c]:
                return False
        else:
            return False
        prev = c
    return True


def _outputs(gO, gB, gI, ids, table):
    o, B, I = _split(table)
    pair_of = {int(b): (p, 1) for p, b in enumerate(B)}
    pair_of.update({int(i): (p, 2) for p, i in enumerate(I) if i >= 0})
    T = len(ids)
    post, cls = np.zeros(T), np.zeros(T)
    for t, c in enumerate(int(c) for c in ids):
        if c == o:
            post[t] = cls[t] = gO[t]
        else:
            p, kind = pair_of[c]
            post[t] = gB[t, p] + gI[t, p]
            cls[t] = gB[t, p] if kind == 1 else gI[t, p]
    return post, cls


def forward_backward(z, table, lam, forced, ids, dtype=np.float64, renorm=16, want_gamma=False):
    """-> (logz, post [T], cls_post [T]) for the legal path `ids`; with want_gamma also (gO [T], gB [T, P], gI [T, P])."""
    dt = dtype
    o, B, I = _split(table)
    z = np.asarray(z, dt)
    T, P = z.shape[0], len(B)
    forced = np.zeros(T, bool) if forced is None else np.asarray(forced, bool)
    if T == 0:
        return (0.0, np.zeros(0), np.zeros(0)) + ((np.zeros(0), np.zeros((0, P)), np.zeros((0, P))) if want_gamma else ())
    hasI = I >= 0
    Is = np.where(hasI, I, o)
    lam = dt(lam)
    EO = z[:, o].astype(dt)
    EB = z[:, B].astype(dt).reshape(T, P)
    EI = np.where(hasI[None, :], z[:, Is].reshape(T, P), NEG).astype(dt)
    EB[forced] = NEG
    EI[forced] = NEG
    aO = np.empty(T, dt)
    aB = np.empty((T, P), dt)
    aI = np.empty((T, P), dt)
    off = np.zeros(T, np.float64)
    O, Bs, Ii = dt(0), np.full(P, NEG, dt), np.full(P, NEG, dt)
    c = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            rest = _lse_all(dt, np.concatenate([Bs, Ii]))
            nO = dt(EO[t] + _lae(dt, O, dt(rest - lam)))
            nB = (EB[t] + dt(_lae(dt, O, rest) - lam)).astype(dt)
            nI = (EI[t] + _lae(dt, Ii, Bs)).astype(dt)
            O, Bs, Ii = nO, nB, nI
            if t % renorm == renorm - 1:
                m = max(float(O), float(Bs.max()) if P else NEG, float(Ii.max()) if P else NEG)
                m = dt(m)
                O, Bs, Ii = dt(O - m), (Bs - m).astype(dt), (Ii - m).astype(dt)
                c += float(m)
            aO[t], aB[t], aI[t], off[t] = O, Bs, Ii, c
        logz = float(_lse_all(np.float64, np.concatenate([[np.float64(O)], Bs.astype(np.float64), Ii.astype(np.float64)]))) + c
        bO, bX = dt(0), np.zeros(P, dt)
        cb = 0.0
        gO = np.zeros(T)
        gB = np.zeros((T, P))
        gI = np.zeros((T, P))
        for t in range(T - 1, -1, -1):
            cst = off[t] + cb - logz
            gO[t] = np.exp(np.float64(aO[t]) + np.float64(bO) + cst)
            gB[t] = np.exp(aB[t].astype(np.float64) + bX.astype(np.float64) + cst)
            gI[t] = np.exp(aI[t].astype(np.float64) + bX.astype(np.float64) + cst)
            if t == 0:
                break
            SB = _lse_all(dt, (EB[t] + bX).astype(dt))
            wO = dt(EO[t] + bO)
            nO = dt(_lae(dt, wO, dt(SB - lam)))
            nX = _lae(dt, np.full(P, dt(_lae(dt, wO, SB) - lam), dt), (EI[t] + bX).astype(dt)) if P else bX
            bO, bX = nO, nX
            if t % renorm == 0:
                m = dt(max(float(bO), float(bX.max()) if P else NEG))
                bO, bX = dt(bO - m), (bX - m).astype(dt)
                cb += float(m)
    post, cls = _outputs(gO, gB, gI, ids, table)
    return (logz, post, cls) + ((gO, gB, gI) if want_gamma else ())


def brute_force(z, table, lam, forced, ids):
    """Every class string over ALL C classes enumerated (tiny T and C only) -> (logz, post, cls_post) of the legal path `ids`."""
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
    paths, tot = paths[good], tot[good]
    m = tot.max()
    logz = float(m + np.log(np.exp(tot - m).sum()))
    pw = np.exp(tot - logz)
    g = np.zeros((T, C))
    for t in range(T):
        np.add.at(g[t], paths[:, t], pw)
    P = len(B)
    gB = g[:, B].reshape(T, P)
    gI = np.where((I >= 0)[None, :], g[:, np.where(I >= 0, I, o)].reshape(T, P), 0.0)
    post, cls = _outputs(g[:, o], gB, gI, ids, table)
    return logz, post, cls
