"""numpy forward-backward over the BIO grammar of wfl_decode_bigram, the restatement of what wfl_decode_bigram_posterior computes
(include/wfl_asr.h), for the tests.  Grammar, symbols, virtual start, forced frames, `table` and `W` as in bio_bigram_ref.

    weight of a legal path = exp(sum_t z[t][c_t] + sum over opened runs W[previous symbol][opened symbol])
    logZ = log sum over all legal paths,      gamma_t(c) = exp(alpha_t(c) + beta_t(c) - logZ)
    post[t]     = gamma_t(B-p) + gamma_t(I-p) for ids[t] in {B-p, I-p},  gamma_t(O) for ids[t] == O
    cls_post[t] = gamma_t(ids[t])

With end[O] = alpha(O), end[p] = log(exp alpha(B-p) + exp alpha(I-p)) and W[O][O] taken as 0 (O after O costs nothing):
    forward    B-q' = e(B-q) + lse_s (end[s] + W[s][q])     O' = e(O) + lse_s (end[s] + W[s][O])     I-q' = e(I-q) + end[q]
    backward   u[O] = e'(O) + beta'(O), u[q] = e'(B-q) + beta'(B-q);  beta(O) = lse_q (W[O][q] + u[q]);
               beta(B-p) = beta(I-p) = log(exp lse_q (W[p][q] + u[q]) + exp(e'(I-p) + beta'(I-p)));  beta at T - 1 = 0

Everything here is in the log domain.  `dtype=np.float64` is the reference.  `dtype=np.float32` keeps the alpha / beta recurrences in
fp32 and subtracts the maximum state every `renorm` frames (offsets in float64), as tests/bio_posterior_ref.py does: its distance from
the float64 run on the same inputs is the yardstick for what fp32 rounding costs.  In both, alpha + beta - logZ is formed in float64.
"""
from __future__ import annotations

import numpy as np

from bio_bigram_ref import _symbols
from bio_posterior_ref import _lae, _lse_all, _outputs
from bio_viterbi_ref import _split

NEG = -np.inf


def _lse_axis(dt, M, axis):
    """log(sum exp M) along an axis in dtype dt; an all -inf line gives -inf."""
    M = np.asarray(M, dt)
    m = M.max(axis=axis)
    ms = np.where(np.isfinite(m), m, dt(0)).astype(dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.exp((M - np.expand_dims(ms, axis)).astype(dt)).astype(dt).sum(axis=axis, dtype=dt)
        return (ms + np.log(s).astype(dt)).astype(dt)


def forward_backward(z, table, W, forced, ids, dtype=np.float64, renorm=16, want_gamma=False):
    """-> (logz, post [T], cls_post [T]) for the legal path `ids`; with want_gamma also (gO [T], gB [T, P], gI [T, P])."""
    dt = dtype
    o, B, I = _split(table)
    z = np.asarray(z, dt)
    T, P = z.shape[0], len(B)
    W = np.array(W, dt).reshape(P + 1, P + 1)
    W[0, 0] = 0                                  # O after O is no opened run
    forced = np.zeros(T, bool) if forced is None else np.asarray(forced, bool)
    if T == 0:
        return (0.0, np.zeros(0), np.zeros(0)) + ((np.zeros(0), np.zeros((0, P)), np.zeros((0, P))) if want_gamma else ())
    hasI = I >= 0
    Is = np.where(hasI, I, o)
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
            both = _lae(dt, Bs, Ii) if P else Bs
            end = np.concatenate([[O], both]).astype(dt)
            into = _lse_axis(dt, (end[:, None] + W).astype(dt), 0)
            nO = dt(EO[t] + into[0])
            nB = (EB[t] + into[1:]).astype(dt)
            nI = (EI[t] + both).astype(dt)
            O, Bs, Ii = nO, nB, nI
            if t % renorm == renorm - 1:
                m = dt(max(float(O), float(Bs.max()) if P else NEG, float(Ii.max()) if P else NEG))
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
            u = np.concatenate([[dt(EO[t] + bO)], (EB[t] + bX).astype(dt)]).astype(dt)
            out = _lse_axis(dt, (W + u[None, :]).astype(dt), 1)
            nX = _lae(dt, out[1:], (EI[t] + bX).astype(dt)) if P else bX
            bO, bX = dt(out[0]), nX
            if t % renorm == 0:
                m = dt(max(float(bO), float(bX.max()) if P else NEG))
                bO, bX = dt(bO - m), (bX - m).astype(dt)
                cb += float(m)
    post, cls = _outputs(gO, gB, gI, ids, table)
    return (logz, post, cls) + ((gO, gB, gI) if want_gamma else ())


def brute_force(z, table, W, forced, ids):
    """Every class string over ALL C classes enumerated (tiny T and C only) -> (logz, post, cls_post) of the legal path `ids`."""
    o, B, I = _split(table)
    sym, kind = _symbols(table)
    z = np.asarray(z, np.float64)
    W = np.asarray(W, np.float64)
    T, C = z.shape
    step = np.full((C + 1, C), NEG)             # [previous class; row C: the virtual O frame][class]: the transition's log weight
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
    good = np.isfinite(tot)
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
