"""numpy expected successions over the BIO grammar of wfl_decode_bigram, the restatement of what wfl_decode_bigram_counts computes
(include/wfl_asr.h), for the tests.  Grammar, symbols, virtual start, forced frames, `table`, `W` and the recurrences are those of
bio_bigram_posterior_ref.  With end_{-1} = (0, -inf, ...), u_t[O] = e_t(O) + beta_t(O), u_t[q] = e_t(B-q) + beta_t(B-q) (logs):

    counts[s][q] = sum_{t = 0 .. T-1} exp(end_{t-1}[s] + W[s][q] + u_t[q] - logZ)      for (s, q) != (O, O);    counts[O][O] = 0

the expected number of runs of q opened directly after symbol s: every B-q frame, and every O frame whose predecessor is not O.

Everything is in the log domain.  `dtype=np.float64` is the reference.  `dtype=np.float32` keeps the alpha / beta recurrences, each
term's exponent and the running counts in fp32 (renormalised every `renorm` frames, offsets in float64): its distance from the float64
run on the same inputs is the yardstick for what fp32 rounding costs.
"""
from __future__ import annotations

import numpy as np

from bio_bigram_posterior_ref import _lse_axis
from bio_bigram_ref import _symbols
from bio_posterior_ref import _lae, _lse_all
from bio_viterbi_ref import _split

NEG = -np.inf


def expected_counts(z, table, W, forced, dtype=np.float64, renorm=16):
    """-> (logz, counts [P + 1, P + 1] float64; rows the previous symbol)."""
    dt = dtype
    o, B, I = _split(table)
    z = np.asarray(z, dt)
    T, P = z.shape[0], len(B)
    W = np.array(W, dt).reshape(P + 1, P + 1)
    W[0, 0] = 0                                  # O after O is no opened run
    forced = np.zeros(T, bool) if forced is None else np.asarray(forced, bool)
    counts = np.zeros((P + 1, P + 1), dt)
    if T == 0:
        return 0.0, counts.astype(np.float64)
    hasI = I >= 0
    Is = np.where(hasI, I, o)
    EO = z[:, o].astype(dt)
    EB = z[:, B].astype(dt).reshape(T, P)
    EI = np.where(hasI[None, :], z[:, Is].reshape(T, P), NEG).astype(dt)
    EB[forced] = NEG
    EI[forced] = NEG
    ends = np.empty((T, P + 1), dt)              # end_{t-1}, what frame t starts from
    off = np.zeros(T, np.float64)                # ... and its offset
    O, Bs, Ii = dt(0), np.full(P, NEG, dt), np.full(P, NEG, dt)
    c = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            both = _lae(dt, Bs, Ii) if P else Bs
            end = np.concatenate([[O], both]).astype(dt)
            ends[t], off[t] = end, c
            into = _lse_axis(dt, (end[:, None] + W).astype(dt), 0)
            O, Bs, Ii = dt(EO[t] + into[0]), (EB[t] + into[1:]).astype(dt), (EI[t] + both).astype(dt)
            if t % renorm == renorm - 1:
                m = dt(max(float(O), float(Bs.max()) if P else NEG, float(Ii.max()) if P else NEG))
                O, Bs, Ii = dt(O - m), (Bs - m).astype(dt), (Ii - m).astype(dt)
                c += float(m)
        logz = float(_lse_all(np.float64, np.concatenate([[np.float64(O)], Bs.astype(np.float64), Ii.astype(np.float64)]))) + c
        bO, bX = dt(0), np.zeros(P, dt)
        cb = 0.0
        for t in range(T - 1, -1, -1):
            u = np.concatenate([[dt(EO[t] + bO)], (EB[t] + bX).astype(dt)]).astype(dt)
            term = (ends[t][:, None] + W).astype(dt) + u[None, :]
            term = term.astype(dt).astype(np.float64) + (off[t] + cb - logz)
            counts = (counts + np.exp(term).astype(dt)).astype(dt)
            if t == 0:
                break
            out = _lse_axis(dt, (W + u[None, :]).astype(dt), 1)
            nX = _lae(dt, out[1:], (EI[t] + bX).astype(dt)) if P else bX
            bO, bX = dt(out[0]), nX
            if t % renorm == 0:
                m = dt(max(float(bO), float(bX.max()) if P else NEG))
                bO, bX = dt(bO - m), (bX - m).astype(dt)
                cb += float(m)
    counts = counts.astype(np.float64)
    counts[0, 0] = 0.0
    return logz, counts


def brute_force(z, table, W, forced):
    """Every class string over ALL C classes enumerated (tiny T and C only) -> (logz, counts): each legal string's successions,
    weighted by its probability."""
    o, B, I = _split(table)
    sym, kind = _symbols(table)
    z = np.asarray(z, np.float64)
    W = np.asarray(W, np.float64)
    T, C = z.shape
    P = len(B)
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
    sym_of = np.array([sym.get(c, 0) for c in range(C)])
    kind_of = np.array([kind.get(c, 3) for c in range(C)])
    counts = np.zeros((P + 1, P + 1))
    prev = np.zeros(len(paths), np.int64)       # the virtual O frame
    for t in range(T):
        c = paths[:, t]
        opened = (kind_of[c] == 1) | ((kind_of[c] == 0) & (prev != 0))
        np.add.at(counts, (prev[opened], sym_of[c][opened]), pw[opened])
        prev = sym_of[c]
    return logz, counts
