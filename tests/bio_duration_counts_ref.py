"""numpy expected run lengths and successions over the explicit-duration BIO grammar of wfl_decode_duration, the restatement of what
wfl_decode_duration_counts computes (include/wfl_asr.h), for the tests.  Grammar, symbols, virtual start, forced frames, `table`, `W`,
`dur`, `sym_dur` and the recurrences (In, R, Y, end, bO, bE, V, Wr, u) are those of bio_duration_posterior_ref.  In logs:

    succ[s][q]        = sum_t exp(end_s(t-1) + W[s][q] + u_t[q] - logZ)                 (s, q) != (O, O);   succ[O][O] = 0
    dur_counts[p][j]  = sum_t exp(R_p^{j+1}(t) + L_p(j+1) + bE_p(t) - logZ)             j = 0 .. D - 2: runs of exactly j + 1 frames
    dur_counts[p][D-1] = sum_t exp(R_p^D(t) + L_p(D) + V_p(t) - logZ)                   runs of D frames or more
    dur_counts[p][D]   = sum_t exp(Y_p(t) + V_p(t) - logZ)                              frames past the D-th

At the last frame bE = V = 0 (logs): a run the clip cuts off counts with its cut length.

`dtype=np.float64` is the reference.  `dtype=np.float32` keeps the recurrences, each term's exponent and the running sums in fp32
(renormalised every `renorm` frames, offsets in float64), as its siblings do: its distance from the float64 run on the same inputs is
the yardstick for what fp32 rounding costs.
"""
from __future__ import annotations

import numpy as np

from bio_bigram_posterior_ref import _lse_axis
from bio_bigram_ref import _symbols
from bio_duration_posterior_ref import path_weights
from bio_duration_ref import _rows
from bio_posterior_ref import _lae, _lse_all
from bio_viterbi_ref import _split

NEG = -np.inf


def expected_counts(z, table, W, dur, sym_dur, forced, dtype=np.float64, renorm=16):
    """-> (logz, succ [P + 1, P + 1] float64, rows the previous symbol; dur_counts [P, D + 1] float64)."""
    dt = dtype
    o, B, I = _split(table)
    z = np.asarray(z, dt)
    T, P = z.shape[0], len(B)
    W = np.array(W, dt).reshape(P + 1, P + 1)
    W[0, 0] = 0                                  # O after O is no opened run
    L64, tail64 = _rows(dur, sym_dur, P)
    L, tail = L64.astype(dt), tail64.astype(dt)
    D = L.shape[1]
    succ = np.zeros((P + 1, P + 1), dt)
    dc = np.zeros((P, D + 1), dt)
    if T == 0:
        return 0.0, succ.astype(np.float64), dc.astype(np.float64)
    forced = np.zeros(T, bool) if forced is None else np.asarray(forced, bool)
    hasI = I >= 0
    Is = np.where(hasI, I, o)
    EO = z[:, o].astype(dt)
    EB = z[:, B].astype(dt).reshape(T, P)
    EI = np.where(hasI[None, :], z[:, Is].reshape(T, P), NEG).astype(dt)
    EB[forced] = NEG
    EI[forced] = NEG
    ends = np.empty((T, P + 1), dt)              # end(t-1), what frame t starts from, and its offset
    offE = np.zeros(T, np.float64)
    aR = np.empty((T, P, D), dt)                 # R^1 .. R^D and Y of frame t, and their offset
    aY = np.empty((T, P), dt)
    offR = np.zeros(T, np.float64)
    O = dt(0)
    R = np.full((P, D), NEG, dt)
    Y = np.full(P, NEG, dt)
    end = np.concatenate([[dt(0)], np.full(P, NEG, dt)]).astype(dt)
    c = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            ends[t], offE[t] = end, c
            into = _lse_axis(dt, (end[:, None] + W).astype(dt), 0)
            Y = ((EI[t] + tail).astype(dt) + _lae(dt, Y, (L[:, D - 1] + R[:, D - 1]).astype(dt))).astype(dt) if P else Y
            Rn = np.empty_like(R)
            Rn[:, 0] = (EB[t] + into[1:]).astype(dt)
            Rn[:, 1:] = (R[:, :-1] + EI[t][:, None]).astype(dt)
            R = Rn
            O = dt(EO[t] + into[0])
            if t % renorm == renorm - 1:
                m = dt(max(float(O), float(R.max()) if P else NEG, float(Y.max()) if P else NEG))
                O, R, Y = dt(O - m), (R - m).astype(dt), (Y - m).astype(dt)
                c += float(m)
            e = _lae(dt, _lse_axis(dt, (R + L).astype(dt), 1), Y) if P else Y
            end = np.concatenate([[O], e]).astype(dt)
            aR[t], aY[t], offR[t] = R, Y, c
        logz = float(_lse_all(np.float64, end.astype(np.float64))) + c
        bO, bE, V = dt(0), np.zeros(P, dt), np.zeros(P, dt)
        Wr = L.copy()
        cb = 0.0

        def add(acc, term, cst):
            term = term.astype(dt).astype(np.float64) + cst
            return (acc + np.exp(term).astype(dt)).astype(dt)

        for t in range(T - 1, -1, -1):
            if P:
                cst = offR[t] + cb - logz
                if D > 1:
                    dc[:, :D - 1] = add(dc[:, :D - 1], (aR[t][:, :D - 1] + L[:, :D - 1]).astype(dt) + bE[:, None], cst)
                dc[:, D - 1] = add(dc[:, D - 1], (aR[t][:, D - 1] + L[:, D - 1]).astype(dt) + V, cst)
                dc[:, D] = add(dc[:, D], aY[t] + V, cst)
            u = np.concatenate([[dt(EO[t] + bO)], (EB[t] + Wr[:, 0]).astype(dt)]).astype(dt)
            succ = add(succ, (ends[t][:, None] + W).astype(dt) + u[None, :], offE[t] + cb - logz)
            if t == 0:
                break
            out = _lse_axis(dt, (W + u[None, :]).astype(dt), 1)
            bO, bE = dt(out[0]), out[1:].astype(dt)
            if P:
                V = _lae(dt, bE, ((EI[t] + tail).astype(dt) + V).astype(dt))
                Wn = np.empty_like(Wr)
                Wn[:, :-1] = _lae(dt, (L[:, :-1] + bE[:, None]).astype(dt), (EI[t][:, None] + Wr[:, 1:]).astype(dt))
                Wn[:, D - 1] = (L[:, D - 1] + V).astype(dt)
                Wr = Wn
            if t % renorm == 0:
                m = dt(max(float(bO), float(bE.max()) if P else NEG, float(V.max()) if P else NEG, float(Wr.max()) if P else NEG))
                bO, bE, V, Wr = dt(bO - m), (bE - m).astype(dt), (V - m).astype(dt), (Wr - m).astype(dt)
                cb += float(m)
    succ = succ.astype(np.float64)
    succ[0, 0] = 0.0
    return logz, succ, dc.astype(np.float64)


def brute_force(z, table, W, dur, sym_dur, forced):
    """Every class string over ALL C classes enumerated (tiny T and C only) -> (logz, succ, dur_counts): each legal string's runs and
    successions counted directly, weighted by its probability."""
    o, B, I = _split(table)
    sym, kind = _symbols(table)
    T, C = np.asarray(z).shape
    P = len(B)
    D = np.asarray(dur).shape[1] - 1
    paths, tot = path_weights(z, table, W, dur, sym_dur, forced)
    good = np.isfinite(tot)
    paths, tot = paths[good], tot[good]
    m = tot.max()
    logz = float(m + np.log(np.exp(tot - m).sum()))
    pw = np.exp(tot - logz)
    sym_of = np.array([sym.get(c, 0) for c in range(C)])
    kind_of = np.array([kind.get(c, 3) for c in range(C)])
    succ = np.zeros((P + 1, P + 1))
    dc = np.zeros((P, D + 1))

    def close(cur, rl, w):
        sel = cur > 0
        np.add.at(dc, (cur[sel] - 1, np.minimum(rl[sel], D) - 1), w[sel])
        np.add.at(dc, (cur[sel] - 1, np.full(int(sel.sum()), D)), w[sel] * np.maximum(rl[sel] - D, 0))

    M = len(paths)
    prev = np.zeros(M, np.int64)                # the virtual O frame
    cur, rl = np.zeros(M, np.int64), np.zeros(M, np.int64)
    for t in range(T):
        c = paths[:, t]
        opened = (kind_of[c] == 1) | ((kind_of[c] == 0) & (prev != 0))
        np.add.at(succ, (prev[opened], sym_of[c][opened]), pw[opened])
        closes = kind_of[c] != 2
        close(np.where(closes, cur, 0), rl, pw)
        opens = kind_of[c] == 1
        cur = np.where(opens, sym_of[c], np.where(closes, 0, cur))
        rl = np.where(opens, 1, np.where(closes, 0, rl + 1))
        prev = sym_of[c]
    close(cur, rl, pw)
    return logz, succ, dc
