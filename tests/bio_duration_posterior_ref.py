"""numpy forward-backward over the explicit-duration BIO grammar of wfl_decode_duration, the restatement of what
wfl_decode_duration_posterior computes (include/wfl_asr.h), for the tests.  Grammar, symbols, virtual start, forced frames, `table`,
`W`, `dur` and `sym_dur` as in bio_duration_ref.

    weight of a legal path = exp(sum_t z[t][c_t] + sum over opened runs W[previous symbol][opened symbol] + sum over phoneme runs L_q(d))
    logZ = log sum over all legal paths
    post[t]     = the posterior that frame t belongs to phoneme p at all, for ids[t] in {B-p, I-p}; that it is O for ids[t] == O
    cls_post[t] = the posterior of the exact class ids[t]: on B-p that a run of p opens exactly there

In the log domain, with W[O][O] taken as 0, everything of frame t - 1 on the right and end(-1) = (0, -inf, ...):
    forward    In_q(t) = lse_s (end_s(t-1) + W[s][q])
               R_q^1(t) = e_t(B-q) + In_q(t);   R_q^j(t) = e_t(I-q) + R_q^{j-1}(t-1)   2 <= j <= D
               Y_q(t) = e_t(I-q) + tail_q + lse(Y_q(t-1), L_q(D) + R_q^D(t-1))
               end_q(t) = lse(lse_j (L_q(j) + R_q^j(t)), Y_q(t));     O(t) = e_t(O) + In_O(t);     logZ = lse_s end_s(T-1)
    backward   bE_q(t): after a run of q has ended at t; Wr_q^j(t): t is the j-th frame of a run; V_q(t): inside the tail.
               At T - 1: bO = bE = V = 0, Wr^j = L(j).   u_t[O] = e_t(O) + bO(t), u_t[q] = e_t(B-q) + Wr_q^1(t);
               (bO, bE)(t-1) = lse_q (W[s][q] + u_t[q]);     V_q(t-1) = lse(bE_q(t-1), e_t(I-q) + tail_q + V_q(t))
               Wr_q^j(t-1) = lse(L_q(j) + bE_q(t-1), e_t(I-q) + Wr_q^{j+1}(t))  j < D;     Wr_q^D(t-1) = L_q(D) + V_q(t-1)
    phoneme p at t: lse(lse_j (R_p^j(t) + Wr_p^j(t)), Y_p(t) + V_p(t)) - logZ;   B-p at t: R_p^1(t) + Wr_p^1(t) - logZ

`dtype=np.float64` is the reference.  `dtype=np.float32` keeps the recurrences in fp32 and subtracts the largest state, history entry
and tail state every `renorm` frames (offsets in float64), as tests/bio_bigram_posterior_ref.py does: its distance from the float64
run on the same inputs is the yardstick for what fp32 rounding costs.  In both, the sums over a frame's terms are formed in float64.
"""
from __future__ import annotations

import numpy as np

from bio_bigram_posterior_ref import _lse_axis
from bio_bigram_ref import _symbols
from bio_duration_ref import _rows, run_score
from bio_posterior_ref import _lae, _lse_all
from bio_viterbi_ref import _split

NEG = -np.inf


def _lse64(*xs):
    v = np.array([float(x) for x in xs], np.float64)
    return float(_lse_all(np.float64, v))


def forward_backward(z, table, W, dur, sym_dur, forced, ids, dtype=np.float64, renorm=16):
    """-> (logz, post [T], cls_post [T]) for the legal path `ids`."""
    dt = dtype
    o, B, I = _split(table)
    sym, kind = _symbols(table)
    z = np.asarray(z, dt)
    T, P = z.shape[0], len(B)
    W = np.array(W, dt).reshape(P + 1, P + 1)
    W[0, 0] = 0                                  # O after O is no opened run
    if T == 0:
        return 0.0, np.zeros(0), np.zeros(0)
    L64, tail64 = _rows(dur, sym_dur, P)
    L, tail = L64.astype(dt), tail64.astype(dt)
    D = L.shape[1]
    forced = np.zeros(T, bool) if forced is None else np.asarray(forced, bool)
    hasI = I >= 0
    Is = np.where(hasI, I, o)
    EO = z[:, o].astype(dt)
    EB = z[:, B].astype(dt).reshape(T, P)
    EI = np.where(hasI[None, :], z[:, Is].reshape(T, P), NEG).astype(dt)
    EB[forced] = NEG
    EI[forced] = NEG
    ps = np.array([sym[int(c)] for c in ids], np.int64)             # the path's symbol per frame
    pk = np.array([kind[int(c)] for c in ids], np.int64)
    aR = np.full((T, D), NEG, dt)               # the path's own symbol: R^1 .. R^D, Y; O's state on an O frame
    aY = np.full(T, NEG, dt)
    aO = np.full(T, NEG, dt)
    off = np.zeros(T, np.float64)
    O = dt(0)
    R = np.full((P, D), NEG, dt)
    Y = np.full(P, NEG, dt)
    end = np.concatenate([[dt(0)], np.full(P, NEG, dt)]).astype(dt)
    c = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(T):
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
            off[t] = c
            if ps[t] == 0:
                aO[t] = O
            else:
                aR[t], aY[t] = R[ps[t] - 1], Y[ps[t] - 1]
        logz = float(_lse_all(np.float64, end.astype(np.float64))) + c
        bO, bE, V = dt(0), np.zeros(P, dt), np.zeros(P, dt)
        Wr = L.copy()
        cb = 0.0
        post, cls = np.zeros(T), np.zeros(T)
        for t in range(T - 1, -1, -1):
            cst = off[t] + cb - logz
            if ps[t] == 0:
                post[t] = cls[t] = np.exp(np.float64(aO[t]) + np.float64(bO) + cst)
            else:
                p = ps[t] - 1
                terms = aR[t].astype(np.float64) + Wr[p].astype(np.float64)
                tail_term = np.float64(aY[t]) + np.float64(V[p])
                first = float(terms[0])
                rest = _lse64(*terms[1:], tail_term)
                post[t] = np.exp(_lse64(first, rest) + cst)
                cls[t] = np.exp((first if pk[t] == 1 else rest) + cst)
            if t == 0:
                break
            u = np.concatenate([[dt(EO[t] + bO)], (EB[t] + Wr[:, 0]).astype(dt)]).astype(dt)
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
    return logz, post, cls


def path_weights(z, table, W, dur, sym_dur, forced=None):
    """Every class string over ALL C classes (tiny T and C only) -> (paths [M, T], log weight [M]; -inf: not a path of the grammar).
    The weight of a legal string is bio_duration_ref.objective's (tests/test_decode_duration_posterior_cpu.py holds the two together);
    the enumeration is vectorised over the strings, as bio_duration_ref.brute_force's."""
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
    return paths, tot


def brute_force(z, table, W, dur, sym_dur, forced, ids):
    """Every class string enumerated -> (logz, post, cls_post) of the legal path `ids`."""
    o, B, I = _split(table)
    sym, kind = _symbols(table)
    paths, tot = path_weights(z, table, W, dur, sym_dur, forced)
    T, C = np.asarray(z).shape
    good = np.isfinite(tot)
    paths, tot = paths[good], tot[good]
    m = tot.max()
    logz = float(m + np.log(np.exp(tot - m).sum()))
    pw = np.exp(tot - logz)
    g = np.zeros((T, C))
    for t in range(T):
        np.add.at(g[t], paths[:, t], pw)
    post, cls = np.zeros(T), np.zeros(T)
    for t, c in enumerate(int(c) for c in ids):
        cls[t] = g[t, c]
        if c == o:
            post[t] = g[t, c]
        else:
            p = sym[c] - 1
            post[t] = g[t, B[p]] + (g[t, I[p]] if I[p] >= 0 else 0.0)
    return logz, post, cls
