"""numpy restatement of wfl_align_duration_prior_counts (include/wfl_asr.h): the posterior distribution of every token's run length over
the explicit-duration lattice of wfl_align_duration_prior, for the tests.  Emissions, prior and sweeps are those of
tests/duration_prior_posterior_ref.py (its header has the recurrences); the backward sweep carries one more quantity per token,

    Q_k^e(t)   = EI_{t+1}(k) + .. + EI_e(k) + bE_{k+1}(e)         e = t .. t + D - 2
    Q_k^t(t)   = bE_{k+1}(t),      Q_k^e(t-1) = EI_t(k) + Q_k^e(t)

and the row of token k, in the layout of a table row, is

    dur_post[k][d-1] = P(d_k = d)          = sum_t exp(aR_k^1(t) + L_k(d) + Q_k^{t+d-1}(t) - logZ)        1 <= d < D
    dur_post[k][D-1] = P(d_k >= D)         = sum_t exp(aR_k^D(t) + L_k(D) + V_k(t) - logZ)
    dur_post[k][D]   = E[max(d_k - D, 0)]  = sum_t exp(aY_k(t) + V_k(t) - logZ)

(frame t as the D-th frame of a run: once per run of D frames or more; frame t inside the tail: once per frame past the D-th).

`dtype=np.float64` is the reference.  `dtype=np.float32` keeps emissions, table and recurrences in fp32 and renormalises as the kernel
does -- alpha every `renorm` frames by the maximum over G, X, Y and the ring, beta by the maximum over bE, V, the W ring and the Q
ring, offsets in float64: its distance from float64 on the same inputs is the yardstick for what fp32 costs.  In both, alpha + beta -
logZ and the sums over the frames are formed in float64.

enumerate_lengths sums P(d_k = d) over every segmentation of a tiny lattice (viterbi_duration_prior_ref.segmentations).
"""
from __future__ import annotations

import numpy as np

import duration_prior_posterior_ref as PR
import viterbi_duration_prior_ref as VD
import viterbi_ref as V
import viterbi_window_ref as W
from posterior_ref import NEG, _lae

_max = PR._max


def expected_counts(z, alternatives, gaps, rows, table, windows=None, dtype=np.float64, renorm=16):
    """-> dict(logz, dur_post [N, D + 1] float64), or None when the lattice holds no path of finite weight."""
    dt = dtype
    _, EB, EI, EG = V.emissions(z, alternatives, gaps)
    if windows is not None:
        EB = W.mask_eb(EB, windows)
    EB, EI, EG = EB.astype(dt), EI.astype(dt), EG.astype(dt)
    T, N = EG.shape[0], len(alternatives)
    if T == 0 or T < N:
        return None
    L, tail = VD.token_priors(rows, table)
    L, tail = L.astype(dt), tail.astype(dt)
    D = L.shape[1]
    f8 = np.float64

    A_R1 = np.empty((T, N))                       # alpha on its true scale, float64: what was held in dt, plus the offset
    A_RD = np.empty((T, N))
    A_Y = np.empty((T, N))
    G = np.full(N + 1, NEG, dt)
    X = np.full(N, NEG, dt)
    Y = np.full(N, NEG, dt)
    R = np.full((D, N), NEG, dt)                  # R[j - 1] = aR^j
    G[0] = 0
    c = 0.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for t in range(T):
            ent = _lae(dt, G, np.concatenate([np.full(1, NEG, dt), X]).astype(dt))
            G = (ent + EG[t]).astype(dt)
            Y = ((_lae(dt, Y, (R[D - 1] + L[:, D - 1]).astype(dt)) + EI[t]).astype(dt) + tail).astype(dt)
            Rn = np.empty_like(R)
            Rn[0] = (ent[:N] + EB[t]).astype(dt)
            Rn[1:] = (R[:-1] + EI[t]).astype(dt)
            R = Rn
            X = _lae(dt, *[(R[j] + L[:, j]).astype(dt) for j in range(D)], Y) if N else X
            if N:
                A_R1[t] = R[0].astype(f8) + c     # (as the kernel: aR^1 on the scale of before the frame's renormalisation)
            if t % renorm == renorm - 1:
                m = _max(G, X, Y, R)
                if not np.isfinite(m):
                    m = 0.0
                m = dt(m)
                G, X, Y, R = (G - m).astype(dt), (X - m).astype(dt), (Y - m).astype(dt), (R - m).astype(dt)
                c += float(m)
            if N:
                A_RD[t] = R[D - 1].astype(f8) + c
                A_Y[t] = Y.astype(f8) + c
        ends = [np.array([f8(G[N])])] + ([np.array([f8(X[N - 1])])] if N else [])
        if not np.isfinite(max(float(e[0]) for e in ends)):
            return None
        logz = float(_lae(f8, *ends)[0]) + c

        post = np.zeros((N, D + 1))
        bE = np.full(N + 1, NEG, dt)
        bE[N] = 0
        Vv = np.full(N, NEG, dt)
        Wv = np.full((D, N), NEG, dt)             # Wv[j - 1] = W^j
        Qv = np.full((max(D - 1, 0), N), NEG, dt)  # Qv[i] = Q^{t + i}(t)
        ep = np.zeros(N, dt)
        cb = 0.0
        for t in range(T - 1, -1, -1):
            nE = bE[1:]
            Vv = _lae(dt, nE, ((ep + tail).astype(dt) + Vv).astype(dt))
            Wn = np.empty_like(Wv)
            for j in range(1, D):
                Wn[j - 1] = _lae(dt, (L[:, j - 1] + nE).astype(dt), (ep + Wv[j]).astype(dt))
            Wn[D - 1] = (L[:, D - 1] + Vv).astype(dt)
            Wv = Wn
            if D > 1:
                Qn = np.empty_like(Qv)
                Qn[0] = nE
                Qn[1:] = (ep + Qv[:-1]).astype(dt)
                Qv = Qn
            cst = cb - logz
            for d in range(1, D):
                post[:, d - 1] += np.exp(A_R1[t] + (L[:, d - 1] + Qv[d - 1]).astype(dt).astype(f8) + cst)
            post[:, D - 1] += np.exp(A_RD[t] + (L[:, D - 1] + Vv).astype(dt).astype(f8) + cst)
            post[:, D] += np.exp(A_Y[t] + Vv.astype(f8) + cst)
            if t == 0:
                break
            nb = np.empty_like(bE)
            nb[:N] = _lae(dt, (bE[:N] + EG[t]).astype(dt), (EB[t] + Wv[0]).astype(dt))
            nb[N] = bE[N] + EG[t]
            bE = nb.astype(dt)
            ep = EI[t]
            if t % renorm == 0:
                m = _max(bE, Vv, Wv, Qv)
                if not np.isfinite(m):
                    m = 0.0
                m = dt(m)
                bE, Vv, Wv, Qv = (bE - m).astype(dt), (Vv - m).astype(dt), (Wv - m).astype(dt), (Qv - m).astype(dt)
                cb += float(m)
    return {"logz": logz, "dur_post": post}


def three(z, alternatives, gaps, rows, table, windows=None, dtype=np.float64, renorm=16):
    """The entry's three outputs for one clip -> (logz, dur_post, status): status 1 and zeros where the lattice holds no path."""
    r = expected_counts(z, alternatives, gaps, rows, table, windows, dtype, renorm)
    if r is None:
        return 0.0, np.zeros((len(alternatives), np.asarray(table).shape[1])), 1
    return r["logz"], r["dur_post"], 0


def expected_length(dur_post):
    """E[d_k] of every row: sum_d d P(d) + D P(>= D) + the excess."""
    dur_post = np.asarray(dur_post, np.float64)
    D = dur_post.shape[1] - 1
    return dur_post[:, :D] @ np.arange(1, D + 1, dtype=np.float64) + dur_post[:, D]


def enumerate_lengths(z, alternatives, gaps, rows, table, windows=None):
    """Every segmentation of a tiny lattice -> dict(logz, dur_post [N, D + 1], n_paths), or None without a path of finite weight."""
    T, N = len(z), len(alternatives)
    D = np.asarray(table).shape[1] - 1
    segs, logw = [], []
    for seg in VD.segmentations(T, N):
        w = VD.path_score(VD.states_of(seg, T), z, alternatives, gaps, rows, table, windows)
        if np.isfinite(w):
            segs.append(seg)
            logw.append(w)
    if not segs:
        return None
    logw = np.array(logw)
    m = logw.max()
    logz = float(m + np.log(np.exp(logw - m).sum()))
    p = np.exp(logw - logz)
    post = np.zeros((N, D + 1))
    for w, seg in zip(p, segs):
        for k, (_, d) in enumerate(seg):
            if d < D:
                post[k, d - 1] += w
            else:
                post[k, D - 1] += w
                post[k, D] += w * (d - D)
    return {"logz": logz, "dur_post": post, "n_paths": len(segs)}
