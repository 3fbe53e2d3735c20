"""numpy restatement of what wfl_align_insertions computes (include/wfl_asr.h), for the tests: per place of a transcript the log
likelihood ratio of inserting every phoneme of a table there, against the transcript as written.

    ins[j][p] = logZ(transcript with a token of the one pair subs[p] inserted in front of token j, j = N: behind the last token;
                     the new token without a window, the others with theirs) - logZ(transcript)                      j = 0 .. N

The states G / B / I, alpha / beta, EB / EI and the notation are those of align_edits_ref; the two sweeps are the same and keep

    A_j(t) = lse(alpha_{t-1}(G_j), alpha_{t-1}(I_{j-1}), alpha_{t-1}(B_{j-1}))     the forward step's `in` of slot j, slot N included
    F_j(t) = beta_t(G_j)                                                           what follows a token that ends at t in front of
                                                                                   token j: G_j has exactly the successors it has

and from those, without touching the rest of the lattice again,

    r(t) = lse(A_j(t) + EB_t(p), r(t-1) + EI_t(p)),   ins[j][p] = lse_t(r(t) + F_j(t)) - logZ

`dtype=np.float64` is the reference.  `dtype=np.float32` keeps the emissions, the sweeps and the r chains in fp32 (renormalised every
`renorm` frames, offsets per frame in float64, the chain carried relative to alpha's offset of its frame) and forms the sums over t
and the differences to logZ in float64, as the kernel does: its distance from float64 is the yardstick of the GPU test.
"""
from __future__ import annotations

import numpy as np

import align_edits_ref as E
import posterior_ref as P
import viterbi_ref as V

NEG = -np.inf
OPEN = (0, 2 ** 31 - 1)


def insertion_scores(z, alternatives, gaps, subs, windows=None, dtype=np.float64, renorm=16):
    """-> dict(logz, ins [N + 1, P] float64), or None when the transcript itself has no path (T < N, T == 0, windows)."""
    dt = dtype
    e, EB, EI, EG = V.emissions(z, alternatives, gaps)
    T, N, Pn = EG.shape[0], len(alternatives), len(subs)
    if T < N or T == 0:
        return None
    win = E.window_mask(T, windows, N)
    EB = np.where(win, EB, NEG).astype(dt)
    EI, EG = EI.astype(dt), EG.astype(dt)
    sB = e[:, [b for b, _ in subs]].astype(dt) if Pn else np.zeros((T, 0), dt)
    sI = e[:, [i for _, i in subs]].astype(dt) if Pn else np.zeros((T, 0), dt)
    lae = P._lae

    # ---- forward: A [T, N + 1] relative to offA [T]
    A = np.empty((T, N + 1), dt)
    offA = np.zeros(T, np.float64)
    G = np.full(N + 1, NEG, dt)
    B = np.full(N, NEG, dt)
    I = np.full(N, NEG, dt)
    G[0] = 0
    c = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            inn = lae(dt, G, P._shift_right(I, dt), P._shift_right(B, dt))
            A[t], offA[t] = inn, c
            ii = lae(dt, I, B)
            G = (inn + EG[t]).astype(dt)
            B = (inn[:N] + EB[t]).astype(dt)
            I = (ii + EI[t]).astype(dt)
            if t % renorm == renorm - 1:
                m = max(G.max(), B.max() if N else NEG, I.max() if N else NEG)
                if not np.isfinite(m):
                    m = dt(0)
                G, B, I = (G - m).astype(dt), (B - m).astype(dt), (I - m).astype(dt)
                c += float(m)
        ends = [np.float64(G[N])] + ([np.float64(I[N - 1]), np.float64(B[N - 1])] if N else [])
        logz = float(lae(np.float64, *[np.array([x]) for x in ends])[0]) + c
        if not np.isfinite(logz):
            return None

        # ---- backward: F [T, N + 1] = beta_t(G_j), relative to offB [T]
        F = np.empty((T, N + 1), dt)
        offB = np.zeros(T, np.float64)
        bG = np.full(N + 1, NEG, dt)
        bX = np.full(N, NEG, dt)
        bG[N] = 0
        if N:
            bX[N - 1] = 0
        cb = 0.0
        for t in range(T - 1, -1, -1):
            F[t], offB[t] = bG, cb
            if t == 0:
                break
            xG = (bG + EG[t]).astype(dt)
            xB = (bX + EB[t]).astype(dt)
            xI = (bX + EI[t]).astype(dt)
            nG = lae(dt, xG, np.concatenate([xB, np.full(1, NEG, dt)]).astype(dt))
            nX = lae(dt, xI, xG[1:], np.concatenate([xB[1:], np.full(1, NEG, dt)]).astype(dt)) if N else bX
            bG, bX = nG, nX
            if t % renorm == 0:
                m = max(bG.max(), bX.max() if N else NEG)
                if not np.isfinite(m):
                    m = dt(0)
                bG, bX = (bG - m).astype(dt), (bX - m).astype(dt)
                cb += float(m)

        # ---- the chains, all (j, p) at once; r is carried relative to offA[t]
        ins = np.full((N + 1, Pn), NEG, np.float64)
        if Pn:
            off = offA + offB
            v = np.empty((T, N + 1, Pn), np.float64)
            r = np.full((N + 1, Pn), NEG, dt)
            for t in range(T):
                d = dt(offA[t] - offA[t - 1]) if t else dt(0)
                enter = (A[t][:, None] + sB[t][None, :]).astype(dt)
                stay = ((r - d).astype(dt) + sI[t][None, :]).astype(dt)
                r = lae(dt, enter, stay)
                v[t] = (r + F[t][:, None]).astype(dt).astype(np.float64) + off[t]
            ins = E._lse64(v, 0) - logz
    return {"logz": logz, "ins": ins}


def by_definition(z, alternatives, gaps, subs, windows=None):
    """The definition itself: logZ of every transcript with [subs[p]] inserted at place j, the new token with an open window, by
    posterior_ref's forward-backward (windows through viterbi_window_ref), minus the transcript's own.
    -> dict(logz, ins [N + 1, P]) or None."""
    import viterbi_window_ref as W

    def logz(alts, wins):
        if len(z) < len(alts):
            return NEG
        out = P.forward_backward(z, alts, gaps) if wins is None else W.forward_backward(z, alts, gaps, wins)
        return NEG if out is None else out["logz"]
    N, Pn = len(alternatives), len(subs)
    base = logz(list(alternatives), windows)
    if not np.isfinite(base):
        return None
    ins = np.full((N + 1, Pn), NEG)
    for j in range(N + 1):
        for p, pair in enumerate(subs):
            alts = list(alternatives[:j]) + [[tuple(pair)]] + list(alternatives[j:])
            wins = None if windows is None else list(windows[:j]) + [OPEN] + list(windows[j:])
            ins[j, p] = logz(alts, wins) - base
    return {"logz": base, "ins": ins}
