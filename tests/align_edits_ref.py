"""numpy restatement of what wfl_align_edits computes (include/wfl_asr.h), for the tests: per transcript token the log likelihood
ratio of every single substitution from a table, and of the token's deletion, against the transcript as written.

    edits[k][p] = logZ(transcript with token k's alternatives replaced by the one pair subs[p]) - logZ(transcript)      p < P
    edits[k][P] = logZ(transcript without token k and without its window) - logZ(transcript)

Built on posterior_ref (its log-add, its renormalisation rule) and viterbi_ref.emissions.  One forward and one backward sweep of the
transcript's own lattice give, per frame t and token k,

    A_k(t) = lse(alpha_{t-1}(G_k), alpha_{t-1}(I_{k-1}), alpha_{t-1}(B_{k-1}))     the mass that may enter token k at t (t = 0 .. T;
                                                                                   at t = 0: 0 for k = 0, -inf otherwise)
    E_k(t) = beta_t(G_{k+1})                                                       the mass that leaves token k after t: G_{k+1} has
                                                                                   exactly the successors of I_k other than I_k itself
    D_k(t) = EB_t(k) + beta_t(B_k)                                                 entering token k at t and everything after

and from those, without touching the rest of the lattice again,

    substitution   r_p(t) = lse(A_k(t) + EB_t(p) [k's window], r_p(t-1) + EI_t(p)),   logZ_p(k) = lse_t(r_p(t) + E_k(t))
    deletion       k < N - 1: lse_t(A_k(t) + D_{k+1}(t));   k = N - 1: A_k(T)

`dtype=np.float64` is the reference.  `dtype=np.float32` keeps the emissions, the sweeps and the r chains in fp32 (renormalised every
`renorm` frames, offsets per frame in float64, the chain carried relative to alpha's offset of its frame) and forms the sums over t
and the differences to logZ in float64, as the kernel does: its distance from float64 is the yardstick of the GPU test.
"""
from __future__ import annotations

import numpy as np

import posterior_ref as P
import viterbi_ref as V

NEG = -np.inf


def _lse64(v, axis=0):
    """float64 log-sum-exp along `axis`; an all -inf column gives -inf."""
    v = np.asarray(v, np.float64)
    m = v.max(axis=axis, keepdims=True)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return (ms + np.log(np.exp(v - ms).sum(axis=axis, keepdims=True))).squeeze(axis)


def window_mask(T, windows, N):
    """[T, N] bool: frame t is inside token k's (lo, hi) start window (None: every frame is)."""
    ok = np.ones((T, N), bool)
    if windows is not None:
        t = np.arange(T)
        for k, (lo, hi) in enumerate(windows):
            ok[:, k] = (t >= lo) & (t <= hi)
    return ok


def edit_scores(z, alternatives, gaps, subs, windows=None, dtype=np.float64, renorm=16):
    """-> dict(logz, edits [N, P + 1] float64), or None when the transcript itself has no path (T < N, T == 0, windows)."""
    dt = dtype
    e, EB, EI, EG = V.emissions(z, alternatives, gaps)
    T, N, Pn = EG.shape[0], len(alternatives), len(subs)
    if T < N or T == 0:
        return None
    win = window_mask(T, windows, N)
    EB = np.where(win, EB, NEG).astype(dt)
    EI, EG = EI.astype(dt), EG.astype(dt)
    sB = e[:, [b for b, _ in subs]].astype(dt) if Pn else np.zeros((T, 0), dt)
    sI = e[:, [i for _, i in subs]].astype(dt) if Pn else np.zeros((T, 0), dt)
    lae = P._lae

    # ---- forward: A [T + 1, N + 1] relative to offA [T + 1]
    A = np.empty((T + 1, N + 1), dt)
    offA = np.zeros(T + 1, np.float64)
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
        A[T], offA[T] = lae(dt, G, P._shift_right(I, dt), P._shift_right(B, dt)), c
        ends = [np.float64(G[N])] + ([np.float64(I[N - 1]), np.float64(B[N - 1])] if N else [])
        logz = float(lae(np.float64, *[np.array([x]) for x in ends])[0]) + c
        if not np.isfinite(logz):
            return None

        # ---- backward: E [T, N] = beta_t(G_{k+1}), D [T, N] = EB_t(k) + beta_t(B_k), relative to offB [T]
        E = np.empty((T, N), dt)
        D = np.empty((T, N), dt)
        offB = np.zeros(T, np.float64)
        bG = np.full(N + 1, NEG, dt)
        bX = np.full(N, NEG, dt)
        bG[N] = 0
        if N:
            bX[N - 1] = 0
        cb = 0.0
        for t in range(T - 1, -1, -1):
            E[t], D[t], offB[t] = bG[1:], (bX + EB[t]).astype(dt), cb
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

        # ---- the edit recursions, all (k, p) at once; r is carried relative to offA[t]
        edits = np.full((N, Pn + 1), NEG, np.float64)
        if N:
            off = (offA[:T] + offB)[:, None]
            if Pn:
                v = np.empty((T, N, Pn), np.float64)
                r = np.full((N, Pn), NEG, dt)
                for t in range(T):
                    d = dt(offA[t] - offA[t - 1]) if t else dt(0)
                    enter = (A[t, :N, None] + np.where(win[t][:, None], sB[t][None, :], dt(NEG))).astype(dt)
                    stay = ((r - d).astype(dt) + sI[t][None, :]).astype(dt)
                    r = lae(dt, enter, stay)
                    v[t] = (r + E[t][:, None]).astype(dt).astype(np.float64) + off[t]
                edits[:, :Pn] = _lse64(v, 0)
            if N > 1:
                edits[:N - 1, Pn] = _lse64((A[:T, :N - 1] + D[:, 1:]).astype(dt).astype(np.float64) + off, 0)
            edits[N - 1, Pn] = float(A[T, N - 1]) + offA[T]
            edits -= logz
    return {"logz": logz, "edits": edits}


def by_definition(z, alternatives, gaps, subs, windows=None, logz_of=None):
    """The definition itself: logZ of every edited transcript by posterior_ref's forward-backward (windows through
    viterbi_window_ref), minus the transcript's own.  -> dict(logz, edits [N, P + 1]) or None."""
    import viterbi_window_ref as W

    def logz(alts, wins):
        if logz_of is not None:
            return logz_of(alts, wins)
        if len(z) < len(alts):
            return NEG
        out = P.forward_backward(z, alts, gaps) if wins is None else W.forward_backward(z, alts, gaps, wins)
        return NEG if out is None else out["logz"]
    N, Pn = len(alternatives), len(subs)
    base = logz(list(alternatives), windows)
    if not np.isfinite(base):
        return None
    edits = np.full((N, Pn + 1), NEG)
    for k in range(N):
        for p, pair in enumerate(subs):
            alts = list(alternatives)
            alts[k] = [tuple(pair)]
            edits[k, p] = logz(alts, windows) - base
        alts = list(alternatives[:k]) + list(alternatives[k + 1:])
        wins = None if windows is None else list(windows[:k]) + list(windows[k + 1:])
        edits[k, Pn] = logz(alts, wins) - base
    return {"logz": base, "edits": edits}
