"""float64 numpy restatement of the explicit-duration forced alignment that wfl_align_duration_prior computes (include/wfl_asr.h), for
the tests.  A run of d frames of token k (one B frame, d - 1 I frames) with table row r adds

    L_k(d) = table[r][d-1]                               1 <= d <= D
           = table[r][D-1] + (d - D) * table[r][D]       d >  D              (row -1: L = 0)

to the path's score.  Frame by frame, everything of frame t - 1 on the right:

    Ent_k(t) = max(G_k(t-1), X_{k-1}(t-1))        G first on a tie; Ent_0(0) = 0, every other Ent_k(0) = -inf
    G_k(t)   = Ent_k(t) + EG_t
    R_k^1(t) = Ent_k(t) + EB_t(k)                 (EB masked by the windows)
    R_k^j(t) = R_k^{j-1}(t-1) + EI_t(k)
    Y_k(t)   = max(Y_k(t-1), R_k^D(t-1) + L_k(D)) + EI_t(k) + tail_k         Y first on a tie
    X_k(t)   = max(max_j R_k^j(t) + L_k(j), Y_k(t))                          shortest j first, Y last on a tie
    end      = max(G_N(T-1), X_{N-1}(T-1))        G first

States are viterbi_ref's (G_k = 3k, B_k = 3k + 1, I_k = 3k + 2), so viterbi_ref.legal and viterbi_ref.path_score apply to the paths.
"""
from __future__ import annotations

import numpy as np

import viterbi_ref as V
import viterbi_window_ref as W

NEG = -np.inf


def token_priors(rows, table):
    """rows [N] (-1: none), table [n_rows][D + 1] -> (L [N, D], tail [N]) float64."""
    table = np.asarray(table, np.float64)
    D = table.shape[1] - 1
    rows = np.asarray(rows, np.int64).reshape(-1)
    L = np.zeros((len(rows), D))
    tail = np.zeros(len(rows))
    has = rows >= 0
    L[has] = table[rows[has], :D]
    tail[has] = table[rows[has], D]
    return L, tail


def run_prior(d, Lk, tailk):
    """L_k(d) of one token (Lk [D], tailk a float) -- never inf - inf: a tail of -inf counts only where d > D."""
    D = len(Lk)
    if d <= D:
        return float(Lk[d - 1])
    return float(Lk[D - 1]) + (d - D) * float(tailk)


def run_lengths(states, N):
    """Frames each token occupies (its B and I frames) -> [N] ints."""
    s = np.asarray(states, np.int64)
    tokens = s[s % 3 != 0] // 3
    return np.bincount(tokens, minlength=N)[:N]


def _emissions(z, alternatives, gaps, windows):
    _, EB, EI, EG = V.emissions(z, alternatives, gaps)
    if windows is not None:
        EB = W.mask_eb(EB, windows)
    return EB, EI, EG


def path_score(states, z, alternatives, gaps, rows, table, windows=None):
    """The float64 score of a state sequence: its emissions (EB through the windows) plus the prior of its runs."""
    EB, EI, EG = _emissions(z, alternatives, gaps, windows)
    L, tail = token_priors(rows, table)
    total = float(sum(V.state_emission(int(s), t, EB, EI, EG) for t, s in enumerate(states)))
    for k, d in enumerate(run_lengths(states, len(alternatives))):
        total += run_prior(int(d), L[k], tail[k])
    return total


def viterbi(z, alternatives, gaps, rows, table, windows=None):
    """-> (states [T], score, run lengths [N]), or None when no path has a finite score."""
    EB, EI, EG = _emissions(z, alternatives, gaps, windows)
    T, N = EG.shape[0], len(alternatives)
    if T < N or T == 0:
        return None
    L, tail = token_priors(rows, table)
    D = L.shape[1]
    G = np.full(N + 1, NEG)
    X = np.full(N, NEG)
    Y = np.full(N, NEG)
    R = np.full((D, N), NEG)                       # R[j - 1] = R^j
    ae = np.zeros((T, N + 1), bool)                # Ent_k: False G_k, True X_{k-1}
    ay = np.zeros((T, max(N, 1)), bool)            # Y_k: False stay, True entered
    dw = np.zeros((T, max(N, 1)), np.int64)        # X_k's duration, D + 1: Y
    with np.errstate(invalid="ignore"):
        for t in range(T):
            if t == 0:
                ent = np.full(N + 1, NEG)
                ent[0] = 0.0
            else:
                left = np.concatenate([[NEG], X])
                ent = G.copy()
                w = left > ent
                ent[w] = left[w]
                ae[t] = w
            G = ent + EG[t]
            yc = R[D - 1] + L[:, D - 1]
            w = yc > Y
            ay[t, :N] = w
            Y = np.where(w, yc, Y) + EI[t] + tail
            Rn = np.empty_like(R)
            Rn[0] = ent[:N] + EB[t]
            Rn[1:] = R[:-1] + EI[t]
            R = Rn
            X = R[0] + L[:, 0]
            d = np.ones(N, np.int64)
            for j in range(1, D):
                cand = R[j] + L[:, j]
                w = cand > X
                X = np.where(w, cand, X)
                d[w] = j + 1
            w = Y > X
            X = np.where(w, Y, X)
            d[w] = D + 1
            dw[t, :N] = d
    score, k, cnt = G[N], N, -2                    # the walker of the kernel: cnt -2 gap, -1 tail, 0 a run's last frame, j >= 1 the rest
    if N and X[N - 1] > score:
        score, k, cnt = X[N - 1], N - 1, 0
    if not np.isfinite(score):
        return None
    states = np.empty(T, np.int64)
    for t in range(T - 1, -1, -1):
        if cnt == -2:
            states[t] = 3 * k
            if ae[t, k]:
                k, cnt = k - 1, 0
            continue
        if cnt == 0:
            cnt = -1 if dw[t, k] > D else int(dw[t, k])
        if cnt == -1:
            states[t] = 3 * k + 2
            if ay[t, k]:
                cnt = D
            continue
        if cnt > 1:
            states[t] = 3 * k + 2
            cnt -= 1
            continue
        states[t] = 3 * k + 1
        if ae[t, k]:
            k, cnt = k - 1, 0
        else:
            cnt = -2
    return states, float(score), run_lengths(states, N)


def segmentations(T, N):
    """Every (start, length) per token with the runs in order inside T frames (tiny T and N only) -> lists of N (start, length)."""
    def rec(k, first):
        if k == N:
            yield []
            return
        for s in range(first, T):
            for d in range(1, T - s + 1):
                for rest in rec(k + 1, s + d):
                    yield [(s, d)] + rest
    return rec(0, 0)


def states_of(seg, T):
    states = np.zeros(T, np.int64)
    prev = 0
    for k, (s, d) in enumerate(seg):
        states[prev:s] = 3 * k
        states[s] = 3 * k + 1
        states[s + 1:s + d] = 3 * k + 2
        prev = s + d
    states[prev:] = 3 * len(seg)
    return states


def brute_force(z, alternatives, gaps, rows, table, windows=None):
    """-> the best score over every segmentation, or None when none is finite."""
    T, N = len(z), len(alternatives)
    best = None
    for seg in segmentations(T, N):
        if windows is not None and any(not (lo <= s <= hi) for (s, _), (lo, hi) in zip(seg, windows)):
            continue
        sc = path_score(states_of(seg, T), z, alternatives, gaps, rows, table)
        if np.isfinite(sc) and (best is None or sc > best):
            best = sc
    return best
