"""float64 numpy restatement of the forced alignment WITH MINIMUM DURATIONS (wfl_align_min_duration; include/wfl_asr.h), for the tests.

    token k occupies at least D_k frames: a run is frame 1 in B_k, frames 2 .. D_k - 1 in the chain states H_k^2 .. H_k^{D_k-1} (which
    emit EI and are written as I_k), every later frame in I_k; the token is left from I_k alone, from B_k as well where D_k == 1

`viterbi` is the DP over those expanded states (ties as viterbi_ref.viterbi: the first listed predecessor, I_k before its chain); the
paths it returns are in the three-state numbering of viterbi_ref (a chain frame is 3k + 2).  The enumeration checks the run lengths on
the state sequences themselves: viterbi_window_ref.accepted_paths, filtered.
"""
from __future__ import annotations

import numpy as np

import viterbi_ref as V
import viterbi_window_ref as W

NEG = -np.inf
MAX_MIN_FRAMES = 8
CHAIN = MAX_MIN_FRAMES - 2


def viterbi(z, alternatives, gaps, min_frames, windows=None):
    """-> (states [T], score), or (None, 0.0) when no path meets the durations (and the windows, when given)."""
    _, EB, EI, EG = V.emissions(z, alternatives, gaps)
    if windows is not None:
        EB = W.mask_eb(EB, windows)
    T, N = EG.shape[0], len(alternatives)
    d = np.asarray(min_frames, np.int64).reshape(N)
    assert ((d >= 1) & (d <= MAX_MIN_FRAMES)).all()
    if T < N or T == 0:
        return None, 0.0
    G = np.full(N + 1, NEG)
    B = np.full(N, NEG)
    I = np.full(N, NEG)
    H = np.full((N, CHAIN), NEG)                  # H[:, j] = H^{j + 2}
    G[0] = EG[0]
    if N:
        B[0] = EB[0, 0]
    ag = np.zeros((T, N + 1), np.int8)            # G_k / B_k: 0 G_k, 1 I_{k-1}, 2 B_{k-1}
    ai = np.zeros((T, max(N, 1)), np.int8)        # I_k: 0 I_k, 1 X_k (the chain's last state, B_k for D_k <= 2)
    rows = np.arange(N)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            cI = np.concatenate([[NEG], I])
            cB = np.concatenate([[NEG], np.where(d > 1, NEG, B)])
            m = G.copy()
            a = np.zeros(N + 1, np.int8)
            w = cI > m
            m[w], a[w] = cI[w], 1
            w = cB > m
            m[w], a[w] = cB[w], 2
            X = np.where(d <= 2, B, H[rows, np.maximum(d - 3, 0)]) if N else B
            wi = X > I
            mi = np.where(wi, X, I)
            ag[t] = a
            ai[t, :N] = wi
            nH = np.full((N, CHAIN), NEG)
            for j in range(CHAIN):
                src = B if j == 0 else H[:, j - 1]
                nH[:, j] = np.where(j + 3 <= d, src + EI[t], NEG)
            H = nH
            G = m + EG[t]
            B = m[:N] + EB[t]
            I = mi + EI[t]
    s, score = 3 * N, G[N]
    if N:
        if I[N - 1] > score:
            s, score = 3 * N - 1, I[N - 1]
        if d[N - 1] == 1 and B[N - 1] > score:
            s, score = 3 * N - 2, B[N - 1]
    if not np.isfinite(score):
        return None, 0.0
    path = np.empty(T, np.int64)
    t = T - 1
    while t >= 0:
        path[t] = s
        if t == 0:
            break
        k, j = divmod(s, 3)
        if j == 2 and ai[t, k] and d[k] >= 3:     # entered through the chain: D_k - 2 chain frames, then B_k
            for _ in range(int(d[k]) - 2):
                t -= 1
                path[t] = s
            s -= 1
        else:
            s = s - int(ai[t, k]) if j == 2 else 3 * k - int(ag[t, k])
        t -= 1
    return path, float(score)


def run_lengths(states, N):
    """Frames each token occupies (its B and I frames) -> [N] ints."""
    out = np.zeros(N, np.int64)
    for s in states:
        k, j = divmod(int(s), 3)
        if j:
            out[k] += 1
    return out


def accepted_paths(T, N, windows, min_frames):
    """viterbi_window_ref.accepted_paths whose every run has at least D_k frames (tiny T and N only)."""
    d = np.asarray(min_frames, np.int64).reshape(N)
    return [p for p in W.accepted_paths(T, N, windows) if (run_lengths(p, N) >= d).all()]


def brute_force(z, alternatives, gaps, windows, min_frames):
    """-> (best score or None, number of accepted paths), by enumeration on the unmasked emissions."""
    _, EB, EI, EG = V.emissions(z, alternatives, gaps)
    paths = accepted_paths(len(z), len(alternatives), windows, min_frames)
    if not paths:
        return None, 0
    w = [sum(V.state_emission(int(s), t, EB, EI, EG) for t, s in enumerate(p)) for p in paths]
    return float(max(w)), len(paths)
