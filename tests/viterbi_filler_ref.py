"""float64 numpy restatement of the forced alignment WITH FILLER TOKENS (wfl_align_filler; include/wfl_asr.h), for the tests.

    states, arcs, start, end and tie order as tests/viterbi_ref.py (G_k = 3k, B_k = 3k + 1, I_k = 3k + 2); fill[k] in {0, 1}, phi >= 0:
    EB_t(k) = EI_t(k) = max over ALL classes of e_t[c] - phi      where fill[k] == 1 (e: the log-posteriors, as every emission there)
    windows (lo, hi) mask EB alone, of a filler like any token's.
    outputs: in a filler's frames tok = k and ids = the frame's first arg-max class over all classes.
"""
from __future__ import annotations

import numpy as np

import viterbi_ref as V

NEG = -np.inf


def _flags(fill, N):
    f = np.zeros(N, bool) if fill is None else np.asarray(fill).astype(bool).reshape(-1)
    assert len(f) == N, "one flag per token"
    return f


def emissions(z, alternatives, gaps, fill=None, phi=1.0, windows=None):
    """-> EB [T, N], EI [T, N], EG [T]: viterbi_ref's, the flagged tokens' columns replaced, EB masked by the windows."""
    e, EB, EI, EG = V.emissions(z, alternatives, gaps)
    T, N = EB.shape
    f = _flags(fill, N)
    if T:
        top = e.max(axis=1) - float(phi)
        EB[:, f] = top[:, None]
        EI[:, f] = top[:, None]
    if windows is not None:
        t = np.arange(T)
        for k, (lo, hi) in enumerate(windows):
            EB[(t < lo) | (t > hi), k] = NEG
    return EB, EI, EG


def legal(states, N):
    return V.legal([int(s) for s in states], N)


def path_score(states, z, alternatives, gaps, fill=None, phi=1.0, windows=None):
    """Sum of the path's emissions (-inf where a token opens outside its window)."""
    EB, EI, EG = emissions(z, alternatives, gaps, fill, phi, windows)
    return float(sum(V.state_emission(int(s), t, EB, EI, EG) for t, s in enumerate(states)))


def all_paths(T, N):
    """Every legal state path of a tiny lattice, by walking the arcs back from the end states."""
    out = []

    def walk(t, tail):
        if t == 0:
            if tail[0] in (0, 1):
                out.append(tuple(tail))
            return
        for p in V.preds(tail[0], N):
            walk(t - 1, [p] + tail)
    if T >= 1:
        for e in ((3 * N, 3 * N - 1, 3 * N - 2) if N else (0,)):
            walk(T - 1, [e])
    return [p for p in out if N or p[0] == 0]


def viterbi(z, alternatives, gaps, fill=None, phi=1.0, windows=None):
    """-> (states [T], score), or (None, 0.0) when the lattice holds no path (T < N, or windows no path meets).  The DP over all
    3N + 1 states, vectorised over states, ties to the first listed predecessor, from a virtual frame -1 in G_0."""
    EB, EI, EG = emissions(z, alternatives, gaps, fill, phi, windows)
    T, N = EG.shape[0], len(alternatives)
    if T < N:
        return None, 0.0
    if T == 0:
        return np.zeros(0, np.int64), 0.0
    G = np.full(N + 1, NEG)
    B = np.full(N, NEG)
    I = np.full(N, NEG)
    G[0] = 0.0
    ag = np.zeros((T, N + 1), np.int8)            # G_k / B_k: 0 G_k, 1 I_{k-1}, 2 B_{k-1}
    ai = np.zeros((T, max(N, 1)), np.int8)        # I_k: 0 I_k, 1 B_k
    for t in range(T):
        cI = np.concatenate([[NEG], I])
        cB = np.concatenate([[NEG], B])
        m = G.copy()
        a = np.zeros(N + 1, np.int8)
        w = cI > m
        m[w], a[w] = cI[w], 1
        w = cB > m
        m[w], a[w] = cB[w], 2
        wi = B > I
        mi = np.where(wi, B, I)
        ag[t] = a
        ai[t, :N] = wi
        G, B, I = m + EG[t], m[:N] + EB[t], mi + EI[t]
    s, score = 3 * N, G[N]
    if N:
        if I[N - 1] > score:
            s, score = 3 * N - 1, I[N - 1]
        if B[N - 1] > score:
            s, score = 3 * N - 2, B[N - 1]
    if score == NEG:
        return None, 0.0
    path = np.empty(T, np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = s
        k, j = divmod(int(s), 3)
        s = s - int(ai[t, k]) if j == 2 else 3 * k - int(ag[t, k])
    return path, float(score)


def outputs(states, z, alternatives, o_id, fill=None):
    """states -> (ids, tok) as wfl_align_filler writes them."""
    ids, tok = V.outputs(states, z, alternatives, o_id)
    f = _flags(fill, len(alternatives))
    for t, k in enumerate(tok):
        if k >= 0 and f[k]:
            ids[t] = int(np.argmax(z[t]))
    return ids, tok


def plant(T, N, C, alternatives, gaps, rng, fill=None, runs=None, margin=8.0, scale=1.0):
    """Random logits with a path planted on its classes -> (z float32, planted states).  runs: per token (gap frames in front, frames
    of the token), laid out from frame 0, the rest of the clip a trailing gap; None: the tokens share the clip evenly with a few
    leading gap frames each (as viterbi_ref.plant).  A frame of a plain token or of a gap has `margin` added to its class.  In a
    filler's frames the planted winner is a class that is neither a gap class nor a class of the two neighbouring tokens, set to
    the largest other logit of the frame + `margin` -- its margin over EVERY other class."""
    f = _flags(fill, N)
    if runs is None:
        bounds = np.linspace(0, T, N + 1).astype(int)
        runs = []
        for a, b in zip(bounds[:-1], bounds[1:]):
            g = min(int(rng.integers(0, max(1, (b - a) // 3))), b - a - 1)
            runs.append((g, b - a - g))
    assert len(runs) == N and sum(g + d for g, d in runs) <= T and all(d >= 1 for _, d in runs)
    states = np.zeros(T, np.int64)
    t = 0
    for k, (g, d) in enumerate(runs):
        states[t:t + g] = 3 * k
        states[t + g] = 3 * k + 1
        states[t + g + 1:t + g + d] = 3 * k + 2
        t += g + d
    states[t:] = 3 * N
    z = rng.standard_normal((T, C)) * scale
    for t, s in enumerate(states):
        k, j = divmod(int(s), 3)
        if j == 0:
            z[t, gaps[0]] += margin
        elif f[k]:
            taken = set(gaps)
            for q in (k - 1, k + 1):
                if 0 <= q < N:
                    taken |= {c for pair in alternatives[q] for c in pair}
            free = [c for c in range(C) if c not in taken]
            w = free[int(rng.integers(0, len(free)))]
            z[t, w] = np.delete(z[t], w).max() + margin
        else:
            b, i = alternatives[k][0]
            z[t, b if j == 1 else i] += margin
    return z.astype(np.float32), states
