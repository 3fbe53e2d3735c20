"""float64 numpy restatement of the forced alignment that wfl_align computes (include/wfl_asr.h), for the tests.

    states G_0, B_0, I_0, ..., B_{N-1}, I_{N-1}, G_N   (G_k = 3k, B_k = 3k + 1, I_k = 3k + 2)
    G_k <- {G_k, I_{k-1}, B_{k-1}},  B_k <- {G_k, I_{k-1}, B_{k-1}},  I_k <- {I_k, B_k}   (first listed wins an exact tie)
    start G_0 | B_0, end G_N | I_{N-1} | B_{N-1}
"""
from __future__ import annotations

import itertools

import numpy as np

NEG = -np.inf


def log_softmax(z):
    z = np.asarray(z, np.float64)
    m = z.max(axis=1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))


def emissions(z, alternatives, gaps):
    """-> EB [T, N], EI [T, N], EG [T] (float64 log-posteriors)."""
    e = log_softmax(z)
    T = e.shape[0]
    N = len(alternatives)
    EB = np.full((T, N), NEG)
    EI = np.full((T, N), NEG)
    for k, alts in enumerate(alternatives):
        EB[:, k] = np.max(np.stack([e[:, b] for b, _ in alts], 1), 1)
        EI[:, k] = np.max(np.stack([e[:, i] for _, i in alts], 1), 1)
    EG = np.max(np.stack([e[:, g] for g in gaps], 1), 1)
    return e, EB, EI, EG


def preds(s, N):
    k, j = divmod(s, 3)
    if j == 2:
        return [s, s - 1]
    return [p for p in (3 * k, 3 * k - 1, 3 * k - 2) if p >= 0]


def state_emission(s, t, EB, EI, EG):
    k, j = divmod(s, 3)
    return EG[t] if j == 0 else (EB[t, k] if j == 1 else EI[t, k])


def viterbi(z, alternatives, gaps):
    """-> (states [T] or None when T < N, score).  The DP over all 3N + 1 states (vectorised over states), ties to the first
    listed predecessor."""
    _, EB, EI, EG = emissions(z, alternatives, gaps)
    T, N = EG.shape[0], len(alternatives)
    if T < N:
        return None, 0.0
    G = np.full(N + 1, NEG)
    B = np.full(N, NEG)
    I = np.full(N, NEG)
    G[0] = EG[0]
    if N:
        B[0] = EB[0, 0]
    ag = np.zeros((T, N + 1), np.int8)            # G_k / B_k: 0 G_k, 1 I_{k-1}, 2 B_{k-1}
    ai = np.zeros((T, max(N, 1)), np.int8)        # I_k: 0 I_k, 1 B_k
    for t in range(1, T):
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
        G = m + EG[t]
        B = m[:N] + EB[t]
        I = mi + EI[t]
    s, score = 3 * N, G[N]
    if N:
        if I[N - 1] > score:
            s, score = 3 * N - 1, I[N - 1]
        if B[N - 1] > score:
            s, score = 3 * N - 2, B[N - 1]
    path = np.empty(T, np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = s
        if t == 0:
            break
        k, j = divmod(s, 3)
        s = s - int(ai[t, k]) if j == 2 else 3 * k - int(ag[t, k])
    return path, float(score)


def path_score(states, z, alternatives, gaps):
    _, EB, EI, EG = emissions(z, alternatives, gaps)
    return float(sum(state_emission(int(s), t, EB, EI, EG) for t, s in enumerate(states)))


def legal(states, N):
    T = len(states)
    if T == 0:
        return N == 0
    if states[0] not in (0, 1):
        return False
    if states[-1] not in ((3 * N, 3 * N - 1, 3 * N - 2) if N else (0,)):
        return False
    for t in range(1, T):
        if states[t - 1] not in preds(int(states[t]), N):
            return False
    return True


def brute_force(z, alternatives, gaps):
    """Every legal path enumerated (tiny T and N only) -> (best states, best score) with the DP's tie order: among equal scores the
    path whose predecessor choices come first, walking back from the preferred end state."""
    T, N = len(z), len(alternatives)
    S = 3 * N + 1
    best, best_path = None, None
    for states in itertools.product(range(S), repeat=T):
        if not legal(states, N):
            continue
        sc = path_score(states, z, alternatives, gaps)
        if best is None or sc > best + 1e-12:
            best, best_path = sc, states
    return (np.array(best_path) if best_path is not None else None), best


def outputs(states, z, alternatives, o_id):
    """states -> (ids, tok) as wfl_align writes them."""
    ids, tok = [], []
    for t, s in enumerate(states):
        k, j = divmod(int(s), 3)
        if j == 0:
            ids.append(o_id)
            tok.append(-1)
            continue
        cols = [a[0] if j == 1 else a[1] for a in alternatives[k]]
        vals = [z[t][c] for c in cols]
        ids.append(cols[int(np.argmax(vals))])
        tok.append(k)
    return np.array(ids, np.int32), np.array(tok, np.int32)


def plant(T, N, C, alternatives, gaps, rng, margin=8.0, scale=1.0):
    """Random logits with a path planted by `margin` on its classes: (z, planted states).  The planted path then beats every path
    that differs from it by far more than 1e-2."""
    z = rng.standard_normal((T, C)) * scale
    # a legal path: token k gets the frames of its share of the clip, a few leading gap frames, then B, then I
    states = np.zeros(T, np.int64)
    if T == N:
        states[:] = 3 * np.arange(N) + 1
    else:
        bounds = np.linspace(0, T, N + 1).astype(int)
        for k in range(N):
            a, b = bounds[k], bounds[k + 1]
            g = rng.integers(0, max(1, (b - a) // 3))            # leading gap frames of this token's span
            g = min(g, b - a - 1)
            states[a:a + g] = 3 * k
            states[a + g] = 3 * k + 1
            states[a + g + 1:b] = 3 * k + 2
    for t, s in enumerate(states):
        k, j = divmod(int(s), 3)
        if j == 0:
            z[t, gaps[0]] += margin
        else:
            b, i = alternatives[k][0]
            z[t, b if j == 1 else i] += margin
    return z.astype(np.float32), states
