"""float64 numpy restatement of the forced alignment WITH OPTIONAL TOKENS (wfl_align_optional; include/wfl_asr.h), for the tests.

    states, emissions, tie order as tests/viterbi_ref.py (G_k = 3k, B_k = 3k + 1, I_k = 3k + 2), opt[k] in {0, 1}, lam >= 0:
    B_k <- {G_k, I_{k-1}, B_{k-1}, G_{k-1} - lam, I_{k-2} - lam, B_{k-2} - lam}     the last three only where opt[k-1] == 1
    G_k <- {G_k, I_{k-1}, B_{k-1}},  I_k <- {I_k, B_k}                              unchanged (the first listed wins an exact tie)
    start: a virtual frame -1 in G_0 with score 0 (so frame 0 is G_0 | B_0, and B_1 at -lam where opt[0] == 1)
    end:   G_N | I_{N-1} | B_{N-1}, and where opt[N-1] == 1  | G_{N-1} - lam | I_{N-2} - lam | B_{N-2} - lam
    windows (lo, hi) mask EB alone; a skipped token's window is never consulted.
"""
from __future__ import annotations

import numpy as np

import viterbi_ref as V

NEG = -np.inf


def _flags(opt, N):
    o = np.zeros(N, bool) if opt is None else np.asarray(opt).astype(bool).reshape(-1)
    assert len(o) == N, "one flag per token"
    return o


def min_frames_needed(opt):
    """N - sum over the maximal runs of optional tokens of ceil(len / 2), at least 1."""
    need, run = len(opt), 0
    for f in list(opt) + [0]:
        if f:
            run += 1
        else:
            need -= (run + 1) // 2
            run = 0
    return max(need, 1)


def preds(s, N, opt):
    k, j = divmod(int(s), 3)
    if j == 2:
        return [s, s - 1]
    p = [3 * k, 3 * k - 1, 3 * k - 2]
    if j == 1 and k >= 1 and opt[k - 1]:
        p += [3 * k - 3, 3 * k - 4, 3 * k - 5]
    return [q for q in p if q >= 0]


def start_states(N, opt):
    return [0] + ([1] if N else []) + ([4] if N >= 2 and opt[0] else [])


def end_states(N, opt):
    """In the order of preference."""
    e = [3 * N] + ([3 * N - 1, 3 * N - 2] if N else [])
    if N and opt[N - 1]:
        e += [q for q in (3 * N - 3, 3 * N - 4, 3 * N - 5) if q >= 0]
    return e


def legal(states, N, opt):
    opt = _flags(opt, N)
    T = len(states)
    if T == 0:
        return N == 0
    if int(states[0]) not in start_states(N, opt) or int(states[-1]) not in end_states(N, opt):
        return False
    return all(int(states[t - 1]) in preds(states[t], N, opt) for t in range(1, T))


def tokens_of(states):
    """The tokens a path visits, in order (its `tok` without the gaps and the repeats)."""
    out = []
    for s in states:
        k, j = divmod(int(s), 3)
        if j and (not out or out[-1] != k):
            out.append(k)
    return out


def skipped_of(states, N):
    sk = np.ones(N, np.int32)
    sk[tokens_of(states)] = 0
    return sk


def path_score(states, z, alternatives, gaps, lam=0.0):
    """Sum of the path's emissions minus lam per skipped token."""
    return V.path_score(states, z, alternatives, gaps) - lam * int(skipped_of(states, len(alternatives)).sum())


def all_paths(T, N, opt):
    """Every legal state path of a tiny lattice, by walking the arcs back from the end states."""
    opt = _flags(opt, N)
    starts = set(start_states(N, opt))
    out = []

    def walk(t, tail):
        if t == 0:
            if tail[0] in starts:
                out.append(tuple(tail))
            return
        for p in preds(tail[0], N, opt):
            walk(t - 1, [p] + tail)
    if T >= 1:
        for e in end_states(N, opt):
            walk(T - 1, [e])
    return out


def viterbi(z, alternatives, gaps, opt=None, lam=0.0, windows=None):
    """-> (states [T], score), or (None, 0.0) when the lattice holds no path.  The DP over all 3N + 1 states, vectorised over
    states, ties to the first listed predecessor.  score = sum of the emissions - lam * skipped tokens."""
    _, EB, EI, EG = V.emissions(z, alternatives, gaps)
    T, N = EG.shape[0], len(alternatives)
    opt = _flags(opt, N)
    if T == 0:
        return (np.zeros(0, np.int64), 0.0) if N == 0 else (None, 0.0)
    if windows is not None:
        EB = EB.copy()
        for k, (lo, hi) in enumerate(windows):
            t = np.arange(T)
            EB[(t < lo) | (t > hi), k] = NEG
    may = np.concatenate([[False], opt[:N - 1]]) if N else np.zeros(0, bool)     # B_k has skip arcs: opt[k-1]
    G = np.full(N + 1, NEG)
    B = np.full(N, NEG)
    I = np.full(N, NEG)
    G[0] = 0.0                                     # the virtual frame -1
    ag = np.zeros((T, N + 1), np.int8)            # G_k: 0 G_k, 1 I_{k-1}, 2 B_{k-1}
    ab = np.zeros((T, max(N, 1)), np.int8)        # B_k: those, 3 G_{k-1}, 4 I_{k-2}, 5 B_{k-2}
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
        mb, b = m[:N].copy(), a[:N].copy()
        if N:
            for code, src in ((3, np.concatenate([[NEG], G[:N - 1]])), (4, np.concatenate([[NEG, NEG], I])[:N]),
                              (5, np.concatenate([[NEG, NEG], B])[:N])):
                w = may & (src - lam > mb)
                mb[w], b[w] = (src - lam)[w], code
        wi = B > I
        mi = np.where(wi, B, I)
        ag[t] = a
        ab[t, :N] = b
        ai[t, :N] = wi
        G, B, I = m + EG[t], mb + EB[t], mi + EI[t]
    vals = {3 * k + j: v for k in range(N) for j, v in ((0, G[k]), (1, B[k]), (2, I[k]))}
    vals[3 * N] = G[N]
    s, score = None, NEG
    for e in end_states(N, opt):
        v = vals[e] - (lam if e < 3 * N - 2 else 0.0)
        if s is None or v > score:
            s, score = e, v
    if score == NEG:
        return None, 0.0
    path = np.empty(T, np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = s
        k, j = divmod(s, 3)
        s = s - int(ai[t, k]) if j == 2 else 3 * k - int(ab[t, k] if j == 1 else ag[t, k])
    return path, float(score)


def outputs(states, z, alternatives, o_id):
    """states -> (ids, tok, skipped) as wfl_align_optional writes them."""
    ids, tok = V.outputs(states, z, alternatives, o_id)
    return ids, tok, skipped_of(states, len(alternatives))


def plant(T, N, C, alternatives, gaps, rng, skipped=(), runs=None, margin=8.0, scale=1.0):
    """Random logits with a path planted by `margin` on its classes -> (z float32, planted states).  skipped: the tokens the path
    leaves out.  runs: per KEPT token (gap frames in front, frames of the token), laid out from frame 0, the rest of the clip a
    trailing gap; None: the kept tokens share the clip evenly with a few leading gap frames each (as viterbi_ref.plant).  A gap
    frame behind the kept token k is in G_{k+1} -- in front of a skipped token the path waits in that token's own gap state."""
    skipped = set(int(k) for k in skipped)
    kept = [k for k in range(N) if k not in skipped]
    if runs is None:
        bounds = np.linspace(0, T, len(kept) + 1).astype(int)
        runs = []
        for a, b in zip(bounds[:-1], bounds[1:]):
            g = min(int(rng.integers(0, max(1, (b - a) // 3))), b - a - 1)
            runs.append((g, b - a - g))
    assert len(runs) == len(kept) and sum(g + d for g, d in runs) <= T and all(d >= 1 for _, d in runs)
    states = np.zeros(T, np.int64)
    t, gap_state = 0, 0
    for k, (g, d) in zip(kept, runs):
        states[t:t + g] = gap_state
        states[t + g] = 3 * k + 1
        states[t + g + 1:t + g + d] = 3 * k + 2
        t += g + d
        gap_state = 3 * (k + 1)
    states[t:] = gap_state
    z = rng.standard_normal((T, C)) * scale
    for t, s in enumerate(states):
        k, j = divmod(int(s), 3)
        if j == 0:
            z[t, gaps[0]] += margin
        else:
            b, i = alternatives[k][0]
            z[t, b if j == 1 else i] += margin
    return z.astype(np.float32), states
