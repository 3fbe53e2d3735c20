"""float64 numpy restatement of the forced alignment of a transcript GRAPH that wfl_align_graph computes (include/wfl_asr.h), for the
tests.  Modelled on tests/viterbi_ref.py, whose emissions it shares.

    N slots in topological order; slot k has predecessors pred(k) (START = -1 or earlier slots) and a final flag
    states G_k = 3k, B_k = 3k + 1, I_k = 3k + 2, G_end = 3N
    m_k(t)   = max{ G_k, then for p in pred(k) in list order: I_p, B_p } of frame t - 1       (first listed wins an exact tie)
    G_k(t)   = m_k(t) + EG_t     B_k(t) = m_k(t) + EB_t(k)     I_k(t) = max{I_k, B_k}(t - 1) + EI_t(k)
    G_end(t) = max{ G_end, then for final f in slot order: I_f, B_f }(t - 1) + EG_t
    start: frame 0 is G_k or B_k of a slot that lists START (G_end when N == 0); end: G_end | I_f | B_f over the finals, in that order
"""
from __future__ import annotations

import itertools

import numpy as np

import viterbi_ref as V

NEG = -np.inf
START, UNUSED = -1, -2
MAXP = 8


def pred_table(preds):
    """lists -> [N, 8] int64, unused entries -2"""
    P = np.full((len(preds), MAXP), UNUSED, np.int64)
    for k, row in enumerate(preds):
        P[k, :len(row)] = row
    return P


def viterbi(z, alternatives, preds, final, gaps):
    """-> (states [T] or None when no path fits, score).  Vectorised over the slots; ties to the first listed candidate."""
    _, EB, EI, EG = V.emissions(z, alternatives, gaps)
    T, N = EG.shape[0], len(alternatives)
    if T == 0:
        return (np.zeros(0, np.int64), 0.0) if N == 0 else (None, 0.0)
    P = pred_table(preds)
    fin = np.nonzero(np.asarray(final, np.int64))[0]
    lists_start = (P == START).any(axis=1) if N else np.zeros(0, bool)
    G = np.where(lists_start, EG[0], NEG)
    B = np.where(lists_start, EB[0], NEG) if N else np.zeros(0)
    I = np.full(N, NEG)
    Ge = EG[0] if N == 0 else NEG
    cm = np.zeros((T, N), np.int8)         # G_k / B_k: 0 G_k, j + 1 the j-th listed predecessor
    ci = np.zeros((T, N), np.int8)         # I_k: 0 I_k, 1 B_k
    xb = np.zeros((T, N), np.int8)         # the predecessor's exit was B (else I: I wins a tie)
    ce = np.zeros(T, np.int64)             # G_end: 0 G_end, f + 1 the final slot f
    xb[0] = B > I
    safe = np.maximum(P, 0)
    for t in range(1, T):
        wx = B > I
        X = np.where(wx, B, I)
        m = G.copy()
        a = np.zeros(N, np.int8)
        for j in range(MAXP):
            if not (P[:, j] >= 0).any():
                continue
            val = np.where(P[:, j] >= 0, X[safe[:, j]], NEG)
            w = val > m
            m[w], a[w] = val[w], j + 1
        me, ae = Ge, 0
        if len(fin):
            f = int(np.argmax(X[fin]))                  # the first maximum: the lowest slot
            if X[fin][f] > me:
                me, ae = X[fin][f], int(fin[f]) + 1
        mi = np.where(wx, B, I)
        cm[t], ci[t], ce[t] = a, wx, ae
        G = m + EG[t]
        B = m + EB[t]
        I = mi + EI[t]
        Ge = me + EG[t]
        xb[t] = B > I
    s, score = 3 * N, Ge
    if len(fin):
        X = np.where(B > I, B, I)
        f = int(np.argmax(X[fin]))
        if X[fin][f] > score:
            k = int(fin[f])
            s, score = 3 * k + (1 if B[k] > I[k] else 2), X[fin][f]
    if score == NEG:
        return None, 0.0
    path = np.empty(T, np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = s
        if t == 0:
            break
        k, j = divmod(int(s), 3)
        p = -1
        if k == N:
            if ce[t]:
                p = int(ce[t]) - 1
        elif j == 2:
            s -= int(ci[t, k])
        elif cm[t, k] == 0:
            s = 3 * k
        else:
            p = int(P[k, cm[t, k] - 1])
        if p >= 0:
            s = 3 * p + (1 if xb[t - 1, p] else 2)
    return path, float(score)


def state_preds(s, preds, final):
    """The states a path may be in at the frame before state s."""
    N = len(preds)
    k, j = divmod(int(s), 3)
    if k == N:
        return [3 * N] + [3 * f + q for f in range(N) if final[f] for q in (2, 1)]
    if j == 2:
        return [s, s - 1]
    return [3 * k] + [3 * p + q for p in preds[k] if p >= 0 for q in (2, 1)]


def legal(states, preds, final):
    T, N = len(states), len(preds)
    if T == 0:
        return N == 0
    k, j = divmod(int(states[0]), 3)
    if N == 0:
        if states[0] != 0:
            return False
    elif k >= N or j == 2 or START not in preds[k]:
        return False
    k, j = divmod(int(states[-1]), 3)
    if not (k == N or (j != 0 and final[k])):
        return False
    return all(states[t - 1] in state_preds(states[t], preds, final) for t in range(1, T))


def path_score(states, z, alternatives, gaps):
    _, EB, EI, EG = V.emissions(z, alternatives, gaps)
    return float(sum(V.state_emission(int(s), t, EB, EI, EG) for t, s in enumerate(states)))


def outputs(states, z, alternatives, o_id):
    """states -> (ids, tok, taken) as wfl_align_graph writes them."""
    N = len(alternatives)
    ids, tok = V.outputs([s if s < 3 * N else 0 for s in states], z, alternatives, o_id) if len(states) else (np.zeros(0, np.int32),) * 2
    taken = np.zeros(N, np.int32)
    taken[tok[tok >= 0]] = 1
    return ids, tok, taken


def plant(T, seq, C, alternatives, gaps, rng, margin=8.0, scale=1.0):
    """Random logits with a path planted through the slots `seq` (a way through the graph, in order): viterbi_ref.plant of that
    sequence as a chain, its states mapped back to the graph's -> (z, planted states)."""
    z, st = V.plant(T, len(seq), C, [alternatives[k] for k in seq], gaps, rng, margin, scale)
    seq = np.asarray(list(seq) + [len(alternatives)], np.int64)          # (a chain's G_N would be G_end; plant never uses it)
    return z, 3 * seq[st // 3] + st % 3


def expansions(elements):
    """parse_variants' elements -> every expansion of the transcript, as lists of tokens, the first variants' first."""
    choices = [[(el,)] if isinstance(el, str) else list(el) for el in elements]
    return [[t for part in combo for t in part] for combo in itertools.product(*choices)]
