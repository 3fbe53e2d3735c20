"""numpy forward-backward over the forced-alignment lattice, the restatement of what wfl_align_posterior computes (include/wfl_asr.h),
for the tests.  Built on viterbi_ref.emissions; lattice and transitions as in viterbi_ref.

    weight of a path = exp(sum_t e_t(state_t)),  logZ = log sum over all accepted paths,  gamma_t(s) = exp(alpha_t(s) + beta_t(s) - logZ)

`dtype=np.float64` is the reference.  `dtype=np.float32` keeps the emissions and the alpha / beta recurrences in fp32, in the log
domain, and subtracts the maximum state every `renorm` frames (offsets in float64) as the kernel does: its distance from the float64
run on the same inputs is the yardstick for what fp32 rounding costs.  In both, alpha + beta - logZ and the per-token sums are formed
in float64.
"""
from __future__ import annotations

import itertools

import numpy as np

import viterbi_ref as V

NEG = -np.inf


def _lae(dt, *xs):
    """log(sum exp x) elementwise in dtype dt, m + log(sum exp(x - m)); -inf in, -inf out."""
    m = xs[0]
    for x in xs[1:]:
        m = np.maximum(m, x)
    ms = np.where(np.isfinite(m), m, dt(0)).astype(dt)
    s = np.zeros_like(ms)
    for x in xs:
        s = (s + np.exp((x - ms).astype(dt)).astype(dt)).astype(dt)
    with np.errstate(divide="ignore"):
        return (ms + np.log(s).astype(dt)).astype(dt)


def _shift_right(x, dt):
    return np.concatenate([np.full(1, NEG, dt), x]).astype(dt)


def forward_backward(z, alternatives, gaps, tok=None, dtype=np.float64, renorm=16, want_gamma=False):
    """-> dict: logz, and with `tok` (wfl_align's per-frame token index, -1 in gaps) tok_post / start_mean / start_sd [N]; with
    want_gamma gG [T, N + 1], gB [T, N], gI [T, N].  None when T < N (infeasible)."""
    dt = dtype
    _, EB, EI, EG = V.emissions(z, alternatives, gaps)
    EB, EI, EG = EB.astype(dt), EI.astype(dt), EG.astype(dt)
    T, N = EG.shape[0], len(alternatives)
    if T < N or T == 0:
        return None
    aG = np.empty((T, N + 1), dt)
    aB = np.empty((T, N), dt)
    aI = np.empty((T, N), dt)
    off = np.zeros(T, np.float64)
    G = np.full(N + 1, NEG, dt)
    B = np.full(N, NEG, dt)
    I = np.full(N, NEG, dt)
    G[0] = 0                                          # a virtual frame -1 in G_0
    c = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            inn = _lae(dt, G, _shift_right(I, dt), _shift_right(B, dt))
            ii = _lae(dt, I, B)
            G = (inn + EG[t]).astype(dt)
            B = (inn[:N] + EB[t]).astype(dt)
            I = (ii + EI[t]).astype(dt)
            if t % renorm == renorm - 1:
                m = max(G.max(), B.max() if N else NEG, I.max() if N else NEG)
                if not np.isfinite(m):
                    m = dt(0)
                G, B, I = (G - m).astype(dt), (B - m).astype(dt), (I - m).astype(dt)
                c += float(m)
            aG[t], aB[t], aI[t], off[t] = G, B, I, c
        ends = [np.float64(G[N])] + ([np.float64(I[N - 1]), np.float64(B[N - 1])] if N else [])
        logz = float(_lae(np.float64, *[np.array([e]) for e in ends])[0]) + c
        # backward: beta(B_k) = beta(I_k) (the same successors)
        bG = np.full(N + 1, NEG, dt)
        bX = np.full(N, NEG, dt)
        bG[N] = 0
        if N:
            bX[N - 1] = 0
        cb = 0.0
        out = {"logz": logz}
        if want_gamma:
            out["gG"], out["gB"], out["gI"] = np.zeros((T, N + 1)), np.zeros((T, N)), np.zeros((T, N))
        if tok is not None:
            tok = np.asarray(tok)
            first = np.array([int(np.nonzero(tok == k)[0][0]) for k in range(N)], np.int64)
            cnt = np.array([int((tok == k).sum()) for k in range(N)], np.float64)
            occ, m0, m1, m2 = (np.zeros(N) for _ in range(4))
        for t in range(T - 1, -1, -1):
            cst = off[t] + cb - logz
            gB = np.exp(aB[t].astype(np.float64) + bX.astype(np.float64) + cst)
            gI = np.exp(aI[t].astype(np.float64) + bX.astype(np.float64) + cst)
            if want_gamma:
                out["gG"][t] = np.exp(aG[t].astype(np.float64) + bG.astype(np.float64) + cst)
                out["gB"][t], out["gI"][t] = gB, gI
            if tok is not None:
                d = (t - first).astype(np.float64)
                m0 += gB
                m1 += gB * d
                m2 += gB * d * d
                k = int(tok[t])
                if k >= 0:
                    occ[k] += gB[k] + gI[k]
            if t == 0:
                break
            xG = (bG + EG[t]).astype(dt)
            xB = (bX + EB[t]).astype(dt)
            xI = (bX + EI[t]).astype(dt)
            nG = _lae(dt, xG, np.concatenate([xB, np.full(1, NEG, dt)]).astype(dt))
            nX = _lae(dt, xI, xG[1:], np.concatenate([xB[1:], np.full(1, NEG, dt)]).astype(dt)) if N else bX
            bG, bX = nG, nX
            if t % renorm == 0:
                m = max(bG.max(), bX.max() if N else NEG)
                if not np.isfinite(m):
                    m = dt(0)
                bG, bX = (bG - m).astype(dt), (bX - m).astype(dt)
                cb += float(m)
    if tok is not None:
        mean = m1 / m0
        out["tok_post"] = occ / cnt
        out["start_mean"] = mean
        out["start_sd"] = np.sqrt(np.maximum(m2 / m0 - mean * mean, 0.0))
        out["sum_gamma_b"] = m0
    return out


def path_score(z, alternatives, gaps, tok):
    """float64 score (sum of e_t) of the path that wfl_align's `tok` describes: a gap frame is in G, the first frame of a token's run
    in B_k (a path enters a token through B_k and visits it once), the run's other frames in I_k."""
    _, EB, EI, EG = V.emissions(z, alternatives, gaps)
    tok = np.asarray(tok, np.int64)
    t = np.arange(len(tok))
    k = np.maximum(tok, 0)
    first = np.concatenate([[True], tok[1:] != tok[:-1]])
    if not len(alternatives):
        return float(EG.sum())
    return float(np.where(tok < 0, EG, np.where(first, EB[t, k], EI[t, k])).sum())


def brute_force(z, alternatives, gaps, tok=None):
    """Every accepted path enumerated (tiny T and N only): the same dict as forward_backward(want_gamma=True)."""
    _, EB, EI, EG = V.emissions(z, alternatives, gaps)
    T, N = len(z), len(alternatives)
    S = 3 * N + 1
    paths, logw = [], []
    for states in itertools.product(range(S), repeat=T):
        if V.legal(states, N):
            paths.append(states)
            logw.append(sum(V.state_emission(int(s), t, EB, EI, EG) for t, s in enumerate(states)))
    logw = np.array(logw)
    m = logw.max()
    logz = float(m + np.log(np.exp(logw - m).sum()))
    p = np.exp(logw - logz)
    g = np.zeros((T, S))
    for w, states in zip(p, paths):
        for t, s in enumerate(states):
            g[t, s] += w
    out = {"logz": logz, "gG": g[:, 0::3], "gB": g[:, 1::3], "gI": g[:, 2::3], "n_paths": len(paths)}
    if tok is not None:
        tok = np.asarray(tok)
        tp, mu, sd = np.zeros(N), np.zeros(N), np.zeros(N)
        for k in range(N):
            fr = np.nonzero(tok == k)[0]
            tp[k] = (out["gB"][fr, k] + out["gI"][fr, k]).mean()
            d = np.arange(T) - fr[0]
            mu[k] = (out["gB"][:, k] * d).sum()
            sd[k] = np.sqrt(max((out["gB"][:, k] * d * d).sum() - mu[k] ** 2, 0.0))
        out["tok_post"], out["start_mean"], out["start_sd"] = tp, mu, sd
    return out


def planted_logits(T, N, C, tokens_cls, gaps, rng, boost, scale=3.0):
    """Scaled standard-normal logits; with boost > 0 the classes of a random monotone path (token k: one B frame, then I frames, no
    gaps) are raised by `boost`, so that posteriors spread over the whole of [0, 1].  tokens_cls: per token its alternatives."""
    z = rng.standard_normal((T, C)) * scale
    if boost > 0 and N > 0 and T >= N:
        cuts = np.sort(rng.choice(np.arange(1, T), N - 1, replace=False)) if N > 1 else np.zeros(0, np.int64)
        st = np.concatenate([[0], cuts]).astype(np.int64)
        en = np.concatenate([cuts, [T]]).astype(np.int64)
        for k in range(N):
            b, i = tokens_cls[k][0]
            z[st[k], b] += boost
            z[st[k] + 1:en[k], i] += boost
    return z.astype(np.float32)
