"""numpy forward-backward over the explicit-duration lattice of wfl_align_duration_prior, the restatement of what
wfl_align_duration_prior_posterior computes (include/wfl_asr.h), for the tests.  Emissions as tests/viterbi_ref.py (log-softmax, the
maximum over a token's alternatives; windows mask EB), the prior as tests/viterbi_duration_prior_ref.py (L [N, D] and tail [N] from the
table's rows, row -1: zeros).  A path weighs exp(sum_t e_t + sum_k L_k(d_k)).

    ent_k(t)  = lse(aG_k(t-1), aX_{k-1}(t-1))                      ent_0(0) = 0, every other ent_k(0) = -inf
    aG_k(t)   = ent_k(t) + EG_t
    aR_k^1(t) = ent_k(t) + EB_t(k);   aR_k^j(t) = aR_k^{j-1}(t-1) + EI_t(k)
    aY_k(t)   = lse(aY_k(t-1), aR_k^D(t-1) + L_k(D)) + EI_t(k) + tail_k
    aX_k(t)   = lse(aR_k^1(t) + L_k(1), .., aR_k^D(t) + L_k(D), aY_k(t))
    logZ      = lse(aG_N(T-1), aX_{N-1}(T-1))
    V_k(t)    = lse(bE_{k+1}(t), EI_{t+1}(k) + tail_k + V_k(t+1))
    W_k^j(t)  = lse(L_k(j) + bE_{k+1}(t), EI_{t+1}(k) + W_k^{j+1}(t+1))   j < D;      W_k^D(t) = L_k(D) + V_k(t)
    bE_k(t-1) = lse(bE_k(t) + EG_t, EB_t(k) + W_k^1(t))
    start_k(t) = exp(aR_k^1(t) + W_k^1(t) - logZ),   end_k(t) = exp(aX_k(t) + bE_{k+1}(t) - logZ)
    occ_k(t)   = sum_j exp(aR_k^j(t) + W_k^j(t) - logZ) + exp(aY_k(t) + V_k(t) - logZ)

occ is formed from alpha and beta of the run states themselves, NOT as (starts so far) - (ends before): the kernel takes the second
route, so a comparison with it tests that identity as well.

`dtype=np.float64` is the reference.  `dtype=np.float32` keeps emissions, table and recurrences in fp32 and renormalises as the kernel
does -- alpha every `renorm` frames by the maximum over G, X, Y and the ring, beta by the maximum over bE, V and the ring, offsets in
float64: its distance from float64 on the same inputs is the yardstick for what fp32 costs (posterior_ref.forward_backward's rule).
In both, alpha + beta - logZ and the per-token sums are formed in float64.
"""
from __future__ import annotations

import numpy as np

import viterbi_duration_prior_ref as VD
import viterbi_ref as V
import viterbi_window_ref as W
from posterior_ref import NEG, _lae

OUTPUTS = ("logz", "tok_post", "start_mean", "start_sd", "end_mean", "end_sd")


def _max(*xs):
    m = NEG
    for x in xs:
        if np.size(x):
            m = max(m, float(np.max(x)))
    return m


def forward_backward(z, alternatives, gaps, rows, table, tok=None, windows=None, dtype=np.float64, renorm=16, full=False):
    """-> dict: logz, and with `tok` (wfl_align_duration_prior's per-frame token index) tok_post, start_mean, start_sd, end_mean,
    end_sd [N]; full: start, end, occ [T, N] as well.  None when the lattice holds no path of finite weight."""
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

    # alpha on its true scale, float64 (what was held in dt, plus the offset).  aR^1 and aX of every token; the run states aR^1 .. aR^D
    # and aY of every token only with `full` -- else of the one token tok gives the frame, all tok_post asks for (T x D, not T x D x N)
    if tok is not None:
        tok = np.asarray(tok, np.int64)
    A_R1 = np.empty((T, N))
    A_X = np.empty((T, N))
    A_R = np.empty((T, D, N)) if full else np.full((T, D), NEG)
    A_Y = np.empty((T, N)) if full else np.full(T, NEG)
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
            if t % renorm == renorm - 1:
                m = _max(G, X, Y, R)
                if not np.isfinite(m):
                    m = 0.0
                m = dt(m)
                G, X, Y, R = (G - m).astype(dt), (X - m).astype(dt), (Y - m).astype(dt), (R - m).astype(dt)
                c += float(m)
            A_X[t] = X.astype(f8) + c
            if N:
                A_R1[t] = R[0].astype(f8) + c
            if full:
                A_R[t], A_Y[t] = R.astype(f8) + c, Y.astype(f8) + c
            elif tok is not None and tok[t] >= 0:
                A_R[t], A_Y[t] = R[:, tok[t]].astype(f8) + c, f8(Y[tok[t]]) + c
        ends = [np.array([f8(G[N])])] + ([np.array([f8(X[N - 1])])] if N else [])
        if not np.isfinite(max(float(e[0]) for e in ends)):
            return None
        logz = float(_lae(f8, *ends)[0]) + c

        first = np.zeros(N, np.int64)
        last = np.zeros(N, np.int64)
        if tok is not None:
            for k in range(N):
                fr = np.nonzero(tok == k)[0]
                first[k], last[k] = (int(fr[0]), int(fr[-1])) if len(fr) else (0, 0)
        m0, m1, m2, e0, e1, e2, occ_run = (np.zeros(N) for _ in range(7))
        if full:
            start, end, occ = np.zeros((T, N)), np.zeros((T, N)), np.zeros((T, N))
        bE = np.full(N + 1, NEG, dt)
        bE[N] = 0
        Vv = np.full(N, NEG, dt)
        Wv = np.full((D, N), NEG, dt)             # Wv[j - 1] = W^j
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
            cst = cb - logz
            gs = np.exp(A_R1[t] + Wv[0].astype(f8) + cst)
            ge = np.exp(A_X[t] + nE.astype(f8) + cst)
            ds, de = (t - first).astype(f8), (t - last).astype(f8)
            m0 += gs
            m1 += gs * ds
            m2 += gs * ds * ds
            e0 += ge
            e1 += ge * de
            e2 += ge * de * de
            if full:
                start[t], end[t] = gs, ge
                occ[t] = np.exp(A_R[t] + Wv.astype(f8) + cst).sum(axis=0) + np.exp(A_Y[t] + Vv.astype(f8) + cst)
                if tok is not None and tok[t] >= 0:
                    occ_run[tok[t]] += occ[t, tok[t]]
            elif tok is not None and tok[t] >= 0:
                k = tok[t]
                occ_run[k] += np.exp(A_R[t] + Wv[:, k].astype(f8) + cst).sum() + np.exp(A_Y[t] + f8(Vv[k]) + cst)
            if t == 0:
                break
            nb = np.empty_like(bE)
            nb[:N] = _lae(dt, (bE[:N] + EG[t]).astype(dt), (EB[t] + Wv[0]).astype(dt))
            nb[N] = bE[N] + EG[t]
            bE = nb.astype(dt)
            ep = EI[t]
            if t % renorm == 0:
                m = _max(bE, Vv, Wv)
                if not np.isfinite(m):
                    m = 0.0
                m = dt(m)
                bE, Vv, Wv = (bE - m).astype(dt), (Vv - m).astype(dt), (Wv - m).astype(dt)
                cb += float(m)
    out = {"logz": logz}
    if full:
        out.update(start=start, end=end, occ=occ)
    if tok is not None:
        def moments(s0, s1, s2):
            pos = s0 > 0
            mean = np.where(pos, s1 / np.where(pos, s0, 1.0), 0.0)
            var = np.where(pos, s2 / np.where(pos, s0, 1.0) - mean * mean, 0.0)
            return mean, np.sqrt(np.maximum(var, 0.0))

        out["tok_post"] = np.clip(occ_run / np.maximum(last - first + 1, 1), 0.0, 1.0)
        out["start_mean"], out["start_sd"] = moments(m0, m1, m2)
        out["end_mean"], out["end_sd"] = moments(e0, e1, e2)
    return out


def seven(z, alternatives, gaps, rows, table, tok, windows=None, dtype=np.float64, renorm=16):
    """The entry's seven outputs for one clip -> (logz, tok_post, start_mean, start_sd, end_mean, end_sd, status): status 1 and zeros
    where the lattice holds no path."""
    N = len(alternatives)
    r = forward_backward(z, alternatives, gaps, rows, table, tok, windows, dtype, renorm)
    if r is None:
        return (0.0,) + tuple(np.zeros(N) for _ in range(5)) + (1,)
    return tuple(r[k] for k in OUTPUTS) + (0,)


def enumerate_segmentations(z, alternatives, gaps, rows, table, windows=None):
    """Every segmentation of a tiny lattice (viterbi_duration_prior_ref.segmentations) -> dict(logz, start, end, occ [T, N], n_paths),
    or None without a path of finite weight."""
    T, N = len(z), len(alternatives)
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
    start, end, occ = np.zeros((T, N)), np.zeros((T, N)), np.zeros((T, N))
    for w, seg in zip(p, segs):
        for k, (s, d) in enumerate(seg):
            start[s, k] += w
            end[s + d - 1, k] += w
            occ[s:s + d, k] += w
    return {"logz": logz, "start": start, "end": end, "occ": occ, "n_paths": len(segs)}
