"""numpy forward-backward over the forced-alignment lattice WITH MINIMUM DURATIONS, the restatement of what
wfl_align_min_duration_posterior computes (include/wfl_asr.h), for the tests.  Built on viterbi_ref.emissions,
viterbi_window_ref.mask_eb and the state rules of viterbi_min_ref:

    token k with D = D_k has the states B_k, H_k^2 .. H_k^{D-1} (which emit EI) and I_k; a run is one frame in B_k, one in each chain
    state, every later frame in I_k; the token is left from I_k alone, from B_k as well where D_k == 1

    alpha   G_k, B_k <- G_k, I_{k-1}, and B_{k-1} only where D_{k-1} == 1;  H^2 <- B, H^j <- H^{j-1};  I_k <- I_k, X_k
            (X_k = H_k^{D-1} for D >= 3, B_k for D <= 2);  end states G_N, I_{N-1}, and B_{N-1} only where D_{N-1} == 1
    beta    beta_{t-1}(I_k) = lse(beta_t(I_k) + EI_t, beta_t(G_{k+1}) + EG_t, beta_t(B_{k+1}) + EB_t(k+1));  beta_{t-1}(B_k) is that value
            where D == 1, beta_t(I_k) + EI_t where D == 2, beta_t(H^2) + EI_t above;  beta_{t-1}(H^j) = beta_t(H^{j+1}) + EI_t, the last
            chain state going to I_k.  Held as a delay line c[k, e - 1] = beta(the state e frames in front of I_k)

Every gamma is formed from alpha and beta of its own state: the occupancy of the chain does NOT go through the identity
gamma_t(H^j) = gamma_{t-j+1}(B) that the kernel uses, so the comparison tests that identity too.

`dtype=np.float64` is the reference.  `dtype=np.float32, renorm=16` is the restatement mode of posterior_ref.forward_backward: emissions
and recurrences in fp32, the maximum of G, B, I (alpha) and of G, I (beta) subtracted every `renorm` frames with the offsets in float64,
alpha + beta - logZ and the per-token sums in float64.
"""
from __future__ import annotations

import numpy as np

import viterbi_min_ref as M
import viterbi_ref as V
import viterbi_window_ref as W
from posterior_ref import _lae, _shift_right

NEG = -np.inf
CHAIN = M.CHAIN


def _dur(min_frames, N):
    d = np.asarray(min_frames, np.int64).reshape(N)
    assert ((d >= 1) & (d <= M.MAX_MIN_FRAMES)).all()
    return d


def forward_backward(z, alternatives, gaps, min_frames, tok=None, windows=None, dtype=np.float64, renorm=16, want_gamma=False):
    """-> dict: logz, and with `tok` (wfl_align_min_duration's per-frame token index, -1 in gaps) tok_post / start_mean / start_sd /
    sum_gamma_b [N]; with want_gamma gG [T, N + 1], gB [T, N], gI [T, N], gH [T, N, CHAIN] (gH[..., j] of H^{j + 2}).  None when no
    path meets the durations (and the windows): T < N among the reasons."""
    dt = dtype
    _, EB, EI, EG = V.emissions(z, alternatives, gaps)
    if windows is not None:
        EB = W.mask_eb(EB, windows)
    EB, EI, EG = EB.astype(dt), EI.astype(dt), EG.astype(dt)
    T, N = EG.shape[0], len(alternatives)
    if T < N or T == 0:
        return None
    d = _dur(min_frames, N)
    rows = np.arange(N)
    reach = (np.arange(CHAIN)[None, :] + 3 <= d[:, None])          # H^{j+2} exists for D_k >= j + 3
    leave_b = d == 1
    aB = np.empty((T, N), dt)
    aI = np.empty((T, N), dt)
    aG = np.empty((T, N + 1), dt) if want_gamma else None
    aH = np.empty((T, N, CHAIN), dt) if want_gamma else None
    aHrun = np.full((T, CHAIN), NEG, dt)                            # the chain of the token Viterbi's run holds at t
    tokv = np.asarray(tok) if tok is not None else None
    off = np.zeros(T, np.float64)
    G = np.full(N + 1, NEG, dt)
    B = np.full(N, NEG, dt)
    I = np.full(N, NEG, dt)
    H = np.full((N, CHAIN), NEG, dt)
    G[0] = 0                                                        # a virtual frame -1 in G_0
    c = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            inn = _lae(dt, G, _shift_right(I, dt), _shift_right(np.where(leave_b, B, dt(NEG)).astype(dt), dt))
            X = np.where(d <= 2, B, H[rows, np.maximum(d - 3, 0)]).astype(dt) if N else B
            ii = _lae(dt, I, X)
            nH = np.empty_like(H)
            nH[:, 1:] = H[:, :-1]
            nH[:, 0] = B
            H = np.where(reach, (nH + EI[t][:, None]).astype(dt), dt(NEG)).astype(dt)
            G = (inn + EG[t]).astype(dt)
            B = (inn[:N] + EB[t]).astype(dt)
            I = (ii + EI[t]).astype(dt)
            if t % renorm == renorm - 1:
                m = max(G.max(), B.max() if N else NEG, I.max() if N else NEG)
                if not np.isfinite(m):
                    m = dt(0)
                G, B, I, H = (G - m).astype(dt), (B - m).astype(dt), (I - m).astype(dt), (H - m).astype(dt)
                c += float(m)
            aB[t], aI[t], off[t] = B, I, c
            if want_gamma:
                aG[t], aH[t] = G, H
            if tokv is not None and tokv[t] >= 0:
                aHrun[t] = H[int(tokv[t])]
        ends = [np.float64(G[N])]
        if N:
            ends.append(np.float64(I[N - 1]))
            if d[N - 1] == 1:
                ends.append(np.float64(B[N - 1]))
        logz = float(_lae(np.float64, *[np.array([e]) for e in ends])[0]) + c
        if not np.isfinite(logz):
            return None
        bG = np.full(N + 1, NEG, dt)
        bI = np.full(N, NEG, dt)
        cb_line = np.full((N, CHAIN + 1), NEG, dt)                  # c[k, e - 1]: beta of the state e frames in front of I_k
        bG[N] = 0
        if N:
            bI[N - 1] = 0
        cb = 0.0
        out = {"logz": logz}
        if want_gamma:
            out["gG"], out["gB"], out["gI"] = np.zeros((T, N + 1)), np.zeros((T, N)), np.zeros((T, N))
            out["gH"] = np.zeros((T, N, CHAIN))
        if tokv is not None:
            first = np.array([int(np.nonzero(tokv == k)[0][0]) for k in range(N)], np.int64)
            cnt = np.array([int((tokv == k).sum()) for k in range(N)], np.float64)
            occ, m0, m1, m2 = (np.zeros(N) for _ in range(4))
        e_of = d[:, None] - (np.arange(CHAIN)[None, :] + 2)          # H^{j+2} is e = D - (j + 2) frames in front of I_k
        e_idx = np.maximum(e_of - 1, 0)
        for t in range(T - 1, -1, -1):
            cst = off[t] + cb - logz
            bB = np.where(leave_b, bI, cb_line[rows, np.maximum(d - 2, 0)]).astype(dt) if N else bI
            gB = np.exp(aB[t].astype(np.float64) + bB.astype(np.float64) + cst)
            gI = np.exp(aI[t].astype(np.float64) + bI.astype(np.float64) + cst)
            if want_gamma:
                out["gG"][t] = np.exp(aG[t].astype(np.float64) + bG.astype(np.float64) + cst)
                out["gB"][t], out["gI"][t] = gB, gI
                bH = np.where(reach, cb_line[rows[:, None], e_idx], NEG)
                out["gH"][t] = np.where(reach, np.exp(aH[t].astype(np.float64) + bH.astype(np.float64) + cst), 0.0)
            if tokv is not None:
                dd = (t - first).astype(np.float64)
                m0 += gB
                m1 += gB * dd
                m2 += gB * dd * dd
                k = int(tokv[t])
                if k >= 0:
                    bHk = np.where(reach[k], cb_line[k, e_idx[k]], NEG).astype(np.float64)
                    gHk = np.where(reach[k], np.exp(aHrun[t].astype(np.float64) + bHk + cst), 0.0)
                    occ[k] += gB[k] + gI[k] + gHk.sum()
            if t == 0:
                break
            xG = (bG + EG[t]).astype(dt)
            xB = (bB + EB[t]).astype(dt)
            xI = (bI + EI[t]).astype(dt)
            nG = _lae(dt, xG, np.concatenate([xB, np.full(1, NEG, dt)]).astype(dt))
            nI = _lae(dt, xI, xG[1:], np.concatenate([xB[1:], np.full(1, NEG, dt)]).astype(dt)) if N else bI
            nline = np.empty_like(cb_line)
            nline[:, 1:] = cb_line[:, :-1]
            nline[:, 0] = bI
            cb_line = (nline + EI[t][:, None]).astype(dt)
            bG, bI = nG, nI
            if t % renorm == 0:
                m = max(bG.max(), bI.max() if N else NEG)
                if not np.isfinite(m):
                    m = dt(0)
                bG, bI, cb_line = (bG - m).astype(dt), (bI - m).astype(dt), (cb_line - m).astype(dt)
                cb += float(m)
    if tokv is not None:
        mean = m1 / m0
        out["tok_post"] = occ / cnt
        out["start_mean"] = mean
        out["start_sd"] = np.sqrt(np.maximum(m2 / m0 - mean * mean, 0.0))
        out["sum_gamma_b"] = m0
    return out


def expand(states, N, min_frames):
    """A path in the three-state numbering of viterbi_ref (a chain frame written as I_k) -> per frame (kind, k, j): kind 'G' | 'B' |
    'H' | 'I', j the chain state's number (2 .. D_k - 1) for 'H'.  The p-th frame of a run is B (p = 1), H^p (p < D_k), else I."""
    d = _dur(min_frames, N)
    out, pos = [], {}
    for s in states:
        k, j = divmod(int(s), 3)
        if j == 0:
            out.append(("G", k, 0))
            continue
        p = pos[k] = pos.get(k, 0) + 1
        assert (p == 1) == (j == 1)
        out.append(("B", k, 0) if p == 1 else ("H", k, p) if p < d[k] else ("I", k, 0))
    return out


def path_score(z, alternatives, gaps, tok):
    """posterior_ref.path_score: chain frames emit EI, as the I frames they are written as."""
    from posterior_ref import path_score as ps
    return ps(z, alternatives, gaps, tok)


def brute_force(z, alternatives, gaps, windows, min_frames, tok=None):
    """Every path of viterbi_min_ref.accepted_paths enumerated (tiny T and N only): the same dict as
    forward_backward(want_gamma=True), and n_paths; None when there is none."""
    _, EB, EI, EG = V.emissions(z, alternatives, gaps)
    T, N = len(z), len(alternatives)
    paths = M.accepted_paths(T, N, windows, min_frames)
    if not paths:
        return None
    logw = np.array([sum(V.state_emission(int(s), t, EB, EI, EG) for t, s in enumerate(p)) for p in paths])
    m = logw.max()
    logz = float(m + np.log(np.exp(logw - m).sum()))
    w = np.exp(logw - logz)
    out = {"logz": logz, "n_paths": len(paths), "gG": np.zeros((T, N + 1)), "gB": np.zeros((T, N)), "gI": np.zeros((T, N)),
           "gH": np.zeros((T, N, CHAIN))}
    for wp, p in zip(w, paths):
        for t, (kind, k, j) in enumerate(expand(p, N, min_frames)):
            if kind == "H":
                out["gH"][t, k, j - 2] += wp
            else:
                out["g" + kind][t, k] += wp
    if tok is not None:
        tok = np.asarray(tok)
        tp, mu, sd = np.zeros(N), np.zeros(N), np.zeros(N)
        for k in range(N):
            fr = np.nonzero(tok == k)[0]
            tp[k] = (out["gB"][fr, k] + out["gI"][fr, k] + out["gH"][fr, k].sum(axis=1)).mean()
            dd = np.arange(T) - fr[0]
            mu[k] = (out["gB"][:, k] * dd).sum()
            sd[k] = np.sqrt(max((out["gB"][:, k] * dd * dd).sum() - mu[k] ** 2, 0.0))
        out["tok_post"], out["start_mean"], out["start_sd"] = tp, mu, sd
    return out
