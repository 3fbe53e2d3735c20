"""numpy forward-backward over the filler lattice of wfl_align_filler, the restatement of what wfl_align_filler_posterior computes
(include/wfl_asr.h), for the tests.  Lattice and emissions as tests/viterbi_filler_ref.py (a flagged token emits the frame's largest
log-posterior over all classes minus phi; windows mask EB), sums as tests/posterior_ref.py:

    a_t(G_k) = EG_t + lse(a_{t-1}(G_k), a_{t-1}(I_{k-1}), a_{t-1}(B_{k-1}))     a_t(B_k): the same sum + EB_t(k)
    a_t(I_k) = EI_t(k) + lse(a_{t-1}(I_k), a_{t-1}(B_k))
    b_{t-1}(G_k) = lse(b_t(G_k) + EG_t, b_t(B_k) + EB_t(k))
    leave_k(t)   = lse(b_t(G_{k+1}) + EG_t, b_t(B_{k+1}) + EB_t(k+1))           leave_k(T) = 0 for k = N - 1, -inf below
    b_{t-1}(B_k) = b_{t-1}(I_k) = lse(b_t(I_k) + EI_t(k), leave_k(t))
    omega_t(k)   = exp(lse(a_t(B_k), a_t(I_k)) + leave_k(t + 1) - logZ)         the posterior that token k's run ends on frame t

`dtype=np.float64` is the reference; `dtype=np.float32` keeps emissions and recurrences in fp32 and renormalises every `renorm` frames
as the kernel does: its distance from float64 on the same inputs is the yardstick (posterior_ref.forward_backward's rule).
"""
from __future__ import annotations

import numpy as np

import viterbi_filler_ref as VF
import viterbi_ref as V
from posterior_ref import NEG, _lae


def forward_backward(z, alternatives, gaps, fill=None, phi=1.0, tok=None, windows=None, dtype=np.float64, renorm=16, full=False):
    """-> dict: logz, and with `tok` (wfl_align_filler's per-frame token index) the six per-token outputs tok_post, start_mean,
    start_sd, end_mean, end_sd [N] (status is the caller's).  full: gamma_b / gamma_i [T, N], gamma_g [T, N + 1] and omega [T, N] as
    well.  None when the lattice holds no path (T == 0, T < N, windows that cannot be met)."""
    dt = dtype
    EB, EI, EG = VF.emissions(z, alternatives, gaps, fill, phi, windows)
    EB, EI, EG = EB.astype(dt), EI.astype(dt), EG.astype(dt)
    T, N = EG.shape[0], len(alternatives)
    if T == 0 or T < N:
        return None

    def pad(x, n):
        return np.concatenate([x, np.full(n, NEG, dt)]).astype(dt)

    aG = np.empty((T, N + 1), dt)
    aB = np.empty((T, N), dt)
    aI = np.empty((T, N), dt)
    off = np.zeros(T, np.float64)
    G = np.full(N + 1, NEG, dt)
    B = np.full(N, NEG, dt)
    I = np.full(N, NEG, dt)
    G[0] = 0
    c = 0.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for t in range(T):
            inn = _lae(dt, G, np.concatenate([[NEG], I]).astype(dt), np.concatenate([[NEG], B]).astype(dt))
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
        if not np.isfinite(max(ends)):
            return None
        logz = float(_lae(np.float64, *[np.array([e]) for e in ends])[0]) + c
        bG = np.full(N + 1, NEG, dt)
        bX = np.full(N, NEG, dt)
        lv = np.full(N, NEG, dt)                 # leave_k(t + 1), on the scale of b_t
        bG[N] = 0
        if N:
            bX[N - 1] = 0
            lv[N - 1] = 0
        cb = 0.0
        m0, m1, m2, occ, e0, e1, e2 = (np.zeros(N) for _ in range(7))
        first = np.zeros(N, np.int64)
        last = np.zeros(N, np.int64)
        cnt = np.zeros(N)
        if tok is not None:
            tok = np.asarray(tok)
            for k in range(N):
                fr = np.nonzero(tok == k)[0]
                first[k] = int(fr[0]) if len(fr) else 0
                last[k] = int(fr[-1]) if len(fr) else 0
                cnt[k] = len(fr)
        gam_g = np.zeros((T, N + 1))
        gam_b = np.zeros((T, N))
        gam_i = np.zeros((T, N))
        omega = np.zeros((T, N))
        for t in range(T - 1, -1, -1):
            cst = off[t] + cb - logz
            gB = np.exp(aB[t].astype(np.float64) + bX.astype(np.float64) + cst)
            gI = np.exp(aI[t].astype(np.float64) + bX.astype(np.float64) + cst)
            om = np.exp(aB[t].astype(np.float64) + lv.astype(np.float64) + cst) + np.exp(aI[t].astype(np.float64) + lv.astype(np.float64) + cst)
            if full:
                gam_g[t] = np.exp(aG[t].astype(np.float64) + bG.astype(np.float64) + cst)
                gam_b[t], gam_i[t], omega[t] = gB, gI, om
            d = (t - first).astype(np.float64)
            m0 += gB
            m1 += gB * d
            m2 += gB * d * d
            de = (t - last).astype(np.float64)
            e0 += om
            e1 += om * de
            e2 += om * de * de
            if tok is not None and int(tok[t]) >= 0:
                occ[int(tok[t])] += gB[int(tok[t])] + gI[int(tok[t])]
            if t == 0:
                break
            xG = (bG + EG[t]).astype(dt)
            xB = (bX + EB[t]).astype(dt)
            xI = (bX + EI[t]).astype(dt)
            nG = _lae(dt, xG, pad(xB, 1))
            if N:
                lv = _lae(dt, xG[1:], pad(xB[1:], 1))
                nX = _lae(dt, xI, lv)
            else:
                nX = bX
            bG, bX = nG, nX
            if t % renorm == 0:
                m = max(bG.max(), bX.max() if N else NEG)
                if not np.isfinite(m):
                    m = dt(0)
                bG, bX, lv = (bG - m).astype(dt), (bX - m).astype(dt), (lv - m).astype(dt)
                cb += float(m)
    out = {"logz": logz}
    if full:
        out.update(gamma_g=gam_g, gamma_b=gam_b, gamma_i=gam_i, omega=omega)
    if tok is not None:
        def moments(s0, s1, s2):
            pos = s0 > 0
            mean = np.where(pos, s1 / np.where(pos, s0, 1.0), 0.0)
            var = np.where(pos, s2 / np.where(pos, s0, 1.0) - mean * mean, 0.0)
            return mean, np.sqrt(np.maximum(var, 0.0))
        out["tok_post"] = np.where(cnt > 0, np.minimum(occ / np.maximum(cnt, 1.0), 1.0), 0.0)
        out["start_mean"], out["start_sd"] = moments(m0, m1, m2)
        out["end_mean"], out["end_sd"] = moments(e0, e1, e2)
    return out


OUTPUTS = ("logz", "tok_post", "start_mean", "start_sd", "end_mean", "end_sd")


def seven(z, alternatives, gaps, fill, phi, tok, windows=None, dtype=np.float64, renorm=16):
    """The entry's seven outputs for one clip -> (logz, tok_post, start_mean, start_sd, end_mean, end_sd, status): status 1 and zeros
    where the lattice holds no path."""
    N = len(alternatives)
    r = forward_backward(z, alternatives, gaps, fill, phi, tok, windows, dtype, renorm)
    if r is None:
        return (0.0,) + tuple(np.zeros(N) for _ in range(5)) + (1,)
    return tuple(r[k] for k in OUTPUTS) + (0,)


def enumerate_paths(z, alternatives, gaps, fill=None, phi=1.0, windows=None):
    """Every legal path of a tiny lattice (viterbi_filler_ref.all_paths) -> dict(logz, gamma [T, 3N + 1] over the states, omega [T, N],
    n_paths), or None without a path of finite weight."""
    EB, EI, EG = VF.emissions(z, alternatives, gaps, fill, phi, windows)
    T, N = EG.shape[0], len(alternatives)
    paths = VF.all_paths(T, N)
    logw = np.array([sum(V.state_emission(int(s), t, EB, EI, EG) for t, s in enumerate(st)) for st in paths], np.float64)
    if not len(logw) or not np.isfinite(logw.max()):
        return None
    m = logw.max()
    logz = float(m + np.log(np.exp(logw - m).sum()))
    p = np.exp(logw - logz)
    gamma = np.zeros((T, 3 * N + 1))
    omega = np.zeros((T, N))
    for w, st in zip(p, paths):
        for t, s in enumerate(st):
            gamma[t, int(s)] += w
            k, j = divmod(int(s), 3)
            if j and (t == T - 1 or divmod(int(st[t + 1]), 3) != (k, 2)):     # in B_k / I_k now, not in I_k next: the run ends here
                omega[t, k] += w
    return {"logz": logz, "gamma": gamma, "omega": omega, "n_paths": len(paths)}
