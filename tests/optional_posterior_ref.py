"""numpy forward-backward over the skip lattice of wfl_align_optional, the restatement of what wfl_align_optional_posterior computes
(include/wfl_asr.h), for the tests.  Lattice as tests/viterbi_optional_ref.py, sums as tests/posterior_ref.py:

    weight of a path = exp(sum_t e_t(state_t) - lam * its skipped tokens),   in_k(t) = lse(a_{t-1}(G_k), a_{t-1}(I_{k-1}), a_{t-1}(B_{k-1}))
    a_t(G_k) = EG_t + in_k(t),   a_t(I_k) = EI_t(k) + lse(a_{t-1}(I_k), a_{t-1}(B_k)),
    a_t(B_k) = EB_t(k) + lse(in_k(t), in_{k-1}(t) - lam where opt[k-1])
    b_{t-1}(G_k) = lse(b_t(G_k) + EG_t, b_t(B_k) + EB_t(k), b_t(B_{k+1}) + EB_t(k+1) - lam where opt[k])
    b_{t-1}(B_k) = b_{t-1}(I_k) = lse(b_t(I_k) + EI_t(k), b_t(G_{k+1}) + EG_t, b_t(B_{k+1}) + EB_t(k+1),
                                      b_t(B_{k+2}) + EB_t(k+2) - lam where opt[k+1])
    keep_post[k] = sum_t gamma_t(B_k): a path enters B_k at most once, so this is the posterior that token k is present.

`dtype=np.float64` is the reference; `dtype=np.float32` keeps emissions and recurrences in fp32 and renormalises every `renorm` frames
as the kernel does: its distance from float64 on the same inputs is the yardstick (posterior_ref.forward_backward's rule).
"""
from __future__ import annotations

import numpy as np

import viterbi_ref as V
from posterior_ref import NEG, _lae


def _masked_eb(EB, windows):
    if windows is None:
        return EB
    EB = EB.copy()
    t = np.arange(EB.shape[0])
    for k, (lo, hi) in enumerate(windows):
        EB[(t < lo) | (t > hi), k] = NEG
    return EB


def forward_backward(z, alternatives, gaps, opt=None, lam=0.0, tok=None, windows=None, dtype=np.float64, renorm=16):
    """-> dict: logz, keep_post [N], and with `tok` (wfl_align_optional's per-frame token index) tok_post / start_mean / start_sd [N]
    (a token tok does not hold: tok_post 0, start moments about frame 0; zeros where keep_post is 0).  None when the lattice holds no
    path (T == 0 with tokens, too few frames, windows that cannot be met)."""
    dt = dtype
    _, EB, EI, EG = V.emissions(z, alternatives, gaps)
    EB = _masked_eb(EB, windows)
    EB, EI, EG = EB.astype(dt), EI.astype(dt), EG.astype(dt)
    T, N = EG.shape[0], len(alternatives)
    o = np.zeros(N, bool) if opt is None else np.asarray(opt).astype(bool).reshape(-1)
    assert len(o) == N
    lam = dt(lam)
    if T == 0:
        return None
    may = np.concatenate([[False], o[:N - 1]]) if N else np.zeros(0, bool)      # B_k has skip arcs: opt[k-1]

    def pad(x, n):
        return np.concatenate([x, np.full(n, NEG, dt)]).astype(dt)

    aB = np.empty((T, N), dt)
    aI = np.empty((T, N), dt)
    off = np.zeros(T, np.float64)
    G = np.full(N + 1, NEG, dt)
    B = np.full(N, NEG, dt)
    I = np.full(N, NEG, dt)
    G[0] = 0
    c = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            inn = _lae(dt, G, np.concatenate([[NEG], I]).astype(dt), np.concatenate([[NEG], B]).astype(dt))
            ii = _lae(dt, I, B)
            G = (inn + EG[t]).astype(dt)
            if N:
                skip = np.where(may, (np.concatenate([[NEG], inn[:N - 1]]).astype(dt) - lam).astype(dt), dt(NEG)).astype(dt)
                inb = np.where(may, _lae(dt, inn[:N], skip), inn[:N]).astype(dt)
                B = (inb + EB[t]).astype(dt)
            I = (ii + EI[t]).astype(dt)
            if t % renorm == renorm - 1:
                m = max(G.max(), B.max() if N else NEG, I.max() if N else NEG)
                if not np.isfinite(m):
                    m = dt(0)
                G, B, I = (G - m).astype(dt), (B - m).astype(dt), (I - m).astype(dt)
                c += float(m)
            aB[t], aI[t], off[t] = B, I, c
        ends = [np.float64(G[N])] + ([np.float64(I[N - 1]), np.float64(B[N - 1])] if N else [])
        if N and o[N - 1]:
            ends.append(np.float64(G[N - 1]) - np.float64(lam))
            if N >= 2:
                ends += [np.float64(I[N - 2]) - np.float64(lam), np.float64(B[N - 2]) - np.float64(lam)]
        if not np.isfinite(max(ends)):
            return None
        logz = float(_lae(np.float64, *[np.array([e]) for e in ends])[0]) + c
        bG = np.full(N + 1, NEG, dt)
        bX = np.full(N, NEG, dt)
        bG[N] = 0
        if N:
            bX[N - 1] = 0
            if o[N - 1]:
                bG[N - 1] = -lam
                if N >= 2:
                    bX[N - 2] = -lam
        cb = 0.0
        m0, m1, m2, occ = (np.zeros(N) for _ in range(4))
        first = np.zeros(N, np.int64)
        cnt = np.zeros(N)
        if tok is not None:
            tok = np.asarray(tok)
            for k in range(N):
                fr = np.nonzero(tok == k)[0]
                first[k] = int(fr[0]) if len(fr) else 0
                cnt[k] = len(fr)
        optG = np.concatenate([o, [False]])                      # G_k -> B_{k+1}: opt[k]
        optX = np.concatenate([o[1:], [False]]) if N else o      # X_k -> B_{k+2}: opt[k+1]
        for t in range(T - 1, -1, -1):
            cst = off[t] + cb - logz
            gB = np.exp(aB[t].astype(np.float64) + bX.astype(np.float64) + cst)
            gI = np.exp(aI[t].astype(np.float64) + bX.astype(np.float64) + cst)
            d = (t - first).astype(np.float64)
            m0 += gB
            m1 += gB * d
            m2 += gB * d * d
            if tok is not None and int(tok[t]) >= 0:
                occ[int(tok[t])] += gB[int(tok[t])] + gI[int(tok[t])]
            if t == 0:
                break
            xG = (bG + EG[t]).astype(dt)
            xB = (bX + EB[t]).astype(dt)
            xI = (bX + EI[t]).astype(dt)
            nG = _lae(dt, xG, pad(xB, 1))
            sG = (pad(xB[1:], 2)[:N + 1] - lam).astype(dt)
            nG = np.where(optG, _lae(dt, nG, np.where(optG, sG, dt(NEG)).astype(dt)), nG).astype(dt)
            if N:
                nX = _lae(dt, xI, xG[1:], pad(xB[1:], 1))
                sX = (pad(xB[2:], 2)[:N] - lam).astype(dt)
                nX = np.where(optX, _lae(dt, nX, np.where(optX, sX, dt(NEG)).astype(dt)), nX).astype(dt)
            else:
                nX = bX
            bG, bX = nG, nX
            if t % renorm == 0:
                m = max(bG.max(), bX.max() if N else NEG)
                if not np.isfinite(m):
                    m = dt(0)
                bG, bX = (bG - m).astype(dt), (bX - m).astype(dt)
                cb += float(m)
    out = {"logz": logz, "keep_post": np.clip(m0, 0.0, 1.0), "sum_gamma_b": m0}
    if tok is not None:
        pos = m0 > 0
        mean = np.where(pos, m1 / np.where(pos, m0, 1.0), 0.0)
        var = np.where(pos, m2 / np.where(pos, m0, 1.0) - mean * mean, 0.0)
        out["tok_post"] = np.where(cnt > 0, np.minimum(occ / np.maximum(cnt, 1.0), 1.0), 0.0)
        out["start_mean"] = mean
        out["start_sd"] = np.sqrt(np.maximum(var, 0.0))
    return out


def enumerate_paths(z, alternatives, gaps, opt, lam=0.0, windows=None):
    """Every path of a tiny lattice (viterbi_optional_ref.all_paths) -> dict(logz, keep_post), or None without a path."""
    import viterbi_optional_ref as VO
    _, EB, EI, EG = V.emissions(z, alternatives, gaps)
    EB = _masked_eb(EB, windows)
    T, N = EG.shape[0], len(alternatives)
    paths = VO.all_paths(T, N, opt)
    logw, keep = [], []
    for st in paths:
        w = -lam * int(VO.skipped_of(st, N).sum())
        for t, s in enumerate(st):
            w += V.state_emission(int(s), t, EB, EI, EG)
        logw.append(w)
        keep.append(1 - VO.skipped_of(st, N))
    logw = np.array(logw, np.float64)
    if not len(logw) or not np.isfinite(logw.max()):
        return None
    m = logw.max()
    logz = float(m + np.log(np.exp(logw - m).sum()))
    p = np.exp(logw - logz)
    return {"logz": logz, "keep_post": (p[:, None] * np.array(keep, np.float64).reshape(len(p), N)).sum(0), "n_paths": len(paths)}
