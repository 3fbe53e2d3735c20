"""float64 numpy restatement of the WINDOWED forced alignment (wfl_align_windowed, wfl_align_posterior_windowed; include/wfl_asr.h),
for the tests.

    a path is accepted only if, for every token k, the frame t at which it is in B_k satisfies lo_k <= t <= hi_k (inclusive)

which is EB_t(k) = -inf outside the window and nothing else.  So this module holds no second DP: it runs viterbi_ref.viterbi and
posterior_ref.forward_backward as they are, on emissions whose EB is masked (`masked`), and adds only what a window makes possible
and the unwindowed lattice never shows: no path at all (None).  The enumerations check the windows on the state sequences
themselves, not through the mask.
"""
from __future__ import annotations

import contextlib

import numpy as np

import posterior_ref as P
import viterbi_ref as V

NEG = -np.inf
OPEN = (0, 2 ** 31 - 1)


def mask_eb(EB, windows):
    """EB [T, N] -> a copy with -inf where frame t is outside token k's window."""
    EB = EB.copy()
    t = np.arange(EB.shape[0])
    for k, (lo, hi) in enumerate(windows):
        EB[(t < lo) | (t > hi), k] = NEG
    return EB


@contextlib.contextmanager
def masked(windows):
    """Inside, viterbi_ref.emissions (which both reference modules call) returns the windowed EB."""
    plain = V.emissions

    def emissions(z, alternatives, gaps):
        e, EB, EI, EG = plain(z, alternatives, gaps)
        return e, mask_eb(EB, windows), EI, EG
    V.emissions = emissions
    try:
        yield
    finally:
        V.emissions = plain


def viterbi(z, alternatives, gaps, windows):
    """-> (states [T], score), or (None, 0.0) when no path satisfies the windows (T < N among the reasons)."""
    with masked(windows), np.errstate(invalid="ignore"):
        path, score = V.viterbi(z, alternatives, gaps)
    if path is None or not np.isfinite(score):
        return None, 0.0
    return path, score


def forward_backward(z, alternatives, gaps, windows, tok=None, dtype=np.float64, renorm=16, want_gamma=False):
    """posterior_ref.forward_backward over the windowed lattice; None when no path satisfies the windows."""
    with masked(windows), np.errstate(all="ignore"):      # (a lattice without a path: logZ = -inf, the rest of the pass is NaN)
        out = P.forward_backward(z, alternatives, gaps, tok=tok, dtype=dtype, renorm=renorm, want_gamma=want_gamma)
    return out if out is not None and np.isfinite(out["logz"]) else None


def starts(states, N):
    """The frame at which each token is in its B state, -1 for a token the sequence never opens."""
    out = np.full(N, -1, np.int64)
    for t, s in enumerate(states):
        k, j = divmod(int(s), 3)
        if j == 1:
            out[k] = t
    return out


def in_windows(states, windows):
    st = starts(states, len(windows))
    return all(lo <= t <= hi for t, (lo, hi) in zip(st, windows))


def accepted_paths(T, N, windows):
    """Every legal path of the lattice that opens every token inside its window (tiny T and N only): walked back from the end
    states along viterbi_ref.preds, each one confirmed by viterbi_ref.legal, then filtered by the windows."""
    if T == 0:
        return []
    paths = []

    def back(tail):
        if len(tail) == T:
            if tail[0] in (0, 1):
                paths.append(tuple(tail))
            return
        for p in V.preds(tail[0], N):
            back([p] + tail)
    for end in ((3 * N, 3 * N - 1, 3 * N - 2) if N else (0,)):
        back([end])
    assert all(V.legal(p, N) for p in paths) and len(set(paths)) == len(paths)
    return [p for p in paths if in_windows(p, windows)]


def brute_force(z, alternatives, gaps, windows):
    """-> (best score or None, logZ or None, number of accepted paths), by enumeration on the UNMASKED emissions."""
    _, EB, EI, EG = V.emissions(z, alternatives, gaps)
    paths = accepted_paths(len(z), len(alternatives), windows)
    if not paths:
        return None, None, 0
    w = np.array([sum(V.state_emission(int(s), t, EB, EI, EG) for t, s in enumerate(p)) for p in paths])
    m = w.max()
    return float(m), float(m + np.log(np.exp(w - m).sum())), len(paths)
