"""-m gpu: wfl_align_optional (csrc/align.hip with OPT) against the float64 numpy DP of tests/viterbi_optional_ref.py, with the checks
and tolerances of tests/test_gpu_align.py::_check: the kernel's path is legal, its float64 score within 1e-3 of the optimum, `score`
within 1e-3 T, and on planted logits states, ids, tok and skipped equal the reference's."""
import numpy as np
import pytest
import torch

import viterbi_optional_ref as R
from wfl_asr_amd import align as AL

pytestmark = pytest.mark.gpu
C = 141
O_ID = 0
GAPS = [O_ID, 137, 138]
SLOTS = ((127, 2), (511, 2), (1023, 4), (2047, 8), (4096, 9))          # csrc/lattice.h: token cap of a configuration, its R


def _slots(N):
    return next(r for cap, r in SLOTS if N <= cap)


def _alts(N, rng, n_alt=1):
    """Random phonemes, none equal to either of the two before it (a skip between equal neighbours would be an exact tie)."""
    ph = []
    for k in range(N):
        while True:
            p = rng.choice(np.arange(1, 68), size=n_alt, replace=False)
            if not any(set(p.tolist()) & set(q.tolist()) for q in ph[-2:]):
                break
        ph.append(p)
    return [[(int(2 * p - 1), int(2 * p)) for p in q] for q in ph]


def _run(clips, lam, windows=None):
    """clips: list of (z [T, C] float32, alternatives, flags or None) -> numpy (ids, tok, score, status, skipped) per clip."""
    z = np.concatenate([c[0] for c in clips])
    lg = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    T = [len(c[0]) for c in clips]
    out = AL.viterbi_align_optional(lg, T, [c[1] for c in clips], [GAPS] * len(clips), O_ID, [c[2] for c in clips], lam,
                                    windows=windows)
    torch.cuda.synchronize()
    ids, tok, score, status, skipped = (x.cpu().numpy() for x in out)
    res, pos, k0 = [], 0, 0
    for b, t in enumerate(T):
        n = len(clips[b][1])
        res.append((ids[pos:pos + t], tok[pos:pos + t], float(score[b]), int(status[b]), skipped[k0:k0 + n]))
        pos += t
        k0 += n
    return res


def _path_states(ids, tok, alts):
    """(ids, tok) -> the state sequence the kernel walked (B classes are the odd ones here).  A gap frame behind the kept token k is
    in G_{k+1}, whether or not token k + 1 is skipped after it."""
    s = np.zeros(len(ids), np.int64)
    done = 0
    for t in range(len(ids)):
        k = int(tok[t])
        if k < 0:
            s[t] = 3 * done
        else:
            is_b = any(int(ids[t]) == b for b, _ in alts[k])
            s[t] = 3 * k + (1 if is_b else 2)
            done = k + 1
    return s


def _refused(got, status):
    ids, tok, score, st, skipped = got
    assert st == status
    assert (ids == O_ID).all() and (tok == -1).all() and (skipped == 0).all() and score == 0.0


def _check(z, alts, opt, lam, got, windows=None, planted=None):
    ids, tok, score, status, skipped = got
    T, N = len(z), len(alts)
    ref, ref_score = R.viterbi(z, alts, GAPS, opt, lam, windows)
    if ref is None:
        _refused(got, 1)
        return None
    assert status == 0
    states = _path_states(ids, tok, alts)
    assert R.legal(states, N, opt), "the kernel's path is not a legal path"
    if windows is not None:
        for t in np.nonzero(states % 3 == 1)[0]:
            lo, hi = windows[int(states[t]) // 3]
            assert lo <= t <= hi, "a token opens outside its window"
    assert (skipped == R.skipped_of(states, N)).all()
    mine = R.path_score(states, z, alts, GAPS, lam)
    assert mine >= ref_score - 1e-3, (mine, ref_score)
    assert abs(score - ref_score) <= 1e-3 * T, (score, ref_score)
    if planted is not None:
        assert (ref == planted).all(), "the planted path is not the reference's optimum (test setup)"
        rid, rtok, rskip = R.outputs(ref, z, alts, O_ID)
        assert (states == ref).all()
        assert (ids == rid).all() and (tok == rtok).all() and (skipped == rskip).all()
    return states


# ------------------------------------------------------------------------------------------------ no flag set: wfl_align, bit for bit
def test_without_a_flag_every_output_is_wfl_aligns():
    rng = np.random.default_rng(21)
    clips = []
    for N in (0, 1, 5, 127, 128, 300):
        T = N + int(rng.integers(1, 80)) + N // 3
        clips.append((rng.standard_normal((T, C)).astype(np.float32) * 3, _alts(N, rng, 1 + N % 2)))
    clips.append((rng.standard_normal((9, C)).astype(np.float32), _alts(12, rng)))          # T < N: status 1 in both
    lg = torch.from_numpy(np.concatenate([c[0] for c in clips])).cuda()
    Ts, alts = [len(c[0]) for c in clips], [c[1] for c in clips]
    plain = AL.viterbi_align(lg, Ts, alts, [GAPS] * len(clips), O_ID)
    assert plain[3].tolist() == [0] * 6 + [1]
    # windows around the unwindowed path's starts, the last feasible clip's first window emptied: one clip without path
    tok = plain[1].cpu().numpy()
    wins, pos = [], 0
    for T, a in zip(Ts, alts):
        tk = tok[pos:pos + T]
        starts = [int(np.nonzero(tk == k)[0][0]) if (tk == k).any() else 0 for k in range(len(a))]
        wins.append([(max(s - 3, 0), s + 3) for s in starts])
        pos += T
    wins[5][0] = (4, 3)
    windowed = AL.viterbi_align(lg, Ts, alts, [GAPS] * len(clips), O_ID, windows=wins)
    assert windowed[3].tolist() == [0] * 5 + [1, 1]
    zeros = [[False] * len(a) for a in alts]
    for lam in (0.0, 3.0):
        for flags in (zeros, [None] * len(clips)):
            for want, w in ((plain, None), (windowed, wins)):
                got = AL.viterbi_align_optional(lg, Ts, alts, [GAPS] * len(clips), O_ID, flags, lam, windows=w)
                for a, b in zip(want, got[:4]):
                    assert torch.equal(a, b)
                assert not got[4].any()


# ------------------------------------------------------------------------------------------------ planted paths, every configuration
def _skip_set(N, R_):
    """Token 0 and N - 1, tokens in slots 0, 1 and R - 1 of their threads, both sides of the first wave boundary (64 R - 1 and
    64 R + 1) and the second one itself (128 R): never two in a row."""
    want = [0, N - 1, 64 * R_ - 1, 64 * R_ + 1, 128 * R_, 10 * R_, 13 * R_ + 1, 17 * R_ - 1, 20 * R_ + 1, 23 * R_, 27 * R_ - 1]
    out = []
    for k in want:
        if 0 <= k < N and all(abs(k - j) > 1 for j in out):
            out.append(k)
    return sorted(out)


def _runs_entering_from_each(kept, skipped, rng, extra):
    """One frame per kept token, `extra` more frames handed out as gap or token frames, then the kept token behind every skipped one
    is entered from G (a gap in front), from I (no gap, the token before it two frames or more) and from B (no gap, that token one
    frame), in turn."""
    g = np.zeros(len(kept), np.int64)
    d = np.ones(len(kept), np.int64)
    for j in rng.integers(0, len(kept), extra):
        (g if rng.random() < 0.4 else d)[j] += 1
    mode = 0
    for j, k in enumerate(kept):
        if k - 1 in skipped and j > 0:
            if mode == 0:
                g[j] = max(g[j], 1)
            else:
                g[j] = 0
                d[j - 1] = 3 if mode == 1 else 1
            mode = (mode + 1) % 3
    return [(int(a), int(b)) for a, b in zip(g, d)]


PLANTED = {}


def _planted(N):
    if N not in PLANTED:
        rng = np.random.default_rng(N)
        R_ = _slots(N)
        skipped = _skip_set(N, R_)
        kept = [k for k in range(N) if k not in skipped]
        runs = _runs_entering_from_each(kept, set(skipped), rng, 190)
        T = sum(a + b for a, b in runs) + 7
        alts = _alts(N, rng)
        opt = rng.random(N) < 0.3                                          # optional tokens the path keeps, too
        opt[skipped] = True
        z, st = R.plant(T, N, C, alts, GAPS, rng, skipped=skipped, runs=runs)
        entered = {int(st[t - 1]) % 3 for t in range(1, T) if st[t] % 3 == 1 and st[t] // 3 - 1 in skipped}
        assert entered == {0, 1, 2} and st[0] == 4 and st[-1] == 3 * (N - 1), "test setup"
        PLANTED[N] = (z, alts, opt, st)
    return PLANTED[N]


@pytest.mark.parametrize("lam", [0.0, 2.5])
def test_planted_paths_in_every_configuration(lam):
    cases = [_planted(N) for N in (100, 400, 900, 1500, 2100)]
    got = _run([(z, a, o) for z, a, o, _ in cases], lam)
    for (z, alts, opt, st), g in zip(cases, got):
        _check(z, alts, opt, lam, g, planted=st)


# ------------------------------------------------------------------------------------------------ two tokens per frame in the backtrace
@pytest.mark.parametrize("N", [120, 600])
def test_the_two_per_frame_descent(N):
    """Every token optional; every even token one frame and every odd one skipped for N - 8 tokens (>= 48 frames: across a
    32-frame backtrace window and a renormalisation), then one long run, then the same descent to the end."""
    rng = np.random.default_rng(N + 1)
    kept = list(range(0, N, 2))
    long_at = len(kept) - 4
    runs = [(0, 40 if j == long_at else 1) for j in range(len(kept))]
    T = sum(d for _, d in runs)
    assert long_at >= 48
    alts = _alts(N, rng)
    opt = [True] * N
    z, st = R.plant(T, N, C, alts, GAPS, rng, skipped=range(1, N, 2), runs=runs)
    for lam, g in ((0.0, _run([(z, alts, opt)], 0.0)[0]), (2.5, _run([(z, alts, opt)], 2.5)[0])):
        _check(z, alts, opt, lam, g, planted=st)


# ------------------------------------------------------------------------------------------------ the penalty decides
def test_the_penalty_decides_a_skip():
    rng = np.random.default_rng(33)
    alts = _alts(3, rng)
    opt = [False, True, False]
    z, st = R.plant(30, 3, C, alts, GAPS, rng, skipped=[1])
    free, s_skip = R.viterbi(z, alts, GAPS, opt, 0.0)
    _, s_keep = R.viterbi(z, alts, GAPS, None, 0.0)
    delta = s_skip - s_keep
    assert (free == st).all() and delta > 1.0, "test setup"
    lo, hi = 0.5 * delta, 2.0 * delta
    assert R.skipped_of(R.viterbi(z, alts, GAPS, opt, lo)[0], 3).tolist() == [0, 1, 0]      # the reference first
    assert R.skipped_of(R.viterbi(z, alts, GAPS, opt, hi)[0], 3).tolist() == [0, 0, 0]
    a, b = _run([(z, alts, opt)], lo)[0], _run([(z, alts, opt)], hi)[0]
    _check(z, alts, opt, lo, a)
    _check(z, alts, opt, hi, b)
    assert a[4].tolist() == [0, 1, 0] and b[4].tolist() == [0, 0, 0]
    assert abs(a[2] - (s_skip - lo)) <= 1e-3 * 30 and abs(b[2] - s_keep) <= 1e-3 * 30


# ------------------------------------------------------------------------------------------------ feasibility and the refusals
def test_feasibility_and_refused_clips_beside_feasible_ones():
    """The issue's N = 5, all optional: T = 3 is status 0, and on logits planted for it the path holds exactly tokens 0, 2, 4.  The
    issue also asks for status 1 at T = 2; the lattice it defines, its own rule N - sum ceil(run / 2) = 2 and the enumeration of
    every path (tests/test_align_optional_cpu.py) all give that clip the one path B_1 B_3 -- tokens 0, 2 and 4 skipped -- so here
    T = 2 must be status 0 with exactly tokens 1, 3, and T = 1 is the status 1."""
    rng = np.random.default_rng(44)
    z = lambda T: rng.standard_normal((T, C)).astype(np.float32) * 2          # noqa: E731
    a5, a4, a1, big = _alts(5, rng), _alts(4, rng), _alts(1, rng), _alts(4097, rng)
    z024, st024 = R.plant(3, 5, C, a5, GAPS, rng, skipped=[1, 3], runs=[(0, 1)] * 3)
    clips = [(z024, a5, [1] * 5), (z(2), a5, [1] * 5), (z(1), a5, [1] * 5), (z(2), a4, [1, 1, 0, 0]), (z(3), a4, [1, 1, 0, 0]),
             (z(1), a1, [1]), (z(4200), big, [1] * 4097), (z(20), a5, [0, 2, 0, 0, 0]), (z(40), a5, [0, 1, 0, 1, 0])]
    got = _run(clips, 0.0)
    assert [g[3] for g in got] == [0, 0, 1, 1, 0, 0, 2, 4, 0]
    for b, ((zc, alts, opt), g) in enumerate(zip(clips, got)):
        if g[3] in (0, 1):
            _check(zc, alts, opt, 0.0, g, planted=st024 if b == 0 else None)
        else:
            _refused(g, g[3])
    assert got[0][1].tolist() == [0, 2, 4] and got[0][4].tolist() == [0, 1, 0, 1, 0]
    assert got[1][1].tolist() == [1, 3] and got[1][4].tolist() == [1, 0, 1, 0, 1]
    assert sorted(set(got[4][1].tolist()) - {-1}) in ([0, 2, 3], [1, 2, 3])
    for opt, T in (([1] * 5, 2), ([1, 1, 0, 0], 3), ([1], 1), ([0, 1, 0, 1, 0], 3), ([1, 1, 1, 0, 1, 1], 3)):
        assert AL.min_frames_needed(opt) == R.min_frames_needed(opt) == T


# ------------------------------------------------------------------------------------------------ windows
def test_windows_hold_and_an_empty_window_forces_the_skip():
    rng = np.random.default_rng(55)
    N = 60
    alts = _alts(N, rng)
    skipped = [0, 7, 20, 21 + 2, 41, N - 1]
    kept = [k for k in range(N) if k not in skipped]
    runs = _runs_entering_from_each(kept, set(skipped), rng, 70)
    T = sum(a + b for a, b in runs) + 5
    z, st = R.plant(T, N, C, alts, GAPS, rng, skipped=skipped, runs=runs)
    opt = np.zeros(N, bool)
    opt[skipped] = True
    opt[[3, 30]] = True
    starts = {int(s) // 3: t for t, s in enumerate(st) if s % 3 == 1}
    wins = [(starts[k] - 2, starts[k] + 2) if k in starts else (5, 4) for k in range(N)]       # the skipped tokens: empty windows
    zr = rng.standard_normal((T, C)).astype(np.float32) * 3                                  # the same windows on random logits
    got = _run([(z, alts, opt), (zr, alts, opt), (z, alts, None)], 2.5, windows=[wins, wins, wins])
    _check(z, alts, opt, 2.5, got[0], windows=wins, planted=st)
    states = _check(zr, alts, opt, 2.5, got[1], windows=wins)
    assert states is not None and got[1][4][skipped].all()                                   # an empty window: the token is skipped
    _refused(got[2], 1)                                                                       # the same windows without the flags


# ------------------------------------------------------------------------------------------------ independence
def test_a_clip_alone_equals_the_clip_in_a_batch_of_16():
    rng = np.random.default_rng(69)
    clips = []
    for b in range(16):
        N = int(rng.integers(1, 600))
        T = int(rng.integers(max(N // 2, 1), 2 * N + 100))
        clips.append((rng.standard_normal((T, C)).astype(np.float32) * 3, _alts(N, rng, int(rng.integers(1, 4))),
                      (rng.random(N) < 0.5).tolist()))
    batch = _run(clips, 1.0)
    assert {g[3] for g in batch} == {0, 1}
    for b in (0, 5, 15):
        alone = _run([clips[b]], 1.0)[0]
        for x, y in zip(alone, batch[b]):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    for (zc, alts, opt), g in list(zip(clips, batch))[:6]:
        _check(zc, alts, opt, 1.0, g)
