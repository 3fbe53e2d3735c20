"""-m gpu: wfl_align_filler (csrc/align.hip with FILL) against the float64 numpy DP of tests/viterbi_filler_ref.py, with the checks
and tolerances of tests/test_gpu_align.py::_check: the kernel's path is legal, its float64 score within 1e-3 of the optimum, `score`
within 1e-3 T, and on planted logits states, ids and tok equal the reference's."""
import numpy as np
import pytest
import torch

import viterbi_filler_ref as R
import viterbi_ref as V
from wfl_asr_amd import align as AL

pytestmark = pytest.mark.gpu
C = 141
O_ID = 0
GAPS = [O_ID, 137, 138]
SLOTS = ((127, 2), (511, 2), (1023, 4), (2047, 8), (4096, 9))          # csrc/lattice.h: token cap of a configuration, its R
PLACEHOLDER = [(O_ID, O_ID)]                                           # a filler's row of the token table: one valid pair, never read


def _slots(N):
    return next(r for cap, r in SLOTS if N <= cap)


def _alts(N, rng, n_alt=1, fill=None):
    """Random phonemes, none equal to the one before it; a filler gets the placeholder pair."""
    ph = []
    for k in range(N):
        while True:
            p = rng.choice(np.arange(1, 68), size=n_alt, replace=False)
            if not (ph and set(p.tolist()) & set(ph[-1].tolist())):
                break
        ph.append(p)
    out = [[(int(2 * p - 1), int(2 * p)) for p in q] for q in ph]
    if fill is not None:
        out = [PLACEHOLDER if f else a for a, f in zip(out, fill)]
    return out


def _run(clips, phi, windows=None, gaps=GAPS):
    """clips: list of (z [T, C] float32, alternatives, flags or None) -> numpy (ids, tok, score, status) per clip."""
    z = np.concatenate([c[0] for c in clips])
    lg = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    T = [len(c[0]) for c in clips]
    out = AL.viterbi_align_filler(lg, T, [c[1] for c in clips], [gaps] * len(clips), O_ID, [c[2] for c in clips], phi, windows=windows)
    torch.cuda.synchronize()
    ids, tok, score, status = (x.cpu().numpy() for x in out)
    res, pos = [], 0
    for b, t in enumerate(T):
        res.append((ids[pos:pos + t], tok[pos:pos + t], float(score[b]), int(status[b])))
        pos += t
    return res


def _path_states(ids, tok, alts, fill):
    """(ids, tok) -> the state sequence the kernel walked.  A plain token's frame is B_k where its id is one of the token's B classes; a
    filler's frames carry any class, so its run's first frame is B_k and the others I_k (the only way through a token)."""
    s = np.zeros(len(ids), np.int64)
    done = 0
    for t in range(len(ids)):
        k = int(tok[t])
        if k < 0:
            s[t] = 3 * done
        else:
            if fill is not None and fill[k]:
                is_b = t == 0 or int(tok[t - 1]) != k
            else:
                is_b = any(int(ids[t]) == b for b, _ in alts[k])
            s[t] = 3 * k + (1 if is_b else 2)
            done = k + 1
    return s


def _refused(got, status, o_id=O_ID):
    ids, tok, score, st = got
    assert st == status
    assert (ids == o_id).all() and (tok == -1).all() and score == 0.0


def _check(z, alts, fill, phi, got, windows=None, planted=None, gaps=GAPS, exact_ids=True):
    ids, tok, score, status = got
    T, N = len(z), len(alts)
    ref, ref_score = R.viterbi(z, alts, gaps, fill, phi, windows)
    print(f"T {T} N {N} phi {phi}: status {status} score {score:.4f} reference {ref_score:.4f}")
    if ref is None:
        _refused(got, 1)
        return None
    assert status == 0
    states = _path_states(ids, tok, alts, fill)
    assert R.legal(states, N), "the kernel's path is not a legal path"
    if windows is not None:
        for t in np.nonzero(states % 3 == 1)[0]:
            lo, hi = windows[int(states[t]) // 3]
            assert lo <= t <= hi, "a token opens outside its window"
    mine = R.path_score(states, z, alts, gaps, fill, phi)
    print(f"    the kernel's path in float64 {mine:.6f}")
    assert mine >= ref_score - 1e-3, (mine, ref_score)
    assert abs(score - ref_score) <= 1e-3 * T, (score, ref_score)
    if exact_ids:                                      # every frame's id is what the entry defines for the state the path is in
        rid, rtok = R.outputs(states, z, alts, O_ID, fill)
        assert (ids == rid).all() and (tok == rtok).all()
    if planted is not None:
        assert (ref == planted).all(), "the planted path is not the reference's optimum (test setup)"
        rid, rtok = R.outputs(ref, z, alts, O_ID, fill)
        assert (states == ref).all()
        assert (ids == rid).all() and (tok == rtok).all()
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
    for phi in (0.0, 3.0):
        for flags in (zeros, [None] * len(clips)):
            for want, w in ((plain, None), (windowed, wins)):
                got = AL.viterbi_align_filler(lg, Ts, alts, [GAPS] * len(clips), O_ID, flags, phi, windows=w)
                for a, b in zip(want, got):
                    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ planted paths, every configuration
RUN_LENGTHS = (1, 2, 17, 40)        # of the fillers: 17 crosses a renormalisation (16 frames), 40 a stage and a backtrace window (32)


def _filler_set(N, R_):
    """Token 0 and N - 1, tokens in slots 0, 1 and R - 1 of their threads, both sides of the first wave boundary (64 R - 1 and
    64 R + 1) and the second one itself (128 R): never two in a row."""
    want = [0, N - 1, 64 * R_ - 1, 64 * R_ + 1, 128 * R_, 10 * R_, 13 * R_ + 1, 17 * R_ - 1, 20 * R_ + 1, 23 * R_, 27 * R_ - 1]
    out = []
    for k in want:
        if 0 <= k < N and all(abs(k - j) > 1 for j in out):
            out.append(k)
    return sorted(out)


def _plant_case(N, rng, C_=C, gaps=GAPS, fillers=None, extra=190, alts=None, lengths=RUN_LENGTHS):
    fillers = _filler_set(N, _slots(N)) if fillers is None else fillers
    fill = np.zeros(N, bool)
    fill[fillers] = True
    g = np.zeros(N, np.int64)
    d = np.ones(N, np.int64)
    for j in rng.integers(0, N, extra):
        if not fill[j]:
            (g if rng.random() < 0.4 else d)[j] += 1
    for n, k in enumerate(fillers):
        d[k] = lengths[n % len(lengths)]
        g[k] = n % 2
    runs = [(int(a), int(b)) for a, b in zip(g, d)]
    T = sum(a + b for a, b in runs) + 7
    alts = _alts(N, rng, fill=fill) if alts is None else alts
    z, st = R.plant(T, N, C_, alts, gaps, rng, fill=fill, runs=runs)
    return z, alts, fill, st


PLANTED = {}


def _planted(N):
    if N not in PLANTED:
        PLANTED[N] = _plant_case(N, np.random.default_rng(N))
        z, alts, fill, st = PLANTED[N]
        lengths = {int((st // 3 == k).sum() - (st == 3 * k).sum()) for k in np.nonzero(fill)[0]}
        assert lengths == set(RUN_LENGTHS) and fill[0] and fill[N - 1], "test setup"
    return PLANTED[N]


def test_planted_paths_in_every_configuration():
    phi = 1.5
    cases = [_planted(N) for N in (100, 400, 900, 1500, 2100)]
    for (z, alts, fill, st) in cases:                    # in a filler's frames: a winner that is no gap class and no neighbour's class,
        for t in np.nonzero(fill[np.minimum(st // 3, len(alts) - 1)] & (st % 3 != 0))[0][::7]:          # by phi + 1 over every class
            k, w = int(st[t]) // 3, int(z[t].argmax())
            near = {c for q in (k - 1, k + 1) if 0 <= q < len(alts) for pair in alts[q] for c in pair}
            assert w not in near and w not in GAPS and z[t, w] - np.delete(z[t], w).max() >= phi + 1
    got = _run([(z, a, f) for z, a, f, _ in cases], phi)
    for (z, alts, fill, st), g in zip(cases, got):
        _check(z, alts, fill, phi, g, planted=st)


# ------------------------------------------------------------------------------------------------ one row per stage, 32 rows per stage
def test_stage_extremes():
    """C = 1024: F = 1 on the 64-thread configuration, every frame a stage of its own.  C = 5: F = 32.  N = 20, T about 120."""
    rng = np.random.default_rng(61)
    z, alts, fill, st = _plant_case(20, rng, C_=1024, fillers=[0, 5, 11, 19], extra=60)
    assert 100 <= len(z) <= 160
    _check(z, alts, fill, 1.5, _run([(z, alts, fill)], 1.5)[0], planted=st)
    # five classes: O, a = (1, 2), b = (3, 4).  A filler stands between two tokens of one phoneme, so the other's classes are free for it;
    # its runs are short, or the later tokens of that other phoneme would spell a long run of its classes better than the filler does
    a, b = [(1, 2)], [(3, 4)]
    alts5 = [a, PLACEHOLDER, a, b, PLACEHOLDER, b] * 3 + [a, b]
    fillers = [1, 4, 7, 10, 13, 16]
    z, alts5, fill, st = _plant_case(20, rng, C_=5, gaps=[0], fillers=fillers, extra=110, alts=alts5, lengths=(1, 2, 3))
    assert 100 <= len(z) <= 160
    _check(z, alts5, fill, 1.5, _run([(z, alts5, fill)], 1.5, gaps=[0])[0], planted=st, gaps=[0])


# ------------------------------------------------------------------------------------------------ the penalty decides
def test_the_penalty_decides_the_fillers_run():
    rng = np.random.default_rng(33)
    fill = [False, True, False]
    alts = _alts(3, rng, fill=fill)
    L = 10
    z, st = R.plant(30, 3, C, alts, GAPS, rng, fill=fill, runs=[(2, 6), (1, L), (1, 7)])
    _, s_fill = R.viterbi(z, alts, GAPS, fill, 0.0)     # (the score alone: at a price of 0 the filler ties with its neighbours' best frames)
    s_best = max(V.viterbi(z, [alts[0], [(2 * p - 1, 2 * p)], alts[2]], GAPS)[1] for p in range(1, 68))     # its best single phoneme
    delta = s_fill - s_best
    print(f"delta {delta:.3f} over {L} frames")
    assert delta > L, "test setup"
    lo, hi = 0.5 * delta / L, 2.0 * delta / L
    run_of = lambda s: np.nonzero((s == 4) | (s == 5))[0]                                    # noqa: E731
    planted_run = run_of(st)
    assert len(planted_run) == L
    ref_lo, ref_hi = R.viterbi(z, alts, GAPS, fill, lo)[0], R.viterbi(z, alts, GAPS, fill, hi)[0]         # the reference first
    assert (run_of(ref_lo) == planted_run).all() and 1 <= len(run_of(ref_hi)) < L
    a, b = _run([(z, alts, fill)], lo)[0], _run([(z, alts, fill)], hi)[0]
    _check(z, alts, fill, lo, a, planted=st)
    _check(z, alts, fill, hi, b)
    assert (np.nonzero(a[1] == 1)[0] == planted_run).all() and (np.nonzero(b[1] == 1)[0] == run_of(ref_hi)).all()


def test_phi_zero_on_random_logits():
    """A filler then ties exactly with a neighbour wherever the neighbour's class is the frame's best: legality and score only."""
    rng = np.random.default_rng(34)
    clips = []
    for N in (3, 40, 200, 600):
        T = N + int(rng.integers(20, 120))
        fill = rng.random(N) < 0.2
        fill[1:] &= ~fill[:-1]
        fill[[N // 2 - 1, N // 2, N // 2 + 1]] = False, True, False                          # (one at least, never two in a row)
        clips.append((rng.standard_normal((T, C)).astype(np.float32) * 3, _alts(N, rng, fill=fill), fill))
    for (z, alts, fill), g in zip(clips, _run(clips, 0.0)):
        assert _check(z, alts, fill, 0.0, g) is not None and fill.any()


# ------------------------------------------------------------------------------------------------ the refusals
def test_statuses_beside_feasible_clips():
    rng = np.random.default_rng(44)
    z = lambda T: rng.standard_normal((T, C)).astype(np.float32) * 2          # noqa: E731
    f5 = [0, 1, 0, 0, 1]
    a5, big = _alts(5, rng, fill=f5), _alts(4097, rng)
    clips = [(z(30), a5, f5), (z(4), a5, f5), (z(4200), big, [1] + [0] * 4096), (z(20), a5, [0, 2, 0, 0, 0]), (z(40), a5, f5),
             (z(25), a5, f5), (z(5), a5, f5)]
    wins = [None, None, None, None, None, [(0, 3), (2, 2), (1, 2), (9, 12), (10, 30)], None]      # token 2 cannot open after token 1
    got = _run(clips, 1.0, windows=wins)
    assert [g[3] for g in got] == [0, 1, 2, 4, 0, 1, 0]
    for (zc, alts, fill), g, w in zip(clips, got, wins):
        if g[3] == 0:
            _check(zc, alts, fill, 1.0, g)
        else:
            _refused(g, g[3])
    assert R.viterbi(clips[5][0], a5, GAPS, f5, 1.0, wins[5]) == (None, 0.0) and R.viterbi(clips[1][0], a5, GAPS, f5, 1.0) == (None, 0.0)
    assert sorted(set(got[6][1].tolist())) == [0, 1, 2, 3, 4]                                # T == N: every token one frame


# ------------------------------------------------------------------------------------------------ windows
def test_windows_hold_for_a_filler_too():
    rng = np.random.default_rng(55)
    N = 60
    z, alts, fill, st = _plant_case(N, rng, fillers=[0, 7, 20, 23, 41, N - 1], extra=70)
    T = len(z)
    starts = {int(s) // 3: t for t, s in enumerate(st) if s % 3 == 1}
    wins = [(starts[k] - 2, starts[k] + 2) for k in range(N)]
    late = list(wins)
    late[20] = (starts[20] + 2, starts[20] + 3)                                              # the filler may open only two frames late
    zr = rng.standard_normal((T, C)).astype(np.float32) * 3                                  # the same windows on random logits
    got = _run([(z, alts, fill), (zr, alts, fill), (z, alts, fill)], 1.5, windows=[wins, wins, late])
    _check(z, alts, fill, 1.5, got[0], windows=wins, planted=st)
    assert _check(zr, alts, fill, 1.5, got[1], windows=wins) is not None
    states = _check(z, alts, fill, 1.5, got[2], windows=late)
    opened = int(np.nonzero(states == 3 * 20 + 1)[0][0])
    assert late[20][0] <= opened <= late[20][1] and opened != starts[20]


# ------------------------------------------------------------------------------------------------ independence
def test_a_clip_alone_equals_the_clip_in_a_batch_of_16():
    rng = np.random.default_rng(69)
    clips = []
    for b in range(16):
        N = int(rng.integers(1, 600))
        T = int(rng.integers(max(N // 2, 1), 2 * N + 100))
        fill = rng.random(N) < 0.15
        fill[1:] &= ~fill[:-1]
        alts = [PLACEHOLDER if f else a for a, f in zip(_alts(N, rng, int(rng.integers(1, 4))), fill)]
        clips.append((rng.standard_normal((T, C)).astype(np.float32) * 3, alts, fill.tolist()))
    batch = _run(clips, 1.0)
    assert {g[3] for g in batch} == {0, 1}
    for b in (0, 5, 15):
        alone = _run([clips[b]], 1.0)[0]
        for x, y in zip(alone, batch[b]):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    for (zc, alts, fill), g in list(zip(clips, batch))[:6]:
        _check(zc, alts, fill, 1.0, g)
