"""-m gpu: wfl_align_duration_prior_posterior (csrc/align_duration_prior_posterior.hip) against the float64 forward-backward over the
explicit-duration lattice of tests/duration_prior_posterior_ref.py.  `tok` is what wfl_align_duration_prior returned for the same
clips, rows and table.

Tolerances are the project's rule (tests/test_gpu_align_posterior.py, tests/test_gpu_align_filler_posterior.py), restated here for the
six float outputs: for every case the float32 restatement of the reference (same renormalisation period and the same maxima as the
kernel) is run on the same inputs; its largest deviation from float64 over the case, per output, is the yardstick, and the kernel is
allowed 4 x that against float64; where the yardstick is below half an fp32 ulp of the value itself, that half ulp is added (the
outputs are fp32).  Every clip and token of every case is compared, and the figures are printed before anything is asserted.  The
bit-for-bit assertions are "a clip alone equals the clip in a batch": same kernel, same arithmetic.  The reference forms occ from alpha
and beta of the run states, the kernel from the starts and the ends: the comparison holds that identity as well."""
import ctypes

import numpy as np
import pytest
import torch

import duration_posterior_ref as DPR
import duration_prior_posterior_ref as PR
import filler_posterior_ref as FP
import posterior_ref as P
import viterbi_filler_ref as VF
from wfl_asr_amd import align as AL

pytestmark = pytest.mark.gpu
C = 141
O_ID = 0
GAPS = [O_ID, 137, 138]
KEYS = PR.OUTPUTS
SLOTS = ((127, 2), (511, 2), (1023, 4), (2047, 8), (4096, 9))          # csrc/lattice.h: token cap of a configuration, its R
BLOCK = 128                                                            # POST_W: frames per recomputed block
NEG = -np.inf


def _slots(N):
    return next(r for cap, r in SLOTS if N <= cap)


def _alts(N, rng):
    """Random phonemes, none equal to either of the two before it."""
    ph = []
    for _ in range(N):
        while True:
            p = int(rng.integers(1, 68))
            if p not in ph[-2:]:
                break
        ph.append(p)
    return [[(2 * p - 1, 2 * p)] for p in ph]


def _upload(clips):
    T = [len(c[0]) for c in clips]
    lg = torch.from_numpy(np.ascontiguousarray(np.concatenate([c[0] for c in clips]))).cuda()
    return lg, T, [c[1] for c in clips], [GAPS] * len(clips), O_ID


def _split(clips, tok, vst, score, out):
    T = [len(c[0]) for c in clips]
    tok, vst, score = tok.cpu().numpy(), vst.cpu().numpy(), score.cpu().numpy()
    logz, tp, mu, sd, emu, esd, st = (x.cpu().numpy() for x in out)
    res, pos, k0 = [], 0, 0
    for b, t in enumerate(T):
        n = len(clips[b][1])
        res.append(dict(tok=tok[pos:pos + t], vstatus=int(vst[b]), score=float(score[b]), logz=np.array([logz[b]], np.float32),
                        tok_post=tp[k0:k0 + n], start_mean=mu[k0:k0 + n], start_sd=sd[k0:k0 + n], end_mean=emu[k0:k0 + n],
                        end_sd=esd[k0:k0 + n], status=int(st[b])))
        pos += t
        k0 += n
    return res


def _run(clips, table, windows=None, tok_edit=None, search_table=None, post_rows=None):
    """clips: list of (z [T, C] float32, alternatives, rows) -> per clip a dict of the search's tok / status / score and the entry's
    outputs.  search_table: the table the search runs under when it is not the scorer's; post_rows: the scorer's rows likewise."""
    args = _upload(clips)
    rows = [c[2] for c in clips]
    _, tok, score, vst = AL.viterbi_align_duration_prior(*args, rows, table if search_table is None else search_table, windows=windows)
    if tok_edit is not None:
        tok = tok_edit(tok.clone())
    out = AL.duration_prior_posteriors(*args, rows if post_rows is None else post_rows, table, tok, windows=windows)
    torch.cuda.synchronize()
    return _split(clips, tok, vst, score, out)


def _zeros(g):
    return g["logz"][0] == 0 and not any(g[k].any() for k in KEYS[1:])


def _same(a, b):
    return a["status"] == b["status"] and all(a[k].tobytes() == b[k].tobytes() for k in KEYS)


def _half_ulp(ref):
    return 0.5 * np.spacing(np.abs(np.asarray(ref, np.float64)).astype(np.float32)).astype(np.float64)


REFS = {}                                   # a reference is computed once per (case, clip) and left unchanged


def _refs(key, z, alts, rows, table, tok, win):
    if key not in REFS:
        REFS[key] = (PR.forward_backward(z, alts, GAPS, rows, table, tok=tok, windows=win),
                     PR.forward_backward(z, alts, GAPS, rows, table, tok=tok, windows=win, dtype=np.float32))
    return REFS[key]


def _check_case(name, clips, table, got, windows=None, keys=KEYS, refs=None):
    """Every clip of a case against float64, by the 4 x yardstick rule; prints the figures before it asserts.  refs: per clip a
    (float64, float32) pair of dicts from another reference, for the reductions."""
    yard = {k: 0.0 for k in keys}
    r64s = []
    for b, ((z, alts, rows), g) in enumerate(zip(clips, got)):
        win = windows[b] if windows is not None else None
        assert g["status"] == g["vstatus"], (name, b, g["status"], g["vstatus"])
        if g["status"] != 0:
            assert _zeros(g)
            if g["status"] == 1:
                assert PR.forward_backward(z, alts, GAPS, rows, table, windows=win) is None
            r64s.append(None)
            continue
        r64, r32 = refs[b] if refs is not None else _refs((name, b), z, alts, rows, table, g["tok"], win)
        assert r64 is not None, (name, b)
        assert not any(np.isnan(g[k]).any() for k in KEYS)
        assert (g["tok_post"] >= 0).all() and (g["tok_post"] <= 1).all() and (g["start_sd"] >= 0).all() and (g["end_sd"] >= 0).all()
        for k in keys:
            ref = np.atleast_1d(np.asarray(r64[k], np.float64))
            if ref.size:
                yard[k] = max(yard[k], float(np.abs(np.atleast_1d(r32[k]) - ref).max()))
        r64s.append(r64)
    dev = {k: 0.0 for k in keys}
    over = {k: -np.inf for k in keys}
    for g, r64 in zip(got, r64s):
        if r64 is None:
            continue
        for k in keys:
            ref = np.atleast_1d(np.asarray(r64[k], np.float64))
            if not ref.size:
                continue
            d = np.abs(g[k].astype(np.float64) - ref)
            h = _half_ulp(ref)
            allowed = 4 * yard[k] + np.where(yard[k] < h, h, 0.0)
            dev[k] = max(dev[k], float(d.max()))
            over[k] = max(over[k], float((d - allowed).max()))
    for k in keys:
        print(f"{name}: {k}: kernel {dev[k]:.3e}, float32 restatement {yard[k]:.3e}, allowed 4 x = {4 * yard[k]:.3e} (+ half an fp32 ulp "
              f"where that exceeds the restatement), over by {max(over[k], 0.0):.3e}")
    for k in keys:
        assert over[k] <= 0, (name, k, dev[k], yard[k], over[k])
    return r64s


# ------------------------------------------------------------------------------------------------ tables and planted clips
def _soft_table(n_soft, D, rng):
    """n_soft soft rows (entries uniform in [-6, 0], tails in [-1, 0]), then an "exactly D" row (prefix and tail -inf) and a "D or
    more" row (prefix -inf, a finite tail)."""
    t = rng.uniform(-6, 0, (n_soft + 2, D + 1))
    t[:, D] = rng.uniform(-1, 0, n_soft + 2)
    t[n_soft, :D - 1] = NEG
    t[n_soft, D] = NEG
    t[n_soft + 1, :D - 1] = NEG
    return t.astype(np.float32)


def _boundary_threads(N, R_):
    """Threads whose slots R - 1 (of the thread before), 0 and 1 get the hard rows; thread 64 opens the second wave."""
    return [i for i in (10, 64) if i * R_ + 2 < N]


def planted_clip(N, seed, D=8, n_soft=12, margin=6.0):
    """T = int(1.3 N) + 37.  About half the tokens a soft row, the thread-boundary tokens the hard ones: slots R - 1 and 0 exactly D
    frames, slot 1 D frames or more (planted with D + 3).  At the boundaries of the recomputed blocks, in turn: a run that ends on the
    block's last frame with the next token the single first frame of the next block, and a run of more than D frames (a soft row: a
    tail run) across the boundary.  -> ((z, alts, rows), table, the hard tokens, the planted states)"""
    rng = np.random.default_rng(seed)
    R_ = _slots(N)
    T = int(1.3 * N) + 37
    table = _soft_table(n_soft, D, rng)
    rows = np.where(rng.random(N) < 0.5, rng.integers(0, n_soft, N), -1)
    need = np.ones(N, np.int64)
    hard = []
    for i in _boundary_threads(N, R_):
        for k, row, d in ((i * R_ - 1, n_soft, D), (i * R_, n_soft, D), (i * R_ + 1, n_soft + 1, D + 3)):
            rows[k], need[k] = row, d
            hard.append(k)
    alts = _alts(N, rng)
    spare = T - int(need.sum()) - 4
    runs, t, single, turn = [], 0, False, 0
    for k in range(N):
        nxt = (t // BLOCK + 1) * BLOCK
        g, d = 0, int(need[k])
        free = need[k] == 1 and (k + 1 >= N or need[k + 1] == 1)
        if single:
            single = False                                   # the single first frame of a block
        elif free and 2 <= nxt - t <= 4 and turn % 2 == 0 and spare >= nxt - t:
            d, single, turn = nxt - t, True, turn + 1        # ends on the block's last frame
        elif free and 2 <= nxt - t <= 4 and spare >= nxt - t + D:
            d, turn = nxt - t + D, turn + 1                  # more than D frames, across the boundary: a tail run
            rows[k] = int(rng.integers(0, n_soft))
        elif free:
            g = int(spare > 0 and rng.random() < 0.15)
            d = 1 + int(spare > g and rng.random() < 0.2)
        spare -= g + d - int(need[k])
        runs.append((g, d))
        t += g + d
    assert sum(g + d for g, d in runs) <= T and spare >= 0
    z, states = VF.plant(T, N, C, alts, GAPS, rng, runs=runs, margin=margin, scale=1.5)
    return (z, alts, [int(r) for r in rows]), table, hard, states


def _ends(tok, N):
    first = np.array([int(np.nonzero(tok == k)[0][0]) for k in range(N)])
    last = np.array([int(np.nonzero(tok == k)[0][-1]) for k in range(N)])
    return first, last


CONFIG_N = (100, 300, 700, 1500, 2500)


# ------------------------------------------------------------------------------------------------ 1. one clip per configuration
def test_one_clip_per_launch_configuration():
    D = 8
    made = [planted_clip(N, N, D) for N in CONFIG_N]
    got = []
    for m in made:                                           # (a table per clip: one call each)
        got += _run([m[0]], m[1])
    seen = set()
    for N, (clip, tab, hard, _), g in zip(CONFIG_N, made, got):
        _check_case(f"configuration N = {N}", [clip], tab, [g])
        assert g["status"] == 0 and len(hard) >= 3
        first, last = _ends(g["tok"], N)
        length = last - first + 1
        rows = np.array(clip[2])
        exact, more = rows == len(tab) - 2, rows == len(tab) - 1
        assert exact[hard].sum() >= 2 and more[hard].sum() >= 1 and (length[exact] == D).all() and (length[more] >= D).all()
        assert (last % BLOCK == BLOCK - 1).any(), "no run ends on the last frame of a block"
        assert ((first % BLOCK == 0) & (length == 1) & (first > 0)).any(), "no run is the single first frame of a block"
        # (the smallest clip has one block boundary, which the two layouts above take)
        spans = bool(((length > D) & (rows >= 0) & (first // BLOCK != last // BLOCK)).any())
        assert spans or len(g["tok"]) <= 2 * BLOCK, "no tail run spans a block boundary"
        seen.add(spans)
        assert (g["tok_post"][hard] > 0).all()
    assert True in seen


# ------------------------------------------------------------------------------------------------ 2. D = 1 and D = 32, ring placement
def _lds_rings(N, D):
    """How many of the kernel's two rings its LDS holds (include/wfl_asr.h, the entry's workspace formula)."""
    c = [i for i, (cap, _) in enumerate(SLOTS) if N <= cap][0]
    slots = (128, 512, 1024, 2048, 4608)[c]
    return min(2, (148992, 112128, 99840, 75264, 9728)[c] // (4 * slots * D))


def _random_clip(T, N, seed, n_rows, D, scale=2.0, p_row=0.6):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((T, C)) * scale).astype(np.float32)
    rows = np.where(rng.random(N) < p_row, rng.integers(0, max(n_rows, 1), N), -1)
    return z, _alts(N, rng), [int(r) for r in rows]


@pytest.mark.parametrize("D", (1, 32))
def test_the_shortest_and_the_longest_table(D):
    rng = np.random.default_rng(500 + D)
    table = rng.uniform(-6, 0, (10, D + 1)).astype(np.float32)
    table[:, D] = rng.uniform(-1, 0, 10)
    clips = [_random_clip(N + 150, N, 510 + N + D, 10, D) for N in (40, 700)]
    assert [_lds_rings(40, D), _lds_rings(700, D)] == ([2, 2] if D == 1 else [2, 0])
    _check_case(f"D = {D}", clips, table, _run(clips, table))


@pytest.mark.parametrize("N,D", ((300, 27), (300, 28), (700, 12), (700, 13), (700, 24), (700, 25), (1500, 4), (1500, 5), (1500, 9),
                                 (1500, 10)))
def test_both_sides_of_every_ring_threshold(N, D):
    """One clip on each side of every D at which a configuration's LDS lets go of a ring (N <= 127 keeps both at every D, N > 2047 none:
    test 1)."""
    want = {(300, 27): 2, (300, 28): 1, (700, 12): 2, (700, 13): 1, (700, 24): 1, (700, 25): 0, (1500, 4): 2, (1500, 5): 1, (1500, 9): 1,
            (1500, 10): 0}[(N, D)]
    assert _lds_rings(N, D) == want
    rng = np.random.default_rng(600 + N + D)
    table = rng.uniform(-6, 0, (10, D + 1)).astype(np.float32)
    table[:, D] = rng.uniform(-1, 0, 10)
    clips = [_random_clip(N + 150, N, 610 + N + D, 10, D)]
    _check_case(f"N = {N}, D = {D}, {want} rings in LDS", clips, table, _run(clips, table))


# ------------------------------------------------------------------------------------------------ 3. reductions
def test_without_rows_it_is_wfl_align_posterior():
    """Rows all -1: against posterior_ref in float64; the end moments against filler_posterior_ref with no flag."""
    rng = np.random.default_rng(700)
    table = rng.uniform(-6, 0, (3, 5)).astype(np.float32)
    clips = [_random_clip(T, N, 710 + N, 0, 4, p_row=0.0) for T, N in ((190, 40), (470, 300))]
    got = _run(clips, table)
    refs = []
    for (z, alts, _), g in zip(clips, got):
        pair = []
        for dt in (np.float64, np.float32):
            r = dict(P.forward_backward(z, alts, GAPS, tok=g["tok"], dtype=dt))
            f = FP.forward_backward(z, alts, GAPS, None, 1.0, tok=g["tok"], dtype=dt)
            r["end_mean"], r["end_sd"] = f["end_mean"], f["end_sd"]
            pair.append(r)
        refs.append(tuple(pair))
    _check_case("rows all -1", clips, table, got, refs=refs)


def test_a_hard_table_is_the_minimum_duration_posterior():
    """L(1 .. m - 1) = -inf, 0 from m on, tail 0: against duration_posterior_ref at minimum duration m."""
    rng = np.random.default_rng(720)
    table = np.zeros((8, 9), np.float32)
    for d in range(1, 9):
        table[d - 1, :d - 1] = NEG
    clips, mins = [], []
    for T, N in ((260, 40), (1400, 300)):
        z, alts, _ = _random_clip(T, N, 730 + N, 0, 8)
        m = rng.choice([1, 2, 3, 8], N)
        clips.append((z, alts, [int(x) - 1 for x in m]))
        mins.append(m)
    got = _run(clips, table)
    refs = [tuple(DPR.forward_backward(z, alts, GAPS, m, tok=g["tok"], dtype=dt) for dt in (np.float64, np.float32))
            for (z, alts, _), m, g in zip(clips, mins, got)]
    _check_case("minimum durations", clips, table, got, keys=("logz", "tok_post", "start_mean", "start_sd"), refs=refs)


# ------------------------------------------------------------------------------------------------ 4. small clips
def test_small_clips():
    rng = np.random.default_rng(740)
    D = 3
    table = rng.uniform(-3, 0, (4, D + 1)).astype(np.float32)
    table[3] = NEG                                           # a row that forbids every run
    healthy = _random_clip(60, 9, 741, 3, D)
    one_path = _random_clip(12, 12, 742, 3, D)               # T == N
    too_few = _random_clip(5, 7, 743, 3, D)                  # T < N
    z, alts, _ = _random_clip(30, 4, 744, 3, D)
    forbidden = (z, alts, [0, 3, 1, -1])
    single = _random_clip(1, 1, 745, 3, D)                   # N = 1, T = 1
    z = (rng.standard_normal((20, C)) * 1.5).astype(np.float32)
    z[:, 1:3] += 8.0                                         # the only token's classes win every frame: it runs to the clip's end in its tail
    to_the_end = (z, [[(1, 2)]], [0])
    clips = [healthy, one_path, too_few, forbidden, single, to_the_end]
    got = _run(clips, table)
    _check_case("small clips", clips, table, got)
    assert [g["status"] for g in got] == [0, 0, 1, 1, 0, 0]
    assert _same(got[0], _run([healthy], table)[0])          # beside the clips without a path
    g = got[1]
    assert np.abs(g["tok_post"] - 1).max() < 1e-5 and not any(g[k].any() for k in ("start_mean", "start_sd", "end_mean", "end_sd"))
    assert abs(got[4]["tok_post"][0] - 1) < 1e-5
    first, last = _ends(got[5]["tok"], 1)
    assert last[0] == 19 and last[0] - first[0] + 1 > D and got[5]["tok_post"][0] > 0.5


# ------------------------------------------------------------------------------------------------ 5. windows
def test_windows():
    rng = np.random.default_rng(750)
    D = 4
    table = rng.uniform(-4, 0, (6, D + 1)).astype(np.float32)
    table[2, :2] = NEG
    clips = [_random_clip(120, 20, 751, 6, D), _random_clip(400, 150, 752, 6, D), _random_clip(90, 12, 753, 6, D)]
    args = _upload(clips)
    _, tok, _, _ = AL.viterbi_align_duration_prior(*args, [c[2] for c in clips], table)
    free = _split(clips, tok, torch.zeros(3), torch.zeros(3), AL.duration_prior_posteriors(*args, [c[2] for c in clips], table, tok))
    wins = []
    for b, (c, g) in enumerate(zip(clips, free)):
        first, _ = _ends(g["tok"], len(c[1]))
        if b == 0:                                           # wide windows, so that one of them can shut its token's own start out
            wins.append([(int(a) - 10, int(a) + 10) for a in first])
            continue
        lo = first - rng.integers(0, 4, len(first))
        wins.append([(int(a), int(a) + int(w)) for a, w in zip(lo, rng.integers(3, 9, len(first)))])
    first0, _ = _ends(free[0]["tok"], 20)
    wins[0][5] = (int(first0[5]) + 2, int(first0[5]) + 12)   # the unwindowed start is outside: the search moves
    wins[2][4] = (7, 3)                                      # an empty window: no path
    got = _run(clips, table, windows=wins)
    _check_case("windows", clips, table, got, windows=wins)
    assert [g["status"] for g in got] == [0, 0, 1]
    assert not _same(got[0], free[0])
    # a tok that opens a token outside its window is no path of the windowed lattice
    moved = _run(clips[:1], table, windows=[[(a + 40, b + 40) for a, b in wins[0]]], search_table=table,
                 tok_edit=lambda t: torch.from_numpy(free[0]["tok"]).cuda())
    assert moved[0]["status"] in (1, 8) and _zeros(moved[0])


# ------------------------------------------------------------------------------------------------ 6. score <= logz
def test_a_paths_weight_is_part_of_the_sum():
    rng = np.random.default_rng(760)
    D = 5
    table = rng.uniform(-6, 0, (8, D + 1)).astype(np.float32)
    table[:, D] = rng.uniform(-1, 0, 8)
    clips = [_random_clip(N + 90, N, 761 + N, 8, D, scale=s) for N, s in ((30, 1.0), (200, 3.0), (600, 2.0))]
    got = _run(clips, table)
    r64s = _check_case("score <= logz", clips, table, got)
    for b, (g, r) in enumerate(zip(got, r64s)):
        yard = abs(REFS[("score <= logz", b)][1]["logz"] - r["logz"])
        slack = 4 * yard + 1e-3 * len(g["tok"])             # the search's own bound on `score`: 1e-3 per frame
        print(f"score {g['score']:.4f} logz {g['logz'][0]:.4f} slack {slack:.3e}")
        assert g["score"] <= g["logz"][0] + slack


# ------------------------------------------------------------------------------------------------ 7. statuses
def test_statuses_beside_a_healthy_clip():
    rng = np.random.default_rng(770)
    D = 4
    table = rng.uniform(-4, 0, (5, D + 1)).astype(np.float32)
    healthy = _random_clip(200, 60, 771, 5, D)
    solo = _run([healthy], table)[0]
    assert solo["status"] == 0
    # 4: a row out of range
    z, alts, rows = _random_clip(80, 10, 772, 5, D)
    bad_row = (z, alts, rows[:3] + [5] + rows[4:])
    got = _run([healthy, bad_row], table)
    assert got[1]["status"] == 4 and got[1]["vstatus"] == 4 and _zeros(got[1]) and _same(got[0], solo)
    # 8: a token erased from tok
    other = _random_clip(80, 10, 773, 5, D)

    def erase(tok):
        seg = tok[200:280]
        seg[seg == 4] = -1
        return tok
    got = _run([healthy, other], table, tok_edit=erase)
    assert got[1]["status"] == 8 and _zeros(got[1]) and _same(got[0], solo)

    def out_of_range(tok):
        tok[205] = 10
        return tok
    got = _run([healthy, other], table, tok_edit=out_of_range)
    assert got[1]["status"] == 8 and _zeros(got[1]) and _same(got[0], solo)
    # 8: tok from a search under another table, so that a run has a length this table forbids
    strict = table.copy()
    strict[:, 0] = NEG                                       # no run of one frame
    z, alts, _ = _random_clip(80, 10, 774, 5, D)
    rowed = (z, alts, [k % 5 for k in range(10)])
    loose = _run([rowed], table)[0]
    first, last = _ends(loose["tok"], 10)
    assert (last - first == 0).any(), "the other table's search gave no run of one frame"
    got = _run([healthy, rowed], strict, search_table=table)
    assert got[1]["vstatus"] == 0 and got[1]["status"] == 8 and _zeros(got[1])
    # (the healthy clip is scored under `strict` there; its own tok may hold a run of one frame, so only its neighbour is judged)
    # 2: N = 4097
    rng2 = np.random.default_rng(775)
    big = ((rng2.standard_normal((4200, C))).astype(np.float32), [[(1, 2)], [(3, 4)]] * 2048 + [[(5, 6)]], [-1] * 4097)
    got = _run([healthy, big], table)
    assert got[1]["status"] == 2 and _zeros(got[1]) and _same(got[0], solo)


# ------------------------------------------------------------------------------------------------ 8. alone = in a ragged batch
def test_alone_equals_in_a_ragged_batch():
    rng = np.random.default_rng(780)
    D = 6
    table = rng.uniform(-6, 0, (8, D + 1)).astype(np.float32)
    sizes = [(90, 30), (300, 140), (40, 3), (700, 520), (128, 60), (33, 33), (257, 100), (1, 1), (512, 127), (513, 128), (60, 0), (900, 511),
             (1400, 1024), (150, 70), (5, 9), (220, 90)]
    clips = [_random_clip(T, N, 781 + i, 8, D) for i, (T, N) in enumerate(sizes)]
    assert len(clips) == 16
    got = _run(clips, table)
    for b in (1, 3, 12):
        assert got[b]["status"] == 0 and _same(got[b], _run([clips[b]], table)[0]), b
    assert got[14]["status"] == 1 and got[10]["status"] == 0


def test_a_large_batch_runs_in_groups_under_the_workspace_limit(monkeypatch):
    rng = np.random.default_rng(785)
    D = 6
    table = rng.uniform(-6, 0, (8, D + 1)).astype(np.float32)
    sizes = [(90, 30), (300, 140), (5, 9), (257, 100), (40, 3), (150, 70)]
    clips = [_random_clip(T, N, 786 + i, 8, D) for i, (T, N) in enumerate(sizes)]
    whole = _run(clips, table)
    need = [AL.duration_prior_posterior_workspace_bytes([T], [N], D) for T, N in sizes]
    monkeypatch.setattr(AL, "EDITS_WORKSPACE_LIMIT", need[0] + need[1] + 1)          # the first two clips together, not all six
    assert len(AL.edit_groups([t for t, _ in sizes], [n for _, n in sizes],
                              workspace_bytes=lambda t, n: AL.duration_prior_posterior_workspace_bytes(t, n, D))) >= 2
    grouped = _run(clips, table)
    assert [g["status"] for g in whole] == [0, 0, 1, 0, 0, 0]
    for b, (w, g) in enumerate(zip(whole, grouped)):
        assert _same(w, g), b


# ------------------------------------------------------------------------------------------------ 9. C = 1024
def test_one_row_per_stage():
    rng = np.random.default_rng(790)
    D = 4
    table = rng.uniform(-4, 0, (5, D + 1)).astype(np.float32)
    T, N = 150, 60
    z = (rng.standard_normal((T, 1024)) * 2).astype(np.float32)
    alts = [[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 500, N)]
    rows = [int(r) for r in rng.integers(-1, 5, N)]
    gaps = [0, 1021, 1022]
    lg = torch.from_numpy(z).cuda()
    _, tok, score, vst = AL.viterbi_align_duration_prior(lg, [T], [alts], [gaps], 0, [rows], table)
    out = AL.duration_prior_posteriors(lg, [T], [alts], [gaps], 0, [rows], table, tok)
    torch.cuda.synchronize()
    g = _split([(z, alts, rows)], tok, vst, score, out)[0]
    assert g["status"] == 0
    r64 = PR.forward_backward(z, alts, gaps, rows, table, tok=g["tok"])
    r32 = PR.forward_backward(z, alts, gaps, rows, table, tok=g["tok"], dtype=np.float32)
    for k in KEYS:
        ref = np.atleast_1d(np.asarray(r64[k], np.float64))
        yard = float(np.abs(np.atleast_1d(r32[k]) - ref).max())
        d = np.abs(g[k].astype(np.float64) - ref)
        h = _half_ulp(ref)
        print(f"C = 1024: {k}: kernel {d.max():.3e}, float32 restatement {yard:.3e}")
        assert (d <= 4 * yard + np.where(yard < h, h, 0.0)).all(), k


# ------------------------------------------------------------------------------------------------ 10. the C entry on device pointers
def test_the_entry_refuses_on_device_pointers():
    from wfl_asr_amd import _lib
    lib = _lib.load()
    T, N, D = 50, 8, 4
    z, alts, rows = _random_clip(T, N, 795, 3, D)
    table = np.random.default_rng(796).uniform(-3, 0, (3, D + 1)).astype(np.float32)
    lg = torch.from_numpy(z).cuda()
    packed = AL.pack_clips(lg, [T], [alts], [GAPS], None, None)
    _, tok, _, _ = AL.viterbi_align_duration_prior(lg, [T], [alts], [GAPS], O_ID, [rows], table, packed=packed)
    d_tab = torch.from_numpy(table).cuda()
    d_dur = AL.upload_durations([rows], packed.N, lg.device)
    need = AL.duration_prior_posterior_workspace_bytes([T], [N], D)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    outs = [torch.full((max(N, 1),), 7.0, device="cuda") for _ in range(6)]
    st = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
    h = lambda a: a.ctypes.data_as(ctypes.c_void_p)                             # noqa: E731

    def call(ws_bytes=need, dur=d_dur, tab=d_tab, D_=D, end_mean=outs[4]):
        return lib.wfl_align_duration_prior_posterior(p(lg), lg.stride(0), C, O_ID, h(packed.F0), h(packed.T), h(packed.K0), h(packed.N),
                                                      p(packed.d_tc), None, p(packed.d_gc), 1, p(dur), p(tab), 3, D_, p(tok), p(ws),
                                                      ws_bytes, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), p(end_mean), p(outs[5]),
                                                      p(st), None)
    for kw, what in ((dict(ws_bytes=need - 1), b"workspace"), (dict(dur=None), b"null tok_dur"), (dict(tab=None), b"null dur"),
                     (dict(end_mean=None), b"null device pointer"), (dict(D_=0), b"D must be 1 .. 32"), (dict(D_=33), b"D must be 1 .. 32")):
        assert call(**kw) < 0 and what in lib.wfl_last_error(), kw
    torch.cuda.synchronize()
    assert int(st[0]) == 77 and all(float(o[0]) == 7.0 for o in outs)      # nothing was launched after a refusal
    assert call() == 0
    torch.cuda.synchronize()
    assert int(st[0]) == 0 and float(outs[1][0]) != 7.0
