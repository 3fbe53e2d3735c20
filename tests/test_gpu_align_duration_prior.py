"""-m gpu: wfl_align_duration_prior (csrc/align_duration_prior.hip) against the float64 explicit-duration DP of
tests/viterbi_duration_prior_ref.py.  C = 141, logits standard_normal * 3, one ragged batch per test, one clip per configuration:
N in (3, 128, 512, 1024, 2048) at T = N + 150.

Bounds, those of tests/test_gpu_align_min_duration.py: the kernel's path is legal, its float64 score -- emissions plus prior -- is >=
the float64 optimum - 1e-3, and `score` is within 1e-3 T of the optimum.

The random tables: entries uniform in [-6, 0], tails uniform in [-1, 0], about one value in ten -inf.  Independent -inf entries alone
never make a run of D or more frames the optimum on random logits (an I frame scores about 2.5 nats below a gap frame), so the -inf
values are placed in two ways: independently in the 36 soft rows (one in 25), and as the whole prefix L(1) .. L(D - 1) of four hard rows,
two of which also have a tail of -inf (a run of exactly D frames) and two a finite tail (D frames or more).  The hard rows go to the
two tokens at a few thread boundaries (k = i R - 1 the exact one, k = i R the one with a tail), as the sibling test places its largest
minimum durations; every other token draws a soft row or, one in two, none.  The tokens with a tail have four alternatives: L(d)
never grows beyond D, so only the emissions make a run longer than D, and one I class seldom beats three gap classes."""
import numpy as np
import pytest
import torch

import viterbi_duration_prior_ref as DP
import viterbi_min_ref as M
import viterbi_ref as V
import viterbi_window_ref as W
from wfl_asr_amd import align as AL

pytestmark = pytest.mark.gpu
C = 141
O_ID = 0
GAPS = [O_ID, 137, 138]
SIZES = (3, 128, 512, 1024, 2048)
R_OF = {3: 2, 40: 2, 128: 2, 512: 4, 1024: 8, 2048: 9}    # slots per thread of the configuration that takes N tokens (csrc/lattice.h)
STAGE_OF = {3: 7, 40: 7, 128: 29, 512: 29, 1024: 29, 2048: 29}   # logits rows per stage there: min(32, threads x staged values / C)
ALIGN_W, RENORM = 32, 16                                  # the kernel's backtrace window, csrc/lattice.h's renormalisation period
NEG = -np.inf
WORST = {"path": 0.0, "score_per_frame": 0.0}             # the worst deviations seen, printed by every check


def _alts(N, rng):
    return [[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 68, N)]


def _logits(T, rng):
    return rng.standard_normal((T, C)).astype(np.float32) * 3


def _run(clips, rows, table, windows=None, gaps=GAPS, plain=False):
    """clips: [(z, alternatives)]; rows: one list (or None) per clip -> per clip a dict of numpy outputs.  plain: wfl_align itself."""
    T = [len(c[0]) for c in clips]
    lg = torch.from_numpy(np.ascontiguousarray(np.concatenate([c[0] for c in clips]))).cuda()
    args = (lg, T, [c[1] for c in clips], [gaps] * len(clips), O_ID)
    if plain:
        ids, tok, score, status = AL.viterbi_align(*args, windows=windows)
    else:
        ids, tok, score, status = AL.viterbi_align_duration_prior(*args, rows, table, windows=windows)
    torch.cuda.synchronize()
    ids, tok, score, status = (x.cpu().numpy() for x in (ids, tok, score, status))
    out, pos = [], 0
    for b, t in enumerate(T):
        out.append(dict(ids=ids[pos:pos + t], tok=tok[pos:pos + t], score=score[b:b + 1], status=int(status[b])))
        pos += t
    return out


def _states(ids, tok):
    """(ids, tok) -> the state sequence the kernel walked (the B classes are the odd ones here)."""
    s = np.zeros(len(ids), np.int64)
    done = 0
    for t in range(len(ids)):
        k = int(tok[t])
        if k < 0:
            s[t] = 3 * done
        else:
            s[t] = 3 * k + (1 if int(ids[t]) % 2 == 1 else 2)
            done = k + 1
    return s


def _same(a, b):
    return (a["status"] == b["status"] and (a["ids"] == b["ids"]).all() and (a["tok"] == b["tok"]).all()
            and a["score"].tobytes() == b["score"].tobytes())


def _check_against_dp(g, z, alts, rows, table, ref_score, what, windows=None, gaps=GAPS):
    T, N = len(z), len(alts)
    assert g["status"] == 0, what
    states = _states(g["ids"], g["tok"])
    assert V.legal(states, N), f"{what}: the kernel's path is not a legal path"
    rid, rtok = V.outputs(states, z, alts, O_ID)
    assert (rid == g["ids"]).all() and (rtok == g["tok"]).all(), f"{what}: ids / tok are not the path's classes"
    mine = DP.path_score(states, z, alts, gaps, rows, table, windows)
    WORST["path"] = max(WORST["path"], ref_score - mine)
    WORST["score_per_frame"] = max(WORST["score_per_frame"], abs(float(g["score"][0]) - ref_score) / T)
    print(f"{what}: T {T} N {N}: path score {mine:.4f}, reference {ref_score:.4f}, kernel score {g['score'][0]:.4f}; worst so far: path "
          f"{WORST['path']:.3e} below the optimum, score {WORST['score_per_frame']:.3e} per frame off")
    assert mine >= ref_score - 1e-3, (what, mine, ref_score)
    assert abs(float(g["score"][0]) - ref_score) <= 1e-3 * T, (what, g["score"], ref_score)
    return states


@pytest.fixture(scope="module")
def plain_clips():
    """The five clips every test but the D = 32 one runs on, and wfl_align's own output for them."""
    rng = np.random.default_rng(91)
    clips = [(_logits(N + 150, rng), _alts(N, rng)) for N in SIZES]
    return clips, _run(clips, None, None, plain=True)


# ------------------------------------------------------------------------------------------------ 1. no prior
def test_without_a_prior_the_search_is_wfl_aligns(plain_clips):
    clips, plain = plain_clips
    assert all(p["status"] == 0 for p in plain)
    rng = np.random.default_rng(92)
    some = rng.uniform(-6, 0, (5, 4)).astype(np.float32)
    none = [[-1] * len(alts) for _, alts in clips]
    none[1] = None                                        # a clip's None, and spelled out
    zero = np.zeros((2, 33), np.float32)                  # D = 32: the ring of the two largest clips lives in the workspace
    zrows = [[k % 2 for k in range(len(alts))] for _, alts in clips]
    for what, rows, table in (("every row -1", none, some), ("an all-zero table", zrows, zero)):
        got = _run(clips, rows, table)
        for b, ((z, alts), p, g) in enumerate(zip(clips, plain, got)):
            T = len(z)
            assert g["status"] == p["status"] == 0
            sg, sp = _states(g["ids"], g["tok"]), _states(p["ids"], p["tok"])
            assert V.legal(sg, len(alts))
            a, c = V.path_score(sg, z, alts, GAPS), V.path_score(sp, z, alts, GAPS)
            print(f"{what}: T {T} N {len(alts)}: path score {a:.4f}, wfl_align's {c:.4f}; score {g['score'][0]:.4f}, {p['score'][0]:.4f}")
            assert abs(a - c) <= 1e-3 and abs(float(g["score"][0]) - c) <= 1e-3 * T
            alone = _run([clips[b]], [rows[b]], table)[0]
            assert _same(alone, g), (what, b)


# ------------------------------------------------------------------------------------------------ 2. against the float64 DP, D = 3 and 8
def _random_table(D, rng):
    """-> (table [40, D + 1], the exact row, the row with a tail): see the module's docstring."""
    t = rng.uniform(-6, 0, (40, D + 1))
    t[:, D] = rng.uniform(-1, 0, 40)
    t[:36][rng.random((36, D + 1)) < 0.04] = NEG
    t[36:, :D - 1] = NEG
    t[36:38, D] = NEG
    return t.astype(np.float32), (36, 37), (38, 39)


def _straddles(start, end, T, F):
    """Whether the frames start .. end of a run cross a backtrace window (counted from T - 1), a renormalisation and a logits stage
    boundary."""
    return ((T - 1 - start) // ALIGN_W != (T - 1 - end) // ALIGN_W, start // RENORM != end // RENORM, start // F != end // F)


def _draw_case(N, D, rng):
    """-> (z, alternatives, rows, table, the exact rows).  The tokens that get a row with a tail also get four alternatives, so that
    their I frames beat the gap's three classes often enough for the tail to be walked."""
    T, R = N + 150, R_OF[N]
    alts, z = _alts(N, rng), _logits(T, rng)
    table, exact, tailed = _random_table(D, rng)
    rows = np.where(rng.random(N) < 0.5, -1, rng.integers(0, 36, N))
    k = np.arange(N)
    th = k // R
    n_b = max(1, min(6, 60 // (2 * (D - 1))))                                 # thread boundaries: their two hard rows take at most 60
    pick = np.unique(np.linspace(1, max(N // R - 1, 1), n_b).astype(int))      # of the clip's 150 spare frames
    last, first = (k % R == R - 1) & np.isin(th + 1, pick), (k % R == 0) & np.isin(th, pick) & (k > 0)
    rows[last] = rng.choice(exact, size=int(last.sum()))
    rows[first] = rng.choice(tailed, size=int(first.sum()))
    for q in k[first]:
        alts[q] = [(int(2 * p - 1), int(2 * p)) for p in rng.choice(np.arange(1, 68), size=4, replace=False)]
    return z, alts, rows, table, exact


def _dp_case(N, D, seed0):
    """The first seed from seed0 on whose references meet the setup (the kernel is not consulted): the prior's optimum is not the plain
    one; some run is longer than D, some has exactly D frames, some token whose tail is -inf sits at exactly D; of the runs of D or
    more frames some is at a thread's last slot and some at a thread's first, and some straddles a backtrace window, some a
    renormalisation, some a logits stage boundary (the three tokens of the smallest clip cannot do all that: there the batch's other
    clips do, and the test asserts it over the batch)."""
    T, R, F = N + 150, R_OF[N], STAGE_OF[N]
    k = np.arange(N)
    for seed in range(seed0, seed0 + 40):
        z, alts, rows, table, exact = _draw_case(N, D, np.random.default_rng(seed))
        ref = DP.viterbi(z, alts, GAPS, rows, table)
        if ref is None:
            continue
        states, ref_score, runs = ref
        free, _ = V.viterbi(z, alts, GAPS)
        long_ = runs >= D
        exact_hit = np.isin(rows, exact) & (runs == D)
        starts = W.starts(states, N)
        hit = np.array([_straddles(int(starts[q]), int(starts[q] + runs[q] - 1), T, F) for q in k[long_]])
        if ((free != states).any() and (runs > D).any() and (runs == D).any() and exact_hit.any() and (long_ & (k % R == R - 1)).any()
                and (long_ & (k % R == 0) & (k > 0)).any() and len(hit) and (N < 128 or hit.any(axis=0).all())):
            print(f"D {D} N {N}: seed {seed}, {int((runs > D).sum())} runs longer than D, {int((runs == D).sum())} of exactly D, "
                  f"straddling runs {hit.sum(axis=0).tolist()}")
            return z, alts, rows.tolist(), table, ref, hit.any(axis=0)
    raise AssertionError(f"no seed meets the setup for D {D} N {N} (test setup)")


@pytest.fixture(scope="module", params=[3, 8])
def dp_cases(request):
    D = request.param
    return [_dp_case(N, D, 1000 * D + 100 * j) for j, N in enumerate(SIZES)]


def test_against_the_float64_dp(dp_cases):
    tables = {id(c[3]) for c in dp_cases}
    assert len(tables) == len(dp_cases)                   # (every clip drew its own table: one call per clip's table, one ragged batch
    table = np.concatenate([c[3] for c in dp_cases])      # over the tables stacked, the rows shifted)
    shift = np.cumsum([0] + [len(c[3]) for c in dp_cases])
    rows = [[r + int(shift[b]) if r >= 0 else -1 for r in c[2]] for b, c in enumerate(dp_cases)]
    got = _run([(c[0], c[1]) for c in dp_cases], rows, table)
    assert np.all([c[5] for c in dp_cases if len(c[1]) >= 128])
    for (z, alts, r, tab, (states, ref_score, runs), _), g in zip(dp_cases, got):
        assert V.legal(states, len(alts)) and abs(DP.path_score(states, z, alts, GAPS, r, tab) - ref_score) < 1e-6
        _check_against_dp(g, z, alts, r, tab, ref_score, f"random table, D {tab.shape[1] - 1}")


# ------------------------------------------------------------------------------------------------ 3. D = 32: long runs
def test_long_runs_at_d_32():
    """The table rewards long runs: -12 below 20 frames, rising to 0 at 25, tail -0.05.  One gap class here, so that a token's I frame
    and a gap frame score alike on random logits and the prior decides the lengths."""
    d = np.arange(1, 33)
    row = np.where(d < 20, -12.0, np.where(d >= 25, 0.0, -12.0 + 2.0 * (d - 19)))
    table = np.concatenate([row, [-0.05]]).astype(np.float32)[None]
    rows = [[0] * 3, [0 if k % 5 else -1 for k in range(40)]]
    for seed in range(930, 970):                          # the first seed whose references hold runs of 25 to 60 frames and a walked tail
        rng = np.random.default_rng(seed)
        clips = [(_logits(400, rng), _alts(N, rng)) for N in (3, 40)]
        refs = [DP.viterbi(z, alts, [O_ID], r, table) for (z, alts), r in zip(clips, rows)]
        if all(((runs >= 25) & (runs <= 60)).any() and (runs > 32).any() for _, _, runs in refs):
            break
    else:
        raise AssertionError("no run of 25 to 60 frames in the references (test setup)")
    for _, _, runs in refs:
        print("seed", seed, "runs", runs.tolist())
        assert ((runs >= 25) & (runs <= 60)).any() and (runs > 32).any()
    got = _run(clips, rows, table, gaps=[O_ID])
    for (z, alts), r, (states, ref_score, runs), g in zip(clips, rows, refs, got):
        _check_against_dp(g, z, alts, r, table, ref_score, "long runs, D 32", gaps=[O_ID])


# ------------------------------------------------------------------------------------------------ 4. a hard table is min_duration
def test_a_hard_table_is_min_duration(plain_clips):
    clips, _ = plain_clips
    table = np.zeros((600, 9), np.float32)                # row d - 1: -inf below d frames, 0 from there on, tail 0; 600 rows: more than
                                                          # the kernel stages in LDS, so this table is read through the caches
    for d in range(1, 9):
        table[d - 1, :d - 1] = NEG
    rng = np.random.default_rng(94)
    mins, refs = [], []
    for z, alts in clips:
        N, T = len(alts), len(z)
        D = rng.choice([1, 2, 3, 8], size=N, p=[0.6, 0.2, 0.15, 0.05])
        while D.sum() > T - 50:
            D[int(rng.integers(0, N))] = 1
        mins.append(D)
        refs.append(M.viterbi(z, alts, GAPS, D))
    got = _run(clips, [(D - 1).tolist() for D in mins], table)
    for (z, alts), D, (ref, ref_score), g in zip(clips, mins, refs, got):
        assert ref is not None
        states = _check_against_dp(g, z, alts, (D - 1).tolist(), table, ref_score, "hard minimum")
        assert (DP.run_lengths(states, len(alts)) >= D).all()
        assert V.path_score(states, z, alts, GAPS) >= ref_score - 1e-3


# ------------------------------------------------------------------------------------------------ 5. a hard maximum
def test_a_tail_of_minus_infinity_is_a_hard_maximum(plain_clips):
    clips, _ = plain_clips
    D = 2
    table = np.array([[-0.5, -0.25, NEG]], np.float32)
    longer = 0
    refs = []
    for z, alts in clips:
        longer += int((DP.run_lengths(V.viterbi(z, alts, GAPS)[0], len(alts)) > D).sum())
        refs.append(DP.viterbi(z, alts, GAPS, [0] * len(alts), table))
    assert longer > 0 and all(r is not None and (r[2] <= D).all() for r in refs), "test setup"
    got = _run(clips, [[0] * len(alts) for _, alts in clips], table)
    for (z, alts), (_, ref_score, _), g in zip(clips, refs, got):
        states = _check_against_dp(g, z, alts, [0] * len(alts), table, ref_score, "hard maximum")
        assert (DP.run_lengths(states, len(alts)) <= D).all()


# ------------------------------------------------------------------------------------------------ 6. windows
def test_inside_start_windows(dp_cases):
    """+-3 frames around the starts of the unwindowed reference, every seventh token pinned."""
    wins, refs = [], []
    for z, alts, r, tab, (states, _, _), _ in dp_cases:
        s = W.starts(states, len(alts))
        w = [(int(x), int(x)) if k % 7 == 0 else (int(x) - 3, int(x) + 3) for k, x in enumerate(s)]
        wins.append(w)
        refs.append(DP.viterbi(z, alts, GAPS, r, tab, windows=w))
    table = np.concatenate([c[3] for c in dp_cases])
    shift = np.cumsum([0] + [len(c[3]) for c in dp_cases])
    rows = [[r + int(shift[b]) if r >= 0 else -1 for r in c[2]] for b, c in enumerate(dp_cases)]
    got = _run([(c[0], c[1]) for c in dp_cases], rows, table, windows=wins)
    for (z, alts, r, tab, _, _), w, ref, g in zip(dp_cases, wins, refs, got):
        assert ref is not None
        states = _check_against_dp(g, z, alts, r, tab, ref[1], "windowed", windows=w)
        assert W.in_windows(states, w)


# ------------------------------------------------------------------------------------------------ 7. no path beside paths
def test_clips_without_a_path_beside_clips_with_one():
    rng = np.random.default_rng(95)
    table = rng.uniform(-6, 0, (4, 5)).astype(np.float32)
    table[3] = NEG                                        # a row that forbids every duration
    clips = [(_logits(60, rng), _alts(6, rng)), (_logits(70, rng), _alts(5, rng)), (_logits(300, rng), _alts(130, rng)),
             (_logits(50, rng), _alts(4, rng)), (_logits(20, rng), _alts(30, rng))]
    rows = [[0, 1, 2, -1, 0, 1], [0, 1, 3, 1, 0], [k % 3 for k in range(130)], [0, 4, 1, 2], [0] * 30]
    want = [0, 1, 0, 4, 1]                                # (the last: fewer frames than tokens)
    got = _run(clips, rows, table)
    for b, g in enumerate(got):
        assert g["status"] == want[b], b
        if want[b]:
            assert (g["ids"] == O_ID).all() and (g["tok"] == -1).all() and g["score"][0] == 0
            continue
        alone = _run([clips[b]], [rows[b]], table)[0]
        assert _same(alone, g), b
        z, alts = clips[b]
        _check_against_dp(g, z, alts, rows[b], table, DP.viterbi(z, alts, GAPS, rows[b], table)[1], f"clip {b}")
    assert DP.viterbi(clips[1][0], clips[1][1], GAPS, rows[1], table) is None
