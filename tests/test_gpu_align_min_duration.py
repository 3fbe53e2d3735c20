"""-m gpu: wfl_align_min_duration (csrc/align.hip with MIND; the chain is csrc/lattice.h chain_out / chain_shift) against the float64
DP over the expanded states of tests/viterbi_min_ref.py.  C = 141, one ragged batch per test.

Bounds, those of tests/test_gpu_align.py at its T range: the kernel's path is legal, every run has at least D_k frames, its float64
score is >= the constrained float64 optimum - 1e-3 and `score` is within 1e-3 T of it."""
import numpy as np
import pytest
import torch

import viterbi_min_ref as M
import viterbi_ref as V
import viterbi_window_ref as W
from wfl_asr_amd import align as AL

pytestmark = pytest.mark.gpu
C = 141
O_ID = 0
GAPS = [O_ID, 137, 138]
R_OF = {3: 2, 128: 2, 512: 4, 1024: 8, 2048: 9}           # slots per thread of the configuration that takes N tokens (csrc/lattice.h)
STAGE_OF = {3: 7, 128: 29, 512: 29, 1024: 29, 2048: 29}   # logits rows per stage there: min(32, threads x staged values / C)
ALIGN_W, RENORM = 32, 16                                  # csrc/align.hip's backtrace window, csrc/lattice.h's renormalisation period


def _alts(N, rng):
    return [[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 68, N)]


def _run(clips, windows=None, min_frames=None):
    """clips: [(z, alternatives)]; windows / min_frames: None or one entry per clip -> per clip a dict of numpy outputs."""
    T = [len(c[0]) for c in clips]
    lg = torch.from_numpy(np.ascontiguousarray(np.concatenate([c[0] for c in clips]))).cuda()
    ids, tok, score, status = AL.viterbi_align(lg, T, [c[1] for c in clips], [GAPS] * len(clips), O_ID, windows=windows,
                                               min_frames=min_frames)
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


def _check_against_dp(g, z, alts, D, ref_score, what):
    T, N = len(z), len(alts)
    assert g["status"] == 0, what
    states = _states(g["ids"], g["tok"])
    assert V.legal(states, N), f"{what}: the kernel's path is not a legal path"
    assert (M.run_lengths(states, N) >= D).all(), f"{what}: a run is shorter than its minimum duration"
    mine = V.path_score(states, z, alts, GAPS)
    print(f"{what}: T {T} N {N}: path score {mine:.4f}, reference {ref_score:.4f}, kernel score {g['score'][0]:.4f}")
    assert mine >= ref_score - 1e-3, (what, mine, ref_score)
    assert abs(float(g["score"][0]) - ref_score) <= 1e-3 * T, (what, g["score"], ref_score)
    return states


# ------------------------------------------------------------------------------------------------ 1. all ones: bit for bit
def test_all_ones_are_bit_identical_to_the_entries_without_durations():
    rng = np.random.default_rng(81)
    clips = []
    for N in (3, 128, 512, 1024, 2048):                   # one clip per configuration; T = N + 150 spans several logits stages, more
        T = N + 150                                       # than one renormalisation and backtrace window
        clips.append((rng.standard_normal((T, C)).astype(np.float32) * 3, _alts(N, rng)))
    ones = [None, [1] * 128, None, [1] * 1024, [1] * 2048]      # a clip's None, and spelled out
    plain = _run(clips)
    assert all(p["status"] == 0 for p in plain)
    for a, b in zip(plain, _run(clips, min_frames=ones)):
        assert _same(a, b)
    # and inside windows that hold: +-3 frames around the starts of the path above, every seventh token pinned
    wins = []
    for p, (z, alts) in zip(plain, clips):
        s = W.starts(_states(p["ids"], p["tok"]), len(alts))
        wins.append([(int(x), int(x)) if k % 7 == 0 else (int(x) - 3, int(x) + 3) for k, x in enumerate(s)])
    windowed = _run(clips, windows=wins)
    assert all(p["status"] == 0 for p in windowed)
    for a, b in zip(windowed, _run(clips, windows=wins, min_frames=ones)):
        assert _same(a, b)


# ------------------------------------------------------------------------------------------------ 2. against the float64 DP
def _straddles(start, d, T, F):
    """Whether the opening d frames start .. start + d - 1 of a run cross a backtrace window (counted from T - 1), a renormalisation
    and a logits stage boundary."""
    end = start + d - 1
    return ((T - 1 - start) // ALIGN_W != (T - 1 - end) // ALIGN_W, start // RENORM != end // RENORM, start // F != end // F)


def _dp_case(T, N, draw, seed0):
    """Random logits x 3 and durations drawn by `draw(rng, N, unconstrained run lengths)`; the first seed from seed0 on whose references
    meet the setup: the unconstrained optimum violates D_k at a token k = i R - 1 and at a token k = i R with D_k >= 3, and in the
    constrained optimum the opening D_k frames of some run with D_k >= 3 straddle a backtrace window, of some a renormalisation, of
    some a logits stage boundary.  (References alone; the kernel is not consulted.)"""
    R, F = R_OF[N], STAGE_OF[N]
    for seed in range(seed0, seed0 + 40):
        rng = np.random.default_rng(seed)
        alts = _alts(N, rng)
        z = rng.standard_normal((T, C)).astype(np.float32) * 3
        free, _ = V.viterbi(z, alts, GAPS)
        runs = M.run_lengths(free, N)
        D = np.asarray(draw(rng, N, runs), np.int64)
        k = np.arange(N)
        viol = (D >= 3) & (runs < D)
        if not ((viol & (k % R == R - 1)).any() and (viol & (k % R == 0) & (k > 0)).any()) or D.sum() > T:
            continue
        ref, ref_score = M.viterbi(z, alts, GAPS, D)
        if ref is None:
            continue
        starts = W.starts(ref, N)
        hit = np.array([_straddles(int(starts[q]), int(D[q]), T, F) for q in k[D >= 3]])
        if len(hit) and hit.any(axis=0).all():
            print(f"T {T} N {N}: seed {seed}, {int((runs == 1).sum())} one-frame runs in the unconstrained optimum, {int((D > 1).sum())} "
                  f"tokens with D > 1 (sum D {int(D.sum())}), {int(viol.sum())} of them violated by it, straddling runs "
                  f"{hit.sum(axis=0).tolist()}")
            return z, alts, D, ref, ref_score
    raise AssertionError(f"no seed meets the setup for T {T} N {N} (test setup)")


def _draw_from(values, p):
    def draw(rng, N, runs):
        R = R_OF[N]
        D = rng.choice(values, size=N, p=p)
        k = np.arange(N)
        # at every eighth thread boundary both neighbours get D >= 3, one of them the largest value
        edge = (k % R == R - 1) & ((k // R) % 8 == 0) | (k % R == 0) & ((k // R) % 8 == 1) & (k > 0)
        D[edge] = np.where(k[edge] % R == 0, values[-1], 3)
        return D
    return draw


def _draw_1024(rng, N, runs):
    D = _draw_from([1, 2, 3], [1 / 3] * 3)(rng, N, runs)
    while D.sum() > 2300 - 150:                           # sum D <= T - 150
        D[int(rng.integers(0, N))] = 1
    return D


def _draw_2048(rng, N, runs):
    """All 1 except about 20 tokens at k = i R - 1, k = i R and in the middle of a thread's slots, D in {2, 3, 8}."""
    R = R_OF[N]
    D = np.ones(N, np.int64)
    for j, i in enumerate(rng.choice(np.arange(1, N // R), size=7, replace=False)):
        D[i * R - 1] = (3, 8, 2)[j % 3]
        D[i * R] = (8, 3, 3)[j % 3]
        D[i * R + R // 2] = (2, 8, 3)[j % 3]
    return D


DP_CASES = [(40, 3, _draw_from([1, 2, 3, 8], [0.1, 0.1, 0.4, 0.4])), (534, 128, _draw_from([1, 2, 3, 8], [0.4, 0.25, 0.25, 0.1])),
            (1700, 512, _draw_from([1, 2, 3, 8], [0.4, 0.25, 0.25, 0.1])), (2300, 1024, _draw_1024), (2300, 2048, _draw_2048)]


@pytest.fixture(scope="module")
def dp_cases():
    return [_dp_case(T, N, draw, 900 + 100 * j) for j, (T, N, draw) in enumerate(DP_CASES)]


def test_against_the_float64_dp(dp_cases):
    got = _run([(c[0], c[1]) for c in dp_cases], min_frames=[c[2].tolist() for c in dp_cases])
    for (z, alts, D, ref, ref_score), g in zip(dp_cases, got):
        assert V.legal(ref, len(alts)) and (M.run_lengths(ref, len(alts)) >= D).all()
        _check_against_dp(g, z, alts, D, ref_score, "random logits")


# ------------------------------------------------------------------------------------------------ 3. planted
def test_planted_path_and_raised_durations():
    """viterbi_ref.plant at T ~ 3 N leaves no gap frame, so every D_k at its planted run's length sums to T: the two frames a raised
    token needs come from its outer neighbour (k = i R - 2 and k = i R + 1), whose D goes to 1 for the second run."""
    rng = np.random.default_rng(83)
    cases = []
    for N in (128, 512):
        T, R = 3 * N + 5, R_OF[N]
        alts = _alts(N, rng)
        z, planted = V.plant(T, N, C, alts, GAPS, rng, margin=8.0)
        D = np.minimum(M.run_lengths(planted, N), M.MAX_MIN_FRAMES)
        raised = D.copy()
        edge = [k for i in (1, N // R // 2, N // R - 1) for k in (i * R - 1, i * R)]
        raised[edge] = D[edge] + 2
        raised[[k + (-1 if k % R == R - 1 else 1) for k in edge]] = 1
        assert (raised <= M.MAX_MIN_FRAMES).all() and (D >= 2).all()
        cases.append((z, alts, planted, D, raised, edge))
    got = _run([(c[0], c[1]) for c in cases] * 2, min_frames=[c[3].tolist() for c in cases] + [c[4].tolist() for c in cases])
    for j, (z, alts, planted, D, raised, edge) in enumerate(cases):
        N = len(alts)
        g = got[j]                                        # every D_k its planted run's length: the planted path, exactly
        assert (M.viterbi(z, alts, GAPS, D)[0] == planted).all(), "the planted path is not the reference's optimum (test setup)"
        rid, rtok = V.outputs(planted, z, alts, O_ID)
        assert g["status"] == 0 and (g["ids"] == rid).all() and (g["tok"] == rtok).all()
        ref, ref_score = M.viterbi(z, alts, GAPS, raised)  # two frames more at the thread boundaries: the float64 DP's path
        assert ref is not None and (M.run_lengths(planted, N)[edge] < raised[edge]).all()
        states = _check_against_dp(got[len(cases) + j], z, alts, raised, ref_score, "planted, raised")
        assert (M.run_lengths(states, N)[edge] >= raised[edge]).all()


# ------------------------------------------------------------------------------------------------ 4. infeasible beside feasible
def test_infeasible_clips_beside_feasible_ones_in_one_batch():
    rng = np.random.default_rng(84)

    def clip(T, N):
        return rng.standard_normal((T, C)).astype(np.float32) * 3, _alts(N, rng)
    clips = [clip(30, 5), clip(30, 5), clip(300, 130), clip(50, 4), clip(90, 20), clip(60, 6), clip(260, 130), clip(40, 5)]
    mins = [[3] * 5,
            [8, 8, 8, 3, 4],                                                  # sum D = 31 > T = 30
            None,
            [8, 2, 1, 1],                                                     # token 1's window closes before token 0 can end
            [4] * 20,
            [1, 2, 9, 1, 1, 1],                                               # a D of 9: status 4
            [2 if k % 3 else 1 for k in range(130)],
            [1, 0, 1, 1, 1]]                                                  # a D of 0: status 4
    wins = [None, None, None, [(0, 10), (3, 6), (0, 49), (0, 49)], [(4 * k, 4 * k + 10) for k in range(20)], None,
            [(k, k + 120) for k in range(130)], None]
    want = [0, 1, 0, 1, 0, 4, 0, 4]
    for b, ((z, alts), d, w) in enumerate(zip(clips, mins, wins)):            # the host rule predicts every status 1
        if want[b] != 4:
            w = w if w is not None else [AL.OPEN_WINDOW] * len(alts)
            assert AL.windows_feasible(len(z), w, d) == (want[b] == 0), b
    assert AL.windows_feasible(50, wins[3]) and AL.windows_feasible(30, [AL.OPEN_WINDOW] * 5)      # (feasible without the durations)
    got = _run(clips, windows=wins, min_frames=mins)
    for b, g in enumerate(got):
        assert g["status"] == want[b], b
        if want[b]:
            assert (g["ids"] == O_ID).all() and (g["tok"] == -1).all() and g["score"][0] == 0
            continue
        alone = _run([clips[b]], windows=None if wins[b] is None else [wins[b]], min_frames=[mins[b]])[0]
        assert alone["status"] == 0 and _same(alone, g), b
        z, alts = clips[b]
        D = np.ones(len(alts), np.int64) if mins[b] is None else np.array(mins[b])
        ref, ref_score = M.viterbi(z, alts, GAPS, D, windows=wins[b])
        states = _check_against_dp(g, z, alts, D, ref_score, f"clip {b}")
        if wins[b] is not None:
            assert W.in_windows(states, wins[b])


# ------------------------------------------------------------------------------------------------ 5. the sibling entries
def test_the_scoring_entries_refuse_a_batch_packed_with_durations():
    rng = np.random.default_rng(85)
    z, alts = rng.standard_normal((30, C)).astype(np.float32), _alts(4, rng)
    lg = torch.from_numpy(z).cuda()
    args = (lg, [30], [alts], [GAPS])
    packed = AL.pack_clips(*args, min_frames=[[2, 1, 3, 1]])
    assert packed.d_min is not None and packed.d_win is None and packed.d_min.cpu().tolist() == [2, 1, 3, 1]
    ids, tok, score, status = AL.viterbi_align(*args, O_ID, packed=packed)
    assert int(status[0]) == 0
    with pytest.raises(ValueError, match="alignment_posteriors scores the lattice without minimum durations"):
        AL.alignment_posteriors(*args, O_ID, tok, packed=packed)
    with pytest.raises(ValueError, match="edit_scores scores the lattice without minimum durations"):
        AL.edit_scores(*args, O_ID, [(1, 2)], packed=packed)
    with pytest.raises(ValueError, match="insertion_scores scores the lattice without minimum durations"):
        AL.insertion_scores(*args, O_ID, [(1, 2)], packed=packed)
    plain = AL.pack_clips(*args)                                              # without them the same calls run
    assert int(AL.alignment_posteriors(*args, O_ID, AL.viterbi_align(*args, O_ID, packed=plain)[1], packed=plain)[4][0]) == 0
