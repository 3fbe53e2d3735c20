"""-m gpu: wfl_align_windowed / wfl_align_posterior_windowed (csrc/align.hip, csrc/align_posterior.hip; the mask is csrc/lattice.h
win_mask) against the float64 windowed references of tests/viterbi_window_ref.py.  C = 141, one ragged batch per test.

Bounds.  The search: the kernel's path is legal, opens every token inside its window, its float64 score is >= the windowed float64
optimum - 1e-3 and `score` is within 1e-3 T of it -- the bounds of tests/test_gpu_align.py.  The posterior: the rule of
tests/test_gpu_align_posterior.py, 4 x the deviation of the float32 restatement from float64 on the same (windowed) inputs, plus half
an fp32 ulp of the value where that exceeds the restatement's deviation.  start_mean + first frame inside [lo, hi]: the mean is a
convex combination of frames of the window (double), then rounded to fp32: half an fp32 ulp of a number below 16 frames, < 1e-6."""
import numpy as np
import pytest
import torch

import posterior_ref as P
import viterbi_ref as V
import viterbi_window_ref as W
from wfl_asr_amd import align as AL

pytestmark = pytest.mark.gpu
C = 141
O_ID = 0
GAPS = [O_ID, 137, 138]
KEYS = ("logz", "tok_post", "start_mean", "start_sd")
R_OF = {3: 2, 128: 2, 512: 4, 1024: 8, 2048: 9}           # slots per thread of the configuration that takes N tokens (csrc/lattice.h)


def _alts(N, rng):
    return [[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 68, N)]


def _run(clips, windows, posterior=False, tok_from=None):
    """clips: [(z, alternatives)]; windows: None (the unwindowed entries) or per clip a list of (lo, hi) / None -> per clip a dict of
    numpy outputs.  posterior: also alignment_posteriors on the search's tok (or on tok_from: per-clip tok arrays)."""
    T = [len(c[0]) for c in clips]
    lg = torch.from_numpy(np.ascontiguousarray(np.concatenate([c[0] for c in clips]))).cuda()
    args = (lg, T, [c[1] for c in clips], [GAPS] * len(clips), O_ID)
    ids, tok, score, status = AL.viterbi_align(*args, windows=windows)
    post = None
    if posterior:                                         # (the windows reach the posterior in the packed batch)
        ptok = tok if tok_from is None else torch.from_numpy(np.concatenate(tok_from).astype(np.int32)).cuda()
        packed = AL.pack_clips(*args[:4], windows=windows)
        assert (packed.d_win is None) == (windows is None)
        post = [x.cpu().numpy() for x in AL.alignment_posteriors(*args, ptok, packed=packed)]
    torch.cuda.synchronize()
    ids, tok, score, status = (x.cpu().numpy() for x in (ids, tok, score, status))
    out, pos, k0 = [], 0, 0
    for b, t in enumerate(T):
        n = len(clips[b][1])
        g = dict(ids=ids[pos:pos + t], tok=tok[pos:pos + t], score=score[b:b + 1], status=int(status[b]))
        if post is not None:
            g.update(logz=post[0][b:b + 1], tok_post=post[1][k0:k0 + n], start_mean=post[2][k0:k0 + n], start_sd=post[3][k0:k0 + n],
                     pstatus=int(post[4][b]))
        out.append(g)
        pos += t
        k0 += n
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


# ------------------------------------------------------------------------------------------------ 1. open windows: bit for bit
def test_open_windows_are_bit_identical_to_the_unwindowed_entries():
    rng = np.random.default_rng(31)
    clips = []
    for N in (3, 128, 512, 1024, 2048):                   # one clip per configuration; T = N + 150 spans several logits stages, more
        T = N + 150                                       # than one renormalisation, backtrace window and posterior block
        clips.append((rng.standard_normal((T, C)).astype(np.float32) * 3, _alts(N, rng)))
    plain = _run(clips, None, posterior=True)
    # open windows three ways: a clip's None, spelled out, and wider than any clip
    wins = [None, [AL.OPEN_WINDOW] * 128, [(-5, 10 ** 6)] * 512, None, [AL.OPEN_WINDOW] * 2048]
    opened = _run(clips, wins, posterior=True)
    for a, b in zip(plain, opened):
        assert a["status"] == b["status"] == 0 and a["pstatus"] == b["pstatus"] == 0
        assert (a["ids"] == b["ids"]).all() and (a["tok"] == b["tok"]).all()
        assert a["score"].tobytes() == b["score"].tobytes()
        for k in KEYS:
            assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 2. planted path, moved windows
def _moved_windows(starts, T, R):
    """+-2 around every planted start, then a few tokens' windows moved 3 .. 6 frames later, (s + 3, s + 6), which excludes s: the
    tokens at k = i R - 1 and k = i R (the neighbour-thread exchange of both sweeps) and one in the middle of a thread's slots.  Where the
    tokens are dense a moved token pushes its successors: the move runs on over the following tokens until the host rule
    (align.windows_feasible, checked against enumeration in tests/test_align_windows_cpu.py) finds the whole clip feasible."""
    N = len(starts)
    base = [(int(s) - 2, int(s) + 2) for s in starts]
    anchors = sorted({k for i in (1, max(N // R // 2, 1)) for k in (i * R - 1, i * R) if 0 <= k < N} | {min(N - 1, 2 * R + 1)})
    wins = list(base)
    moved = _move_later(wins, starts, anchors, 3, 6, T)
    return base, wins, moved, anchors


def _move_later(wins, starts, anchors, d_lo, d_hi, T):
    """The windows of the tokens `anchors` to (s + d_lo, s + d_hi), each move running on over the following tokens until
    align.windows_feasible finds the clip feasible again -> the moved tokens."""
    moved = set()
    for a in anchors:
        k = a
        while True:
            wins[k] = (int(starts[k]) + d_lo, int(starts[k]) + d_hi)
            moved.add(k)
            if AL.windows_feasible(T, wins) or k + 1 >= len(wins):
                break
            k += 1
    assert AL.windows_feasible(T, wins), "the moved windows are infeasible (test setup)"
    return sorted(moved)


def test_planted_path_with_moved_windows():
    rng = np.random.default_rng(32)
    cases = []
    for T, N in ((40, 3), (300, 128), (700, 512), (2300, 2048)):      # (the last: the 512 x 9 configuration, R = 9)
        alts = _alts(N, rng)
        z, planted = V.plant(T, N, C, alts, GAPS, rng, margin=8.0)
        starts = W.starts(planted, N)
        base, wins, moved, anchors = _moved_windows(starts, T, R_OF[N])
        R = R_OF[N]
        assert any(k % R == 0 and k for k in anchors) and any(k % R == R - 1 for k in anchors)
        assert all(not (wins[k][0] <= starts[k] <= wins[k][1]) for k in moved) and len(moved) < N
        cases.append((z, alts, planted, base, wins, moved))
    got = _run([(c[0], c[1]) for c in cases] * 2, [c[4] for c in cases] + [c[3] for c in cases])
    for j, (z, alts, planted, base, wins, moved) in enumerate(cases):
        T, N = len(z), len(alts)
        g = got[j]
        assert g["status"] == 0
        states = _states(g["ids"], g["tok"])
        assert V.legal(states, N), "the kernel's path is not a legal path"
        st = W.starts(states, N)
        assert all(lo <= t <= hi for t, (lo, hi) in zip(st, wins)), "a token opens outside its window"
        ref, ref_score = W.viterbi(z, alts, GAPS, wins)
        assert ref is not None and (W.starts(ref, N)[moved] != W.starts(planted, N)[moved]).all()
        mine = V.path_score(states, z, alts, GAPS)
        print(f"T {T} N {N}: {len(moved)} moved tokens, path score {mine:.4f}, reference {ref_score:.4f}, kernel score {g['score'][0]:.4f}")
        assert mine >= ref_score - 1e-3, (mine, ref_score)
        assert abs(float(g["score"][0]) - ref_score) <= 1e-3 * T, (g["score"], ref_score)
        # the windows back at +-2 around the planted starts: the planted path, exactly
        r = got[len(cases) + j]
        assert (W.viterbi(z, alts, GAPS, base)[0] == planted).all(), "the planted path is not the reference's optimum (test setup)"
        assert r["status"] == 0 and (_states(r["ids"], r["tok"]) == planted).all()
        rid, rtok = V.outputs(planted, z, alts, O_ID)
        assert (r["ids"] == rid).all() and (r["tok"] == rtok).all()


# ------------------------------------------------------------------------------------------------ 3. infeasible beside feasible
def test_infeasible_clips_beside_feasible_ones_in_one_batch():
    rng = np.random.default_rng(33)

    def clip(T, N):
        return rng.standard_normal((T, C)).astype(np.float32) * 3, _alts(N, rng)
    clips = [clip(30, 5), clip(30, 5), clip(300, 200), clip(50, 4), clip(90, 40), clip(25, 3), clip(200, 130)]
    wins = [[(0, 29)] * 5,
            [(0, 29), (7, 7), (7, 7), (0, 29), (0, 29)],                      # two tokens pinned to one frame
            None,
            [(0, 49), (12, 9), (0, 49), (0, 49)],                             # lo > hi
            [(2 * k, 2 * k + 8) for k in range(40)],
            [(0, 24), (0, 24), (25, 40)],                                     # a window at or beyond T
            [(k, k + 80) for k in range(130)]]
    feasible = [AL.windows_feasible(len(c[0]), w if w is not None else [AL.OPEN_WINDOW] * len(c[1])) for c, w in zip(clips, wins)]
    assert feasible == [True, False, True, False, True, False, True]
    got = _run(clips, wins, posterior=True)
    for b, (g, ok) in enumerate(zip(got, feasible)):
        assert g["status"] == (0 if ok else 1), b
        if not ok:
            assert (g["ids"] == O_ID).all() and (g["tok"] == -1).all() and g["score"][0] == 0
            # (its all -1 tok is no path either: the posterior refuses it as well, and gives zeros)
            assert g["pstatus"] != 0 and g["logz"][0] == 0 and not g["tok_post"].any() and not g["start_sd"].any()
            continue
        alone = _run([clips[b]], [wins[b]], posterior=True)[0]
        assert alone["status"] == 0 and alone["pstatus"] == g["pstatus"] == 0
        assert (alone["ids"] == g["ids"]).all() and (alone["tok"] == g["tok"]).all()
        for k in ("score",) + KEYS:
            assert alone[k].tobytes() == g[k].tobytes(), (b, k)
        st = W.starts(_states(g["ids"], g["tok"]), len(clips[b][1]))
        w = wins[b] if wins[b] is not None else [AL.OPEN_WINDOW] * len(st)
        assert all(lo <= t <= hi for t, (lo, hi) in zip(st, w))


# ------------------------------------------------------------------------------------------------ 4. the windowed posterior
def _half_ulp(ref):
    return 0.5 * np.spacing(np.abs(np.asarray(ref, np.float64)).astype(np.float32)).astype(np.float64)


def _posterior_cases():
    rng = np.random.default_rng(34)
    cases = []
    for T, N, boost in ((40, 3, 4.0), (300, 128, 0.0), (700, 512, 4.0), (1250, 1024, 4.0), (2300, 2048, 4.0)):
        alts = _alts(N, rng)
        z = P.planted_logits(T, N, C, alts, GAPS, rng, boost)
        s = W.starts(V.viterbi(z, alts, GAPS)[0], N)                  # windows around the unwindowed float64 optimum's starts ...
        wins = [(int(x) - int(a), int(x) + int(b)) for x, a, b in zip(s, rng.integers(0, 5, N), rng.integers(0, 5, N))]
        for k in range(0, N, 7):                                      # ... every seventh token pinned to its frame
            wins[k] = (int(s[k]), int(s[k]))
        assert AL.windows_feasible(T, wins), "test setup"               # (the optimum itself satisfies them)
        if N > 3:                                                     # ... and two neighbours across a thread boundary held off it
            R = R_OF[N]
            _move_later(wins, s, [3 * R - 1, 3 * R], 1, 3, T)
        cases.append((z, alts, wins))
    return cases


def test_windowed_posterior_against_the_float64_windowed_forward_backward():
    cases = _posterior_cases()
    got = _run([(c[0], c[1]) for c in cases], [c[2] for c in cases], posterior=True)
    for (z, alts, wins), g in zip(cases, got):
        T, N = len(z), len(alts)
        assert g["status"] == 0 and g["pstatus"] == 0
        r64 = W.forward_backward(z, alts, GAPS, wins, tok=g["tok"])
        r32 = W.forward_backward(z, alts, GAPS, wins, tok=g["tok"], dtype=np.float32)
        assert r64 is not None and r32 is not None
        for k in KEYS:
            ref = np.atleast_1d(np.asarray(r64[k], np.float64))
            yard = float(np.abs(np.atleast_1d(r32[k]) - ref).max())
            h = _half_ulp(ref)
            allowed = 4 * yard + np.where(yard < h, h, 0.0)
            d = np.abs(g[k].astype(np.float64) - ref)
            print(f"T {T} N {N}: {k}: kernel {d.max():.3e}, float32 restatement {yard:.3e}, over by {max(float((d - allowed).max()), 0):.3e}")
            assert (d <= allowed).all(), (T, N, k, float(d.max()), yard)
        first = np.array([int(np.nonzero(g["tok"] == k)[0][0]) for k in range(N)])
        lo, hi = np.array(wins).T
        assert (first >= lo).all() and (first <= hi).all()
        start = g["start_mean"].astype(np.float64) + first
        assert (start >= lo - 1e-6).all() and (start <= hi + 1e-6).all(), "a start's posterior mean lies outside its window"
        pinned = lo == hi
        assert pinned.sum() >= 1 and (g["start_sd"][pinned] == 0).all() and (g["start_mean"][pinned] == 0).all()
        assert (g["start_sd"][~pinned] > 0).any()


def test_a_tok_that_opens_a_token_outside_its_window_is_status_8():
    rng = np.random.default_rng(35)
    clips = [(P.planted_logits(60, 6, C, a, GAPS, rng, 4.0), a) for a in (_alts(6, rng), _alts(6, rng))]
    plain = _run(clips, None)
    f1 = int(np.nonzero(plain[1]["tok"] == 1)[0][0])
    wins = [None, [AL.OPEN_WINDOW, (f1 + 1, f1 + 3)] + [AL.OPEN_WINDOW] * 4]      # token 1 of clip 1 may not open where `tok` opens it
    got = _run(clips, wins, posterior=True, tok_from=[p["tok"] for p in plain])
    assert got[0]["pstatus"] == 0 and got[0]["tok_post"].max() > 0
    assert got[1]["pstatus"] == 8
    g = got[1]
    assert g["logz"][0] == 0 and not g["tok_post"].any() and not g["start_mean"].any() and not g["start_sd"].any()


def test_windows_without_a_path_are_status_1_in_the_posterior():
    """Windows that cannot be met in order, and a `tok` that passes the first-frame check all the same (it is no path: token 1 runs
    before token 0): alpha runs, logZ is -inf, status 1 and zeros.  Beside it a feasible clip, untouched."""
    rng = np.random.default_rng(36)
    clips = [(rng.standard_normal((10, C)).astype(np.float32), _alts(2, rng)), (rng.standard_normal((10, C)).astype(np.float32), _alts(2, rng))]
    wins = [[(4, 6), (0, 3)], [(0, 3), (4, 6)]]
    assert [AL.windows_feasible(10, w) for w in wins] == [False, True]
    tok = [np.array([1, 1, 1, 1, 0, 0, 0, 0, 0, 0], np.int32), np.array([0, 0, 0, 0, 1, 1, 1, 1, 1, 1], np.int32)]
    got = _run(clips, wins, posterior=True, tok_from=tok)
    assert got[0]["status"] == 1 and got[0]["pstatus"] == 1
    g = got[0]
    assert g["logz"][0] == 0 and not g["tok_post"].any() and not g["start_mean"].any() and not g["start_sd"].any()
    assert got[1]["status"] == 0 and got[1]["pstatus"] == 0 and got[1]["tok_post"].max() > 0
