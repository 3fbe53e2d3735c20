"""-m gpu: wfl_align_duration_prior_counts (the counts instantiations of csrc/align_duration_prior_posterior.hip) against the float64
restatement of tests/duration_prior_counts_ref.py: every token's run-length posterior over the explicit-duration lattice.

Tolerances are the project's rule, exactly as tests/test_gpu_align_duration_prior_posterior.py states it: for every case the float32
restatement of the reference (same renormalisation period and the same maxima as the kernel) is run on the same inputs; its largest
deviation from float64 over the case, per output, is the yardstick, and the kernel is allowed 4 x that against float64; where the
yardstick is below half an fp32 ulp of the value itself, that half ulp is added (the outputs are fp32).  The outputs are logz, the
probabilities (columns 0 .. D - 1 of dur_post), the excess (column D), and two figures derived from a row and held by the same rule:
its sum over the D probabilities (1 in exact arithmetic; the half ulp is that of 1: D values rounded to fp32, which sum to 1) and its
expected length.  Every clip and token of every case is compared, and the figures are printed before anything is asserted.  The clips
are planted as that file plants them.  The bit-for-bit assertions are "a clip alone equals the clip in a batch": same kernel, same
arithmetic."""
import ctypes

import numpy as np
import pytest
import torch

import duration_prior_counts_ref as CR
import duration_prior_posterior_ref as PR
import test_gpu_align_duration_prior_posterior as TP
from wfl_asr_amd import align as AL

pytestmark = pytest.mark.gpu
C, O_ID, GAPS, NEG = TP.C, TP.O_ID, TP.GAPS, TP.NEG
KEYS = ("logz", "prob", "excess", "row_sum", "length")


def _count_rings(N, D):
    """How many of the counts kernel's three rings (alpha's, W, Q, in that order) its LDS holds (include/wfl_asr.h, the entry's
    workspace formula; CfgDpp::count_rings_in_lds)."""
    c = [i for i, (cap, _) in enumerate(TP.SLOTS) if N <= cap][0]
    slots = (128, 512, 1024, 2048, 4608)[c]
    room = (148992, 112128, 99840, 75264, 9728)[c] // 4
    return 3 if slots * (3 * D - 1) <= room else 2 if 2 * slots * D <= room else 1 if slots * D <= room else 0


def _split(clips, out, D):
    logz, dp, st = (x.cpu().numpy() for x in out)
    res, k0 = [], 0
    for b, c in enumerate(clips):
        n = len(c[1])
        res.append(dict(logz=np.array([logz[b]], np.float32), dur_post=dp[k0:k0 + n], status=int(st[b])))
        k0 += n
    assert dp.shape == (k0, D + 1)
    return res


def _run(clips, table, windows=None):
    """clips: list of (z [T, C] float32, alternatives, rows) -> per clip a dict of the entry's outputs."""
    out = AL.duration_prior_expected_counts(*TP._upload(clips), [c[2] for c in clips], table, windows=windows)
    torch.cuda.synchronize()
    return _split(clips, out, table.shape[1] - 1)


def _zeros(g):
    return g["logz"][0] == 0 and not g["dur_post"].any()


def _same(a, b):
    return a["status"] == b["status"] and a["logz"].tobytes() == b["logz"].tobytes() and a["dur_post"].tobytes() == b["dur_post"].tobytes()


def _views(logz, dur_post):
    """The five figures the rule is applied to, from a (logz, dur_post) pair, float64."""
    dp = np.asarray(dur_post, np.float64)
    D = dp.shape[1] - 1
    return {"logz": np.atleast_1d(np.float64(logz)), "prob": dp[:, :D], "excess": dp[:, D], "row_sum": dp[:, :D].sum(axis=1),
            "length": CR.expected_length(dp)}


REFS = {}                                   # a reference is computed once per (case, clip) and left unchanged


def _refs(key, z, alts, rows, table, win):
    if key not in REFS:
        REFS[key] = (CR.expected_counts(z, alts, GAPS, rows, table, windows=win),
                     CR.expected_counts(z, alts, GAPS, rows, table, windows=win, dtype=np.float32))
    return REFS[key]


def _check_case(name, clips, table, got, windows=None):
    """Every clip of a case against float64, by the 4 x yardstick rule; prints the figures before it asserts.  -> per clip the float64
    reference (None for a clip without a path) and the per-output allowances of the case (their largest value)."""
    yard = {k: 0.0 for k in KEYS}
    pairs = []
    for b, ((z, alts, rows), g) in enumerate(zip(clips, got)):
        win = windows[b] if windows is not None else None
        if g["status"] != 0:
            assert _zeros(g)
            if g["status"] == 1:
                assert CR.expected_counts(z, alts, GAPS, rows, table, windows=win) is None
            pairs.append(None)
            continue
        r64, r32 = _refs((name, b), z, alts, rows, table, win)
        assert r64 is not None, (name, b)
        assert not np.isnan(g["logz"]).any() and not np.isnan(g["dur_post"]).any() and (g["dur_post"] >= 0).all()
        v64, v32 = _views(r64["logz"], r64["dur_post"]), _views(r32["logz"], r32["dur_post"])
        for k in KEYS:
            if v64[k].size:
                yard[k] = max(yard[k], float(np.abs(v32[k] - v64[k]).max()))
        pairs.append(v64)
    dev = {k: 0.0 for k in KEYS}
    over = {k: -np.inf for k in KEYS}
    allow = {k: 0.0 for k in KEYS}
    for g, v64 in zip(got, pairs):
        if v64 is None:
            continue
        vg = _views(g["logz"][0], g["dur_post"])
        for k in KEYS:
            if not v64[k].size:
                continue
            d = np.abs(vg[k] - v64[k])
            h = TP._half_ulp(v64[k])
            allowed = 4 * yard[k] + np.where(yard[k] < h, h, 0.0)
            dev[k] = max(dev[k], float(d.max()))
            over[k] = max(over[k], float((d - allowed).max()))
            allow[k] = max(allow[k], float(allowed.max()))
    for k in KEYS:
        print(f"{name}: {k}: kernel {dev[k]:.3e}, float32 restatement {yard[k]:.3e}, allowed 4 x = {4 * yard[k]:.3e} (+ half an fp32 ulp "
              f"where that exceeds the restatement), over by {max(over[k], 0.0):.3e}")
    for k in KEYS:
        assert over[k] <= 0, (name, k, dev[k], yard[k], over[k])
    # an entry the table forbids is exactly 0.0
    for (z, alts, rows), g, v64 in zip(clips, got, pairs):
        if v64 is None:
            continue
        r = np.asarray(rows)
        D = table.shape[1] - 1
        forb = np.zeros((len(r), D + 1), bool)
        forb[r >= 0] = np.isneginf(table[r[r >= 0]])
        forb[:, D] |= forb[:, D - 1]                                  # no run reaches D frames: none goes past them
        assert not g["dur_post"][forb].any(), name
    return pairs, allow


def _rand_table(n, D, rng):
    t = rng.uniform(-6, 0, (n, D + 1)).astype(np.float32)
    t[:, D] = rng.uniform(-1, 0, n)
    return t


# ------------------------------------------------------------------------------------------------ 1. one clip per configuration
CONFIG_N = (100, 400, 900, 1800, 2500)


@pytest.mark.parametrize("N", CONFIG_N)
def test_one_clip_per_launch_configuration(N):
    D = 8
    clip, table, hard, _ = TP.planted_clip(N, N, D)
    g = _run([clip], table)[0]
    assert g["status"] == 0 and len(hard) >= 3
    (v64,), _ = _check_case(f"configuration N = {N}", [clip], table, [g])
    rows = np.array(clip[2])
    exact, more = rows == len(table) - 2, rows == len(table) - 1
    assert exact.sum() >= 2 and more.sum() >= 1
    # the two hard rows in the reference the kernel was just held to: exactly D frames is P(>= D) = 1 with no excess, D or more has
    # nothing below D; what they forbid is exactly 0 in the kernel's rows.  (1e-9: the float64 sweeps add up some 3000 frames of
    # scores of the order of 1e3, each good to 1e-16 of that.)
    assert np.abs(v64["prob"][exact, D - 1] - 1).max() < 1e-9 and np.abs(v64["prob"][more, D - 1] - 1).max() < 1e-9
    assert not g["dur_post"][exact, D].any() and not g["dur_post"][exact, :D - 1].any() and not g["dur_post"][more, :D - 1].any()
    assert (v64["excess"][more] > 0).all() and (g["dur_post"][more, D] > 0).all()


# ------------------------------------------------------------------------------------------------ 2. D = 1, 2 and 32; ring placement
@pytest.mark.parametrize("D", (1, 2, 32))
def test_the_shortest_and_the_longest_table(D):
    """At D = 1 there is no Q ring and no histogram entry, at D = 2 the ring is a single word."""
    rng = np.random.default_rng(1500 + D)
    table = _rand_table(10, D, rng)
    clips = [TP._random_clip(N + 150, N, 1510 + N + D, 10, D) for N in (40, 700)]
    assert [_count_rings(40, D), _count_rings(700, D)] == ([3, 3] if D <= 2 else [3, 0])
    pairs, _ = _check_case(f"D = {D}", clips, table, _run(clips, table))
    if D == 1:                                                   # column 0 is P(d >= 1) = 1, in the reference the kernel was held to
        assert all(np.abs(v["prob"][:, 0] - 1).max() < 1e-9 for v in pairs)


THRESHOLDS = {(300, 18): 3, (300, 19): 2, (300, 27): 2, (300, 28): 1, (700, 8): 3, (700, 9): 2, (700, 12): 2, (700, 13): 1, (700, 24): 1,
              (700, 25): 0, (1500, 3): 3, (1500, 4): 2, (1500, 5): 1, (1500, 9): 1, (1500, 10): 0}


@pytest.mark.parametrize("N,D", sorted(THRESHOLDS))
def test_both_sides_of_every_ring_threshold(N, D):
    """One clip on each side of every D at which a configuration's LDS lets go of a ring (N <= 127 keeps all three at every D, N > 2047
    none: test 1)."""
    assert _count_rings(N, D) == THRESHOLDS[(N, D)]
    rng = np.random.default_rng(1600 + N + D)
    table = _rand_table(10, D, rng)
    clips = [TP._random_clip(N + 150, N, 1610 + N + D, 10, D)]
    _check_case(f"N = {N}, D = {D}, {THRESHOLDS[(N, D)]} rings in LDS", clips, table, _run(clips, table))


def test_the_thresholds_are_all_of_them():
    """Every (configuration, D) at which count_rings changes is a pair of cases above."""
    for N in (100, 300, 700, 1500, 2500):
        for D in range(1, 32):
            if _count_rings(N, D) != _count_rings(N, D + 1):
                assert (N, D) in THRESHOLDS and (N, D + 1) in THRESHOLDS, (N, D)


# ------------------------------------------------------------------------------------------------ 3. block and renormalisation edges
@pytest.mark.parametrize("T", (127, 128, 129, 257))
def test_block_and_renormalisation_edges(T):
    rng = np.random.default_rng(1700 + T)
    D = 5
    table = _rand_table(6, D, rng)
    clips = [TP._random_clip(T, 20, 1710 + T, 6, D)]
    _check_case(f"T = {T}", clips, table, _run(clips, table))


# ------------------------------------------------------------------------------------------------ 4. windows, tokens without rows, -inf
def test_windows():
    rng = np.random.default_rng(1750)
    D = 4
    table = _rand_table(6, D, rng)
    table[2, :2] = NEG
    clips = [TP._random_clip(120, 20, 1751, 6, D), TP._random_clip(400, 150, 1752, 6, D), TP._random_clip(90, 12, 1753, 6, D)]
    free = _run(clips, table)
    wins = []
    for c, g in zip(clips, free):                                # a few tokens pinned near where an even spread puts them
        T, N = len(c[0]), len(c[1])
        w = [(0, T - 1)] * N
        for k in range(2, N, 5):
            mid = int((k + 0.5) * T / N)
            w[k] = (max(mid - 3, 0), min(mid + 3, T - 1))
        wins.append(w)
    wins[2][4] = (7, 3)                                          # an empty window: no path
    got = _run(clips, table, windows=wins)
    _check_case("windows", clips, table, got, windows=wins)
    assert [g["status"] for g in got] == [0, 0, 1]
    assert not _same(got[0], free[0])


def test_half_the_tokens_without_a_row():
    rng = np.random.default_rng(1760)
    D = 6
    table = _rand_table(8, D, rng)
    clips = []
    for N in (30, 200, 600):
        z, alts, rows = TP._random_clip(N + 90, N, 1761 + N, 8, D, p_row=1.0)
        clips.append((z, alts, [r if k % 2 else -1 for k, r in enumerate(rows)]))
    assert all(sum(r < 0 for r in c[2]) == len(c[2]) // 2 for c in clips)
    _check_case("half the tokens without a row", clips, table, _run(clips, table))


def test_forbidden_entries_are_exactly_zero():
    rng = np.random.default_rng(1770)
    D = 6
    table = _rand_table(8, D, rng)
    table[rng.random(table.shape) < 0.25] = NEG
    table[0, :] = rng.uniform(-3, 0, D + 1)                      # (one row that forbids nothing, so that paths remain)
    table[1, D] = NEG                                            # a tail alone
    table[2, D - 1] = NEG                                        # no run of D frames or more
    clips = []
    for i, (T, N) in enumerate(((260, 40), (700, 300))):
        z, alts, rows = TP._random_clip(T, N, 1771 + i, 8, D, p_row=0.8)
        clips.append((z, alts, rows))
    got = _run(clips, table)
    assert [g["status"] for g in got] == [0, 0]
    _check_case("forbidden entries", clips, table, got)          # (holds the exact zeros)
    assert any(np.isneginf(table[np.array(c[2])[np.array(c[2]) >= 0]]).any() for c in clips)


# ------------------------------------------------------------------------------------------------ 5. against the posterior kernel
def test_the_expected_length_is_the_posterior_kernels():
    """sum_d d P(d) + D P(>= D) + excess against frames + end_mean - start_mean of duration_prior_posteriors on the same clips; both
    kernels' allowances are added."""
    rng = np.random.default_rng(1780)
    D = 5
    table = _rand_table(8, D, rng)
    clips = [TP._random_clip(N + 90, N, 1781 + N, 8, D, scale=s) for N, s in ((30, 1.0), (200, 3.0), (600, 2.0))]
    got = _run(clips, table)
    _, allow = _check_case("expected length", clips, table, got)
    post = TP._run(clips, table)
    worst = 0.0
    for b, ((z, alts, rows), g, p) in enumerate(zip(clips, got, post)):
        assert g["status"] == 0 and p["status"] == 0
        r64 = PR.forward_backward(z, alts, GAPS, rows, table, tok=p["tok"])
        r32 = PR.forward_backward(z, alts, GAPS, rows, table, tok=p["tok"], dtype=np.float32)
        slack = allow["length"]
        for k in ("start_mean", "end_mean"):
            yard = float(np.abs(r32[k] - r64[k]).max())
            h = float(TP._half_ulp(r64[k]).max())
            slack += 4 * yard + (h if yard < h else 0.0)
        first, last = TP._ends(p["tok"], len(alts))
        want = (last - first + 1) + p["end_mean"].astype(np.float64) - p["start_mean"].astype(np.float64)
        d = float(np.abs(CR.expected_length(g["dur_post"]) - want).max())
        print(f"clip {b}: expected length: the two kernels differ by {d:.3e}, allowed {slack:.3e}")
        worst = max(worst, d - slack)
    assert worst <= 0


# ------------------------------------------------------------------------------------------------ 6. statuses
def test_statuses_beside_a_healthy_clip():
    rng = np.random.default_rng(1790)
    D = 4
    table = _rand_table(6, D, rng)
    table[5] = NEG                                               # a row that forbids every run
    healthy = TP._random_clip(200, 60, 1791, 5, D)
    solo = _run([healthy], table)[0]
    assert solo["status"] == 0
    too_few = TP._random_clip(5, 7, 1792, 5, D)                  # T < N
    z, alts, rows = TP._random_clip(80, 10, 1793, 5, D)
    bad_row = (z, alts, rows[:3] + [6] + rows[4:])               # a row out of range
    z, alts, rows = TP._random_clip(30, 4, 1794, 5, D)
    forbidden = (z, alts, [0, 5, 1, -1])                         # every path forbidden
    got = _run([too_few, healthy, bad_row, forbidden], table)
    assert [g["status"] for g in got] == [1, 0, 4, 1]
    assert all(_zeros(got[b]) for b in (0, 2, 3)) and _same(got[1], solo)
    _check_case("statuses", [too_few, healthy, bad_row, forbidden], table, got)
    rng2 = np.random.default_rng(1795)
    big = ((rng2.standard_normal((4200, C))).astype(np.float32), [[(1, 2)], [(3, 4)]] * 2048 + [[(5, 6)]], [-1] * 4097)
    got = _run([healthy, big], table)
    assert got[1]["status"] == 2 and _zeros(got[1]) and _same(got[0], solo)


# ------------------------------------------------------------------------------------------------ 7. alone = in a ragged batch
def test_alone_equals_in_a_ragged_batch():
    rng = np.random.default_rng(1800)
    D = 6
    table = _rand_table(8, D, rng)
    sizes = [(90, 30), (300, 140), (40, 3), (700, 520), (128, 60), (33, 33), (257, 100), (1, 1), (512, 127), (513, 128), (60, 0), (900, 511),
             (1400, 1024), (150, 70), (5, 9), (220, 90)]
    clips = [TP._random_clip(T, N, 1801 + i, 8, D) for i, (T, N) in enumerate(sizes)]
    got = _run(clips, table)
    for b in (1, 3, 7, 12):
        assert got[b]["status"] == 0 and _same(got[b], _run([clips[b]], table)[0]), b
    assert got[14]["status"] == 1 and got[10]["status"] == 0
    _check_case("ragged batch", [clips[b] for b in (0, 2, 5, 7)], table, [got[b] for b in (0, 2, 5, 7)])


def test_a_large_batch_runs_in_groups_under_the_workspace_limit(monkeypatch):
    rng = np.random.default_rng(1810)
    D = 6
    table = _rand_table(8, D, rng)
    sizes = [(90, 30), (300, 140), (5, 9), (257, 100), (40, 3), (150, 70)]
    clips = [TP._random_clip(T, N, 1811 + i, 8, D) for i, (T, N) in enumerate(sizes)]
    whole = _run(clips, table)
    need = [AL.duration_prior_counts_workspace_bytes([T], [N], D) for T, N in sizes]
    monkeypatch.setattr(AL, "EDITS_WORKSPACE_LIMIT", need[0] + need[1] + 1)          # the first two clips together, not all six
    assert len(AL.edit_groups([t for t, _ in sizes], [n for _, n in sizes],
                              workspace_bytes=lambda t, n: AL.duration_prior_counts_workspace_bytes(t, n, D))) >= 2
    grouped = _run(clips, table)
    assert [g["status"] for g in whole] == [0, 0, 1, 0, 0, 0]
    for b, (w, g) in enumerate(zip(whole, grouped)):
        assert _same(w, g), b


def test_a_batch_packed_with_minimum_durations_is_refused():
    z, alts, rows = TP._random_clip(50, 8, 1820, 3, 4)
    lg = torch.from_numpy(z).cuda()
    packed = AL.pack_clips(lg, [50], [alts], [GAPS], None, None, [[1] * 8])
    with pytest.raises(ValueError, match="min_frames"):
        AL.duration_prior_expected_counts(lg, [50], [alts], [GAPS], O_ID, [rows], np.zeros((3, 5), np.float32), packed=packed)


# ------------------------------------------------------------------------------------------------ 8. the C entry on device pointers
def test_the_entry_refuses_on_device_pointers():
    from wfl_asr_amd import _lib
    lib = _lib.load()
    T, N, D = 50, 8, 4
    z, alts, rows = TP._random_clip(T, N, 1830, 3, D)
    table = np.random.default_rng(1831).uniform(-3, 0, (3, D + 1)).astype(np.float32)
    lg = torch.from_numpy(z).cuda()
    packed = AL.pack_clips(lg, [T], [alts], [GAPS], None, None)
    d_tab = torch.from_numpy(table).cuda()
    d_dur = AL.upload_durations([rows], packed.N, lg.device)
    need = AL.duration_prior_counts_workspace_bytes([T], [N], D)
    assert need > 0 and AL.duration_prior_counts_workspace_bytes([0], [0], D) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    logz = torch.full((1,), 7.0, device="cuda")
    dp = torch.full((N, D + 1), 7.0, device="cuda")
    st = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
    h = lambda a: a.ctypes.data_as(ctypes.c_void_p)                             # noqa: E731

    def call(ws_bytes=need, dur=d_dur, tab=d_tab, D_=D, dur_post=dp, lz=logz, logits=lg):
        return lib.wfl_align_duration_prior_counts(p(logits), lg.stride(0), C, O_ID, h(packed.F0), h(packed.T), h(packed.K0), h(packed.N),
                                                   p(packed.d_tc), None, p(packed.d_gc), 1, p(dur), p(tab), 3, D_, p(ws), ws_bytes,
                                                   p(lz), p(dur_post), p(st), None)
    for kw, what in ((dict(ws_bytes=need - 1), b"workspace"), (dict(dur=None), b"null tok_dur"), (dict(tab=None), b"null dur"),
                     (dict(dur_post=None), b"null device pointer"), (dict(lz=None), b"null device pointer"),
                     (dict(logits=None), b"null device pointer"), (dict(D_=0), b"D must be 1 .. 32"), (dict(D_=33), b"D must be 1 .. 32")):
        assert call(**kw) < 0 and what in lib.wfl_last_error(), kw
    assert lib.wfl_align_duration_prior_counts_workspace_bytes(h(packed.T), h(packed.N), 1, 0) == -1
    assert lib.wfl_align_duration_prior_counts_workspace_bytes(h(packed.T), h(packed.N), 1, 33) == -1
    torch.cuda.synchronize()
    assert int(st[0]) == 77 and float(logz[0]) == 7.0 and float(dp[0, 0]) == 7.0      # nothing was launched after a refusal
    assert call() == 0
    torch.cuda.synchronize()
    assert int(st[0]) == 0 and float(dp[0, 0]) != 7.0
    r64 = CR.expected_counts(z, alts, GAPS, rows, table)
    assert np.abs(dp.cpu().numpy() - r64["dur_post"]).max() < 1e-3
