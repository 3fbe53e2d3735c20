"""-m gpu: wfl_decode_duration (csrc/decode_duration.hip) against the float64 numpy recurrence of tests/bio_duration_ref.py on seeded
logits, seeded transition tables and seeded duration tables, ragged batches.

Criterion and bounds are those of tests/test_gpu_decode_bigram.py (the arithmetic is the same class: fp32 sums of logits and weights,
renormalised every 16 frames, the offset carried in a double): the kernel's path is legal, every forced frame is O, no opened run
takes a -inf entry of W, no run has a length whose L is -inf, the float64 objective of the kernel's path is >= the reference
optimum - 1e-3, and |score - reference score| <= 1e-3 T.  The bounds were fixed before any run and stay as they are.  Measured on one
MI355X over this file's 447 clips: the largest objective gap is 0, the largest score difference 5.7e-4 (the 6000-frame clip) and
7.4e-7 per frame.

Forced frames: the MARGIN = 1e-4 rule of tests/test_gpu_decode.py.  The seeds are chosen so that NO frame of any input is inside that
margin (asserted), so every frame the float64 pre-pass forces must be O, none is excused.

The table and clip builders are tests/test_gpu_decode_bigram.py's, copied.
"""
import numpy as np
import pytest
import torch

import bio_bigram_ref as RB
import bio_duration_ref as R
from wfl_asr_amd import decode as DC

pytestmark = pytest.mark.gpu
MARGIN = 1e-4
LENGTHS = [1, 2, 15, 16, 17, 0, 31, 32, 33, 300]
# every P of {1, 2, 64, 65, 191} and every D of {1, 2, 8, 32}; 191 phonemes are the symbol cap, where only D = 1 keeps the run history in
# LDS: (191, 1) and (191, 32) take the kernel's two paths
CASES = [(1, 1), (2, 32), (2, 8), (64, 8), (65, 2), (65, 32), (191, 1), (191, 32)]
THRESHOLD = 0.5
TINY = (1, [(0, 2), (3, 4), (5, -1)])          # tests/test_decode_duration_cpu.py's class table: O, two phonemes with I, one without
TINY_C = 6


def make_table(P):
    """O = 1 (not the first class); phoneme p: B = 2 + 2p, I = 3 + 2p, every fifth phoneme (from the second on) has no I class, whose
    column is then never chosen; three more never-chosen classes: column 0 and the last two.  -> (C, (o_id, pairs))."""
    pairs = [(2 + 2 * p, -1 if p % 5 == 1 else 3 + 2 * p) for p in range(P)]
    return 2 * P + 4, (1, pairs)


def make_trans(P, rng, forbid=0.0):
    """Random weights in [-8, 0]; `forbid`: that share of the entries -inf, the [p][O] column kept finite."""
    W = -8.0 * rng.random((P + 1, P + 1))
    if forbid:
        mask = rng.random(W.shape) < forbid
        mask[:, 0] = False
        W[mask] = -np.inf
    return W.astype(np.float32)


def make_dur(P, D, rng, forbid=0.2, no_tail=1 / 3, no_prior=0.2):
    """-> (dur [P, D + 1] float32 in [-6, 0], `forbid` of the entries -inf and `no_tail` of the tails -inf; sym_dur [P] int32, a random
    row each, `no_prior` of them -1)."""
    dur = -6.0 * rng.random((P, D + 1))
    dur[rng.random(dur.shape) < forbid] = -np.inf
    dur[rng.random(P) < no_tail, D] = -np.inf
    sd = rng.integers(0, P, size=P)
    sd[rng.random(P) < no_prior] = -1
    return dur.astype(np.float32), sd.astype(np.int32)


def make_clips(P, seed, lengths=LENGTHS):
    """Seeded clips for P phonemes: random logits (x 3), every other one with a planted path."""
    C, table = make_table(P)
    rng = np.random.default_rng(seed)
    clips = []
    for j, T in enumerate(lengths):
        if j % 2 == 0 or T < 5:
            clips.append(rng.standard_normal((T, C)).astype(np.float32) * 3)
        else:
            clips.append(R.plant(T, C, table, rng, margin=4.0, scale=2.0)[0])
    return C, table, clips


SEEDS = {1: 101, 2: 102, 64: 164, 65: 165, 191: 1291}      # chosen on the CPU: no frame inside MARGIN at 0.5


def _split_out(T, ids, score, status):
    ids, score, status = ids.cpu().numpy(), score.cpu().numpy(), status.cpu().numpy()
    out, pos = [], 0
    for b, t in enumerate(T):
        out.append((ids[pos:pos + t], float(score[b]), int(status[b])))
        pos += t
    return out


def _run(clips, table, W, dur, sd, thr, C):
    """clips: list of z [T, C] float32 -> numpy (ids, score, status) per clip."""
    z = np.concatenate(clips) if clips else np.zeros((0, C), np.float32)
    lg = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    T = [len(c) for c in clips]
    ids, score, status = DC.bio_viterbi_duration(lg, T, table, W, dur, sd, thr)
    torch.cuda.synchronize()
    return _split_out(T, ids, score, status)


def _raw(lg, T, table, W, dur, sd, thr):
    """The ABI entry without the Python entry's checks of dur and sym_dur (for the statuses those checks would pre-empt)."""
    clips = DC._check_clips(lg, T, table, 0.0, thr, None)
    nb = len(T)
    ids = torch.empty(lg.shape[0], dtype=torch.int32, device=lg.device)
    score = torch.empty(max(nb, 1), dtype=torch.float32, device=lg.device)
    status = torch.empty(max(nb, 1), dtype=torch.int32, device=lg.device)
    dur = np.ascontiguousarray(dur, np.float32)
    D = dur.shape[1] - 1
    DC._call("wfl_decode_duration", lg, clips, (np.ascontiguousarray(W, np.float32), np.ascontiguousarray(sd, np.int32), dur, len(dur), D,
                                                float(thr)), (ids, score, status), None, ws_more=(D,))
    torch.cuda.synchronize()
    return ids, score[:nb], status[:nb]


def forced_frames(z, thr):
    """The float64 pre-pass; asserts that no frame is inside MARGIN of the threshold and that fp32 would agree."""
    lse, forced, pmax = R.prepass(z, thr)
    if thr > 0 and len(z):
        _, f32, p32 = R.prepass(z, thr, np.float32)
        dev = float(np.abs(p32.astype(np.float64) - pmax).max())
        gap = float(np.abs(pmax - thr).min())
        assert dev <= MARGIN / 4, dev
        assert gap > MARGIN, "a frame of the test input is inside the margin of the threshold: choose another seed"
        assert (f32 == forced).all()
    return lse, forced


GAPS = {"objective": 0.0, "score_per_frame": 0.0}


def _check(z, table, W, dur, sd, thr, got, planted=None, ref=None):
    """The criterion of the module's docstring for one clip -> the float64 objective of the kernel's path.  ref: (ids or None, optimum)
    where the caller has it already."""
    ids, score, status = got
    T = len(z)
    assert status == 0
    assert len(ids) == T
    if T == 0:
        assert score == 0.0
        return 0.0
    lse, forced = forced_frames(z, thr)
    if ref is None:
        ref = R.viterbi(z, table, W, dur, sd, forced)
        assert abs(R.objective(ref[0], z, table, W, dur, sd, forced) - ref[1]) <= 1e-9 * max(1.0, abs(ref[1])), "the reference's own path"
    ref_ids, ref_obj = ref
    assert R.legal(ids, table), "the kernel's path is not a legal path"
    assert (ids[forced] == table[0]).all(), "a forced frame is not O"
    assert RB.forbidden_successions(ids, table, W) == 0, "the kernel's path takes a forbidden succession"
    assert R.forbidden_durations(ids, table, dur, sd) == 0, "a run of the kernel's path has a forbidden duration"
    mine = R.objective(ids, z, table, W, dur, sd, forced)
    ref_score = ref_obj - float(lse.sum())
    GAPS["objective"] = max(GAPS["objective"], ref_obj - mine)
    GAPS["score_per_frame"] = max(GAPS["score_per_frame"], abs(score - ref_score) / T)
    print(f"T {T} P {len(table[1])} D {dur.shape[1] - 1} thr {thr}: objective {mine:.6f} ref {ref_obj:.6f} (gap {ref_obj - mine:.3e}); "
          f"score {score:.4f} ref {ref_score:.4f} (diff {abs(score - ref_score):.3e}); largest so far: gap {GAPS['objective']:.3e}, "
          f"|score diff| / T {GAPS['score_per_frame']:.3e}")
    assert mine >= ref_obj - 1e-3, (mine, ref_obj)
    assert abs(score - ref_score) <= 1e-3 * T, (score, ref_score)
    if planted is not None:
        assert (ref_ids == planted).all(), "the planted path is not the reference's optimum (test setup)"
        assert (ids == planted).all()
    return mine


@pytest.mark.parametrize("P,D", CASES)
def test_ragged_batch_against_float64_recurrence(P, D):
    C, table, clips = make_clips(P, SEEDS[P])
    rng = np.random.default_rng(1000 + 40 * P + D)
    for forbid, thr in ((0.0, 0.0), (0.3, THRESHOLD)):
        W = make_trans(P, rng, forbid)
        dur, sd = make_dur(P, D, rng)
        got = _run(clips, table, W, dur, sd, thr, C)
        assert len(got[LENGTHS.index(0)][0]) == 0
        for z, g in zip(clips, got):
            _check(z, table, W, dur, sd, thr, g)


@pytest.mark.parametrize("D", [1, 2, 3])
def test_tiny_clips_against_brute_force(D):
    """100 clips of 1 .. 6 frames per D in one call, the optimum from the enumeration of every class string: the off-by-one cases of
    the history ring and the tail.  (The seeds: no frame inside MARGIN.)"""
    rng = np.random.default_rng(7300 + D)
    clips = [(rng.standard_normal((int(rng.integers(1, 7)), TINY_C)) * 2).astype(np.float32) for _ in range(100)]
    W = (-3.0 * rng.random((4, 4))).astype(np.float32)
    mask = rng.random((4, 4)) < 0.2
    mask[:, 0] = False
    W[mask] = -np.inf
    dur, sd = make_dur(3, D, rng, forbid=0.25)
    got = _run(clips, TINY, W, dur, sd, THRESHOLD, TINY_C)
    for z, g in zip(clips, got):
        _, forced = forced_frames(z, THRESHOLD)
        _check(z, TINY, W, dur, sd, THRESHOLD, g, ref=(None, R.brute_force(z, TINY, W, dur, sd, forced)[1]))


@pytest.mark.parametrize("prior", ["none", "zero"])
def test_without_a_prior_the_search_is_wfl_decode_bigram(prior):
    """Every sym_dur = -1, and an all-zero table: the objective is wfl_decode_bigram's.  Planted inputs (no ties): identical ids; both
    scores are within the bound of the float64 reference, so within twice the bound of each other."""
    for P, D in ((2, 1), (70, 8), (70, 32)):
        C, table = make_table(P)
        rng = np.random.default_rng(40 + P + D)
        clips = [R.plant(T, C, table, rng)[0] for T in (33, 300)]
        W = make_trans(P, rng)
        dur = np.zeros((3, D + 1), np.float32)
        sd = np.full(P, -1, np.int32) if prior == "none" else rng.integers(0, 3, size=P).astype(np.int32)
        got = _run(clips, table, W, dur, sd, 0.0, C)
        lg = torch.from_numpy(np.concatenate(clips)).cuda()
        ids, score, st = DC.bio_viterbi_bigram(lg, [len(c) for c in clips], table, W, 0.0)
        assert st.cpu().tolist() == [0, 0]
        ids, score, pos = ids.cpu().numpy(), score.cpu().numpy(), 0
        for b, z in enumerate(clips):
            _check(z, table, W, dur, sd, 0.0, got[b])
            assert (got[b][0] == ids[pos:pos + len(z)]).all()
            assert abs(got[b][1] - float(score[b])) <= 2e-3 * len(z)
            pos += len(z)


def test_a_hard_maximum_is_kept():
    """Every row is -inf beyond 3 frames (tail included), W[q][q] is finite, the planted runs last 10 frames: no run of the kernel's
    path exceeds 3 frames."""
    P, D = 20, 5
    C, table = make_table(P)
    rng = np.random.default_rng(61)
    clips = [R.plant(T, C, table, rng, margin=4.0, scale=1.0, min_run=10, max_run=10)[0] for T in (100, 37)]
    W = make_trans(P, rng)
    dur = (-2.0 * rng.random((P, D + 1))).astype(np.float32)
    dur[:, 3:] = -np.inf
    sd = np.arange(P, dtype=np.int32)
    got = _run(clips, table, W, dur, sd, 0.0, C)
    for z, g in zip(clips, got):
        _check(z, table, W, dur, sd, 0.0, g)
        runs = R.run_lengths(g[0], table)
        assert runs and max(d for _, _, d in runs) <= 3


def test_a_hard_minimum_is_kept():
    """L(1) = L(2) = -inf: every phoneme run of the kernel's path has at least 3 frames, the one the clip ends in and the ones in front
    of forced frames too."""
    P, D = 20, 6
    C, table = make_table(P)
    rng = np.random.default_rng(62)
    clips = [R.plant(T, C, table, rng, margin=4.0, scale=2.0, min_run=2, max_run=9)[0] for T in (120, 41)]
    clips.append(rng.standard_normal((90, C)).astype(np.float32) * 3)
    W = make_trans(P, rng)
    dur = (-2.0 * rng.random((P, D + 1))).astype(np.float32)
    dur[:, :2] = -np.inf
    sd = np.arange(P, dtype=np.int32)
    got = _run(clips, table, W, dur, sd, THRESHOLD, C)
    n_runs = n_forced = 0
    for z, g in zip(clips, got):
        _check(z, table, W, dur, sd, THRESHOLD, g)
        runs = R.run_lengths(g[0], table)
        n_runs += len(runs)
        n_forced += int(forced_frames(z, THRESHOLD)[1].sum())
        assert all(d >= 3 for _, _, d in runs), runs
    assert n_runs > 0 and n_forced > 0, "no run or no forced frame (test setup)"


def test_a_long_run_pays_the_tail():
    """D = 4 and a planted run of 40 frames between two stretches of O: the planted segmentation is the reference's optimum, the
    kernel returns it, and the score carries L(4) + 36 tail."""
    P, D = 5, 4
    C, table = make_table(P)
    o, (b, i) = table[0], table[1][2]
    rng = np.random.default_rng(63)
    planted = np.array([o] * 10 + [b] + [i] * 39 + [o] * 11, np.int32)
    z = rng.standard_normal((len(planted), C)).astype(np.float32)
    z[np.arange(len(planted)), planted] += 6.0
    W = np.full((P + 1, P + 1), -1.0, np.float32)
    dur = np.tile(np.array([-3.0, -2.0, -1.5, -0.5, -0.25], np.float32), (P, 1))
    sd = np.arange(P, dtype=np.int32)
    got = _run([z], table, W, dur, sd, 0.0, C)[0]
    _check(z, table, W, dur, sd, 0.0, got, planted=planted)
    want = float(z.astype(np.float64)[np.arange(len(planted)), planted].sum()) - 2.0 + (-0.5 + 36 * -0.25) - float(R.prepass(z, 0.0)[0].sum())
    assert abs(got[1] - want) <= 1e-3 * len(planted), (got[1], want)


def test_one_6000_frame_clip():
    P, D = 70, 32
    C, table, clips = make_clips(P, 11077, lengths=[6000])
    rng = np.random.default_rng(78)
    W = make_trans(P, rng, 0.3)
    dur, sd = make_dur(P, D, rng)
    got = _run(clips, table, W, dur, sd, THRESHOLD, C)
    _check(clips[0], table, W, dur, sd, THRESHOLD, got[0])


def test_a_clip_alone_equals_the_clip_in_a_batch_of_16():
    P, D = 70, 8
    C, table = make_table(P)
    rng = np.random.default_rng(3)
    W = make_trans(P, rng, 0.3)
    dur, sd = make_dur(P, D, rng)
    clips = [rng.standard_normal((int(rng.integers(1, 400)), C)).astype(np.float32) * 3 for _ in range(16)]
    batch = _run(clips, table, W, dur, sd, 0.0, C)
    for b in (0, 5, 15):
        alone = _run([clips[b]], table, W, dur, sd, 0.0, C)[0]
        assert (alone[0] == batch[b][0]).all()
        assert np.float32(alone[1]).tobytes() == np.float32(batch[b][1]).tobytes() and alone[2] == batch[b][2] == 0


def test_symbol_cap_is_reported_and_the_neighbours_are_untouched():
    """tests/test_gpu_decode_bigram.py's arrangement: three clips back to back in one buffer, the middle one decoded with 192 phonemes
    is status 2, all O, score 0; its neighbours, decoded with 70 phonemes before and after that call, are bit for bit what they are
    when all three are decoded with 70 phonemes.  The cap is wfl_decode_bigram's at every D."""
    rng = np.random.default_rng(31)
    C, big = make_table(192)
    _, table = make_table(70)
    W, Wbig = make_trans(70, rng), make_trans(192, rng)
    dur, sd = make_dur(70, 8, rng)
    dbig, sbig = make_dur(192, 8, rng)
    T = [200, 150, 90]
    lg = torch.from_numpy(rng.standard_normal((sum(T), C)).astype(np.float32) * 3).cuda()
    all_ids, all_score, all_st = DC.bio_viterbi_duration(lg, T, table, W, dur, sd, 0.0)
    assert all_st.cpu().tolist() == [0, 0, 0]
    nb = lambda: DC.bio_viterbi_duration(lg, [T[0], T[2]], table, W, dur, sd, 0.0, frame_offsets=[0, T[0] + T[1]])   # noqa: E731
    before = nb()
    ids, score, st = DC.bio_viterbi_duration(lg, [T[1]], big, Wbig, dbig, sbig, 0.0, frame_offsets=[T[0]])
    after = nb()
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [DC.STATUS_OVER_CAP] and score.cpu().tolist() == [0.0]
    assert (ids[T[0]:T[0] + T[1]].cpu().numpy() == big[0]).all()
    assert DC.duration_workspace_bytes([T[1]], 192, 8) == 0
    for got in (before, after):
        assert got[2].cpu().tolist() == [0, 0]
        for a in (slice(0, T[0]), slice(T[0] + T[1], sum(T))):
            assert torch.equal(got[0][a], all_ids[a])
        assert got[1].cpu().numpy().tobytes() == all_score[[0, 2]].cpu().numpy().tobytes()
    # 191 phonemes are inside the cap at the largest D
    _, t191 = make_table(191)
    d191, s191 = make_dur(191, 32, rng)
    st = DC.bio_viterbi_duration(lg, [T[0]], t191, make_trans(191, rng), d191, s191, 0.0)[2]
    assert st.cpu().tolist() == [0]


def test_a_bad_class_table_or_row_is_status_4():
    rng = np.random.default_rng(9)
    C = 141
    z = rng.standard_normal((20, C)).astype(np.float32)
    lg = torch.from_numpy(np.concatenate([z, z])).cuda()
    for pairs in ([(1, 2), (C + 3, 4)],          # a B class out of range
                  [(1, 2), (3, C)],              # an I class out of range
                  [(1, 2), (3, -2)],             # -1 alone means "no I class"
                  [(1, 2), (3, 2)],              # a class used twice
                  [(1, 2), (0, 4)],              # the O class used as a B class
                  [(p + 1, -1) for p in range(C - 1)] + [(5, -1)]):   # more phonemes than classes
        P = len(pairs)
        dur, sd = make_dur(P, 4, rng)
        ids, score, status = DC.bio_viterbi_duration(lg, [20, 20], (0, pairs), make_trans(P, rng), dur, sd, 0.0)
        assert status.cpu().tolist() == [DC.STATUS_BAD_CLASS] * 2, pairs[:3]
        assert (ids.cpu().numpy() == 0).all() and score.cpu().tolist() == [0.0, 0.0]
    table, W = (0, [(1, 2), (3, 4)]), make_trans(2, rng)
    dur = np.zeros((3, 5), np.float32)
    for sd in ([0, -2], [3, 0]):                 # below -1; n_rows
        ids, score, status = _raw(lg, [20, 20], table, W, dur, sd, 0.0)
        assert status.cpu().tolist() == [DC.STATUS_BAD_CLASS] * 2, sd
        assert (ids.cpu().numpy() == 0).all() and score.cpu().tolist() == [0.0, 0.0]
    for sd in ([2, -1], [0, 0]):
        assert _raw(lg, [20, 20], table, W, dur, sd, 0.0)[2].cpu().tolist() == [0, 0]


def test_empty_batch_empty_clip_and_a_table_without_phonemes():
    C, table = make_table(2)
    rng = np.random.default_rng(1)
    W = make_trans(2, rng)
    dur, sd = make_dur(2, 3, rng)
    assert _run([], table, W, dur, sd, 0.0, C) == []
    ids, score, status = DC.bio_viterbi_duration(torch.zeros((0, C), device="cuda"), [0], table, W, dur, sd, 0.0)
    assert status.cpu().tolist() == [0] and ids.numel() == 0 and score.cpu().tolist() == [0.0]
    z = np.random.default_rng(2).standard_normal((30, C)).astype(np.float32)
    for d in (dur, np.zeros((0, 4), np.float32)):                       # no phoneme: O everywhere; also without any row
        got = _run([z], (1, []), np.zeros((1, 1), np.float32), d, np.zeros(0, np.int32), 0.0, C)
        assert got[0][2] == 0 and (got[0][0] == 1).all()


def test_argument_checks_of_the_python_entry():
    P = 3
    C, table = make_table(P)
    lg = torch.zeros((10, C), device="cuda")
    rng = np.random.default_rng(0)
    W = make_trans(P, rng)
    dur = (-rng.random((2, 5))).astype(np.float32)
    sd = np.array([0, -1, 1], np.int32)
    call = lambda **kw: DC.bio_viterbi_duration(lg, [10], table, kw.get("W", W), kw.get("dur", dur), kw.get("sd", sd), kw.get("thr", 0.0))  # noqa: E731
    assert call()[2].cpu().tolist() == [0]
    for bad, what in ((np.nan, "dur holds a NaN"), (np.inf, r"dur holds \+inf")):
        d = dur.copy()
        d[1, 2] = bad
        with pytest.raises(ValueError, match=what):
            call(dur=d)
    d = dur.copy()
    d[0, 4] = 0.5
    with pytest.raises(ValueError, match="tail of dur"):
        call(dur=d)
    d[0, 4] = -np.inf                            # a forbidden tail is fine
    assert call(dur=d)[2].cpu().tolist() == [0]
    with pytest.raises(ValueError, match="dur must be float32"):
        call(dur=dur.astype(np.float64))
    for shape in ((2, 1), (2, 34), (10,)):
        with pytest.raises(ValueError, match=r"dur must be a \[rows, D \+ 1\]"):
            call(dur=np.zeros(shape, np.float32))
    with pytest.raises(ValueError, match="sym_dur must be int32"):
        call(sd=sd.astype(np.int64))
    with pytest.raises(ValueError, match="sym_dur must hold one row per phoneme"):
        call(sd=sd[:2])
    for bad in (-2, 2):
        s = sd.copy()
        s[1] = bad
        with pytest.raises(ValueError, match="sym_dur must lie in -1 .. 1"):
            call(sd=s)
    Wb = W.copy()
    Wb[2, 3] = np.nan
    with pytest.raises(ValueError, match="trans holds a NaN"):
        call(W=Wb)
    with pytest.raises(ValueError, match="threshold"):
        call(thr=-0.5)
