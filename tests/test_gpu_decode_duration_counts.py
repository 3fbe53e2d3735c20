"""-m gpu: wfl_decode_duration_counts (csrc/decode_duration_counts.hip) against the float64 expected run lengths and successions of
tests/bio_duration_counts_ref.py, on the seeded logits, transition tables and duration tables of
tests/test_gpu_decode_duration_posterior.py, ragged batches, scattered layout.  Every entry of logz, succ and dur_counts of every
status-0 clip is compared, and the two tables' totals.

Tolerances (none is a constant; the rule of tests/test_gpu_decode_bigram_counts.py): for every case the float32 log-domain restatement
of the reference (recurrences, each term's exponent and the running sums in fp32, renormalised every 16 frames, offsets in float64) is
run on the same inputs; its maximum deviation from float64 over the case -- separately for logz, the entries of succ, the entries of
dur_counts and the two totals -- is the yardstick, and the kernel is allowed 4 x that against float64, plus half an fp32 ulp of the
value where that half ulp exceeds the yardstick.  A value float64 puts below 1e-30 may be 0.  The figures are printed before anything
is asserted.

Seeds: the clip and table seeds of tests/test_gpu_decode_duration_posterior.py (no frame within MARGIN of the threshold;
forced_frames asserts it) wherever the float64 tables of the case meet the conditions asserted in test_ragged_batch_against_float64
(dur_counts: an entry in (0, 1e-3), an entry above 0.5, a forbidden entry, a nonzero column D where D <= 8; succ: an entry in
(0, 1e-3), an entry above 0.5, a forbidden entry with forbid > 0); the exceptions, found on the CPU under these rules, are listed in
CLIP_SEEDS / TABLE_SEEDS.  With one phoneme and D = 1 the table has two entries: the rule on small and forbidden entries of
dur_counts is asked of the cases with more than two entries.  COLUMN_D_OUT_OF_REACH lists the one case whose generators cannot reach
column D.

Measured on one MI355X over this file's cases (kernel against float64 | the float32 restatement, the yardstick): the entries of
dur_counts deviate by at most 6.6e-5 and those of succ by at most 5.3e-5 (the 2000-frame clip | 1.7e-3), in no case by more than
0.45 x the yardstick; the totals by at most 1.1e-4 (| 2.2e-3); logz by at most 4.6e-5, where half an fp32 ulp decides.  logz equals
wfl_decode_duration_posterior's bit for bit, and wfl_decode_bigram_counts' without a prior (succ within 1.9e-6).  
"""
import functools

import numpy as np
import pytest
import torch

import bio_bigram_counts_ref as BC
import bio_duration_counts_ref as CR
import bio_duration_posterior_ref as DP
import bio_duration_ref as R
import test_gpu_decode_duration as SD
import test_gpu_decode_duration_posterior as TP
from test_gpu_decode_bigram_posterior import _allowed, _layout
from wfl_asr_amd import decode as DC

pytestmark = pytest.mark.gpu
MARGIN = SD.MARGIN
LENGTHS, CASES, CONFIGS = SD.LENGTHS, SD.CASES, TP.CONFIGS
KINDS = ("logz", "succ", "dur", "succ_total", "dur_total")
# (P, D, k) -> seed where the posterior test's seed does not meet this file's conditions on the inputs
CLIP_SEEDS = {}
TABLE_SEEDS = {(1, 1, 1): 40030, (2, 8, 1): 40005}
# the tiny clips: D -> seed (default 7300 + D, the siblings'), where the sibling's table gives the phonemes with an I class no tail
TINY_SEEDS = {1: 7331, 2: 7312}
# (64, 8) at threshold 0.5: with 132 classes the generators leave no stretch of D + 1 = 9 frames free of forced frames (the longest is
# 4, in each of 400 clip seeds tried), so no run can pass its D-th frame and column D is 0 in the reference whatever the seed.  The case
# stays, the stretch is asserted, and column D must then be exactly 0 in the kernel's output too.
COLUMN_D_OUT_OF_REACH = {(64, 8, 1)}


def longest_free_stretch(z, thr):
    best = cur = 0
    for f in SD.forced_frames(z, thr)[1]:
        cur = 0 if f else cur + 1
        best = max(best, cur)
    return best


def forbidden_durations(dur, sd):
    """[P, D + 1] bool: the entries of dur_counts the table forbids (lambda = 0; column D: tau = 0 or lambda(D) = 0)."""
    dur = np.asarray(dur)
    D = dur.shape[1] - 1
    out = np.zeros((len(sd), D + 1), bool)
    for p, r in enumerate(sd):
        if r >= 0:
            out[p] = np.isneginf(dur[r])
            out[p, D] |= np.isneginf(dur[r, D - 1])
    return out


def _run(clips, table, W, dur, sd, thr, C, scattered=False):
    """clips: list of z [T, C] float32 -> per clip dict(logz, succ, dur, status), numpy."""
    T = [len(c) for c in clips]
    offs, host = _layout(clips, C, scattered)
    lg = torch.from_numpy(host).cuda()[:, :C]
    logz, succ, dc, st = DC.duration_expected_counts(lg, T, table, W, dur, sd, thr, frame_offsets=offs)
    torch.cuda.synchronize()
    logz, succ, dc, st = logz.cpu().numpy(), succ.cpu().numpy(), dc.cpu().numpy(), st.cpu().numpy()
    n, D = len(table[1]) + 1, np.asarray(dur).shape[1] - 1
    assert succ.shape == (len(clips), n, n) and dc.shape == (len(clips), n - 1, D + 1) and succ.dtype == dc.dtype == np.float32
    return [dict(logz=np.float32(logz[b]), succ=succ[b], dur=dc[b], status=int(st[b])) for b in range(len(clips))]


def _kinds(logz, succ, dc):
    return dict(logz=np.float64(logz), succ=np.asarray(succ, np.float64), dur=np.asarray(dc, np.float64),
                succ_total=np.float64(np.asarray(succ, np.float64).sum()), dur_total=np.float64(np.asarray(dc, np.float64).sum()))


def _reference(clips, table, W, dur, sd, thr, brute=False):
    """-> (per clip the float64 kinds, yardsticks per kind)."""
    W64 = np.asarray(W, np.float64)
    refs, yard = [], {k: 0.0 for k in KINDS}
    for z in clips:
        _, forced = SD.forced_frames(z, thr)
        r64 = _kinds(*(CR.brute_force(z, table, W64, dur, sd, forced) if brute and len(z) else CR.expected_counts(z, table, W64, dur, sd, forced)))
        r32 = _kinds(*CR.expected_counts(z, table, W64, dur, sd, forced, dtype=np.float32))
        for k in KINDS:
            if np.size(r64[k]):
                yard[k] = max(yard[k], float(np.abs(r32[k] - r64[k]).max()))
        refs.append(r64)
    return refs, yard


def _dev(mine, ref):
    d = np.abs(np.asarray(mine, np.float64) - ref)
    return np.where((np.asarray(mine) == 0) & (ref < 1e-30), 0.0, d)


def _check_case(name, clips, W, dur, sd, got, refs, yard):
    """Every clip of a case against float64 by the 4 x yardstick rule, and the identities on the kernel's own output; prints the
    figures before it asserts.  -> what logz was allowed, per clip."""
    shut = np.isneginf(np.asarray(W, np.float64))
    forb = forbidden_durations(dur, sd)
    D = np.asarray(dur).shape[1] - 1
    dev = {k: 0.0 for k in KINDS}
    over = {k: -np.inf for k in KINDS}
    ident = [0.0, -np.inf]
    allowed_logz = []
    for z, g, r in zip(clips, got, refs):
        assert g["status"] == 0, (name, g["status"])
        mine = _kinds(g["logz"], g["succ"], g["dur"])
        for k in KINDS:
            assert np.isfinite(mine[k]).all(), (name, k)
        assert (mine["succ"] >= 0).all() and mine["succ"][0, 0] == 0.0 and (mine["succ"][shut] == 0.0).all(), name
        assert (mine["dur"] >= 0).all() and (mine["dur"][forb] == 0.0).all(), name
        if not len(z):
            assert g["logz"] == 0 and not mine["succ"].any() and not mine["dur"].any()
            allowed_logz.append(0.0)
            continue
        for k in KINDS:
            if np.size(r[k]):
                d = _dev(mine[k], r[k])
                dev[k] = max(dev[k], float(np.max(d)))
                over[k] = max(over[k], float(np.max(d - _allowed(yard[k], r[k]))))
        # every run is opened once: the runs of p by length = column 1 + p of succ, within the two allowances summed over the terms
        if mine["dur"].size:
            runs, col = mine["dur"][:, :D].sum(1), mine["succ"][:, 1:].sum(0)
            allow = _allowed(yard["dur"], r["dur"][:, :D]).sum(1) + _allowed(yard["succ"], r["succ"][:, 1:]).sum(0)
            ident[0] = max(ident[0], float(np.abs(runs - col).max()))
            ident[1] = max(ident[1], float((np.abs(runs - col) - allow).max()))
            lens = np.concatenate([np.arange(1, D + 1), [1]])
            assert (mine["dur"] * lens).sum() <= len(z) + float((_allowed(yard["dur"], r["dur"]) * lens).sum()), name
        allowed_logz.append(float(_allowed(yard["logz"], r["logz"])))
    for k in KINDS:
        print(f"{name}: {k}: kernel {dev[k]:.3e}, float32 restatement {yard[k]:.3e}, allowed 4 x = {4 * yard[k]:.3e} (+ half an fp32 ulp "
              f"where that exceeds the restatement), over by {max(over[k], 0.0):.3e}")
    print(f"{name}: runs by length against succ's columns: {ident[0]:.3e}, over the summed allowances by {max(ident[1], 0.0):.3e}")
    for k in KINDS:
        assert over[k] <= 0, (name, k, dev[k], yard[k], over[k])
    assert ident[1] <= 0, (name, ident)
    return allowed_logz


@functools.lru_cache(maxsize=None)
def ragged_case(P, D, k):
    """The inputs of a ragged case and their references, computed once: (C, table, clips, W, dur, sd, thr, refs, yard)."""
    seed = CLIP_SEEDS.get((P, D, k), TP.CLIP_SEEDS_K.get((P, D, k), TP.CLIP_SEEDS.get((P, D), SD.SEEDS[P])))
    C, table, clips = SD.make_clips(P, seed)
    if (P, D, k) in TABLE_SEEDS:
        rng = np.random.default_rng(TABLE_SEEDS[(P, D, k)])
        W = SD.make_trans(P, rng, CONFIGS[k][0])
        dur, sd = SD.make_dur(P, D, rng)
        thr = CONFIGS[k][1]
    else:
        W, dur, sd, thr = TP.case_tables(P, D, k)
    refs, yard = _reference(clips, table, W, dur, sd, thr)
    return C, table, clips, W, dur, sd, thr, refs, yard


def input_conditions(P, D, k, W, dur, sd, refs, clips):
    """The conditions on a ragged case's inputs, on the reference alone -> the list of those it misses."""
    live = [r for r, z in zip(refs, clips) if len(z)]
    dc = np.stack([r["dur"] for r in live])
    sc = np.concatenate([r["succ"].ravel() for r in live])
    forb = forbidden_durations(dur, sd)
    shut = np.isneginf(W)
    shut[0, 0] = False
    miss = []
    if dc[0].size > 2:
        if not ((dc > 0) & (dc < 1e-3)).any():
            miss.append("no dur_counts entry in (0, 1e-3)")
        if not forb.any() or dc[:, forb].any():
            miss.append("no forbidden dur_counts entry that is 0")
    if not dc.max() > 0.5:
        miss.append("no dur_counts entry above 0.5")
    if (P, D, k) in COLUMN_D_OUT_OF_REACH:
        if not max(longest_free_stretch(z, CONFIGS[k][1]) for z in clips) <= D or dc[:, :, D].any():
            miss.append("column D is within reach after all")
    elif D <= 8 and not dc[:, :, D].any():
        miss.append("column D is all zero")
    if not (((sc > 0) & (sc < 1e-3)).any() and sc.max() > 0.5):
        miss.append("succ does not span the range")
    if CONFIGS[k][0] > 0 and not shut.any():
        miss.append("no forbidden succession")
    return miss


@pytest.mark.parametrize("P,D", CASES)
@pytest.mark.parametrize("k", [0, 1])
def test_ragged_batch_against_float64(P, D, k):
    C, table, clips, W, dur, sd, thr, refs, yard = ragged_case(P, D, k)
    miss = input_conditions(P, D, k, W, dur, sd, refs, clips)
    assert not miss, f"test setup: {miss}"
    got = _run(clips, table, W, dur, sd, thr, C, scattered=True)
    e = got[LENGTHS.index(0)]
    assert e["status"] == 0 and not e["succ"].any() and not e["dur"].any()
    if (P, D, k) in COLUMN_D_OUT_OF_REACH:
        assert not any(g["dur"][:, D].any() for g in got)
    _check_case(f"P{P} D{D} forbid {CONFIGS[k][0]} thr {thr}", clips, W, dur, sd, got, refs, yard)


@pytest.mark.parametrize("D", [1, 2, 3, 8])
def test_tiny_clips_against_the_enumeration(D):
    """100 clips of 1 .. 6 frames in one call against every class string enumerated: the off-by-one cases of the ring, the tail and the
    cut-off run in all three sweeps.  At D <= 3 the tail and column D are reached; at D = 8 the ring never fills."""
    rng = np.random.default_rng(TINY_SEEDS.get(D, 7300 + D))
    clips = [(rng.standard_normal((int(rng.integers(1, 7)), SD.TINY_C)) * 2).astype(np.float32) for _ in range(100)]
    W = (-3.0 * rng.random((4, 4))).astype(np.float32)
    mask = rng.random((4, 4)) < 0.2
    mask[:, 0] = False
    W[mask] = -np.inf
    dur, sd = SD.make_dur(3, D, rng, forbid=0.25)
    refs, yard = _reference(clips, SD.TINY, W, dur, sd, SD.THRESHOLD, brute=True)
    if D <= 3:
        assert any(r["dur"][:, D].any() for r in refs), "column D is never reached (test setup)"
    got = _run(clips, SD.TINY, W, dur, sd, SD.THRESHOLD, SD.TINY_C)
    _check_case(f"tiny D{D}", clips, W, dur, sd, got, refs, yard)


@pytest.mark.parametrize("prior", ["none", "zero"])
def test_without_a_prior_it_is_wfl_decode_bigram_counts(prior):
    """Every sym_dur = -1, and an all-zero table: succ and logz within the two entries' allowances of wfl_decode_bigram_counts."""
    for P, D in ((2, 1), (70, 8), (70, 32)):
        C, table = SD.make_table(P)
        rng = np.random.default_rng(40 + P + D)
        clips = [R.plant(T, C, table, rng, margin=4.0, scale=2.0)[0] for T in (33, 300)]
        W = SD.make_trans(P, rng)
        dur = np.zeros((3, D + 1), np.float32)
        sd = np.full(P, -1, np.int32) if prior == "none" else rng.integers(0, 3, size=P).astype(np.int32)
        refs, yard = _reference(clips, table, W, dur, sd, 0.0)
        got = _run(clips, table, W, dur, sd, 0.0, C)
        _check_case(f"{prior} P{P} D{D}", clips, W, dur, sd, got, refs, yard)
        lg = torch.from_numpy(np.concatenate(clips)).cuda()
        blz, bcn, bst = DC.bigram_expected_counts(lg, [len(c) for c in clips], table, W, 0.0)
        assert bst.cpu().tolist() == [0, 0]
        blz, bcn = blz.cpu().numpy().astype(np.float64), bcn.cpu().numpy().astype(np.float64)
        W64 = np.asarray(W, np.float64)
        for b, (z, g, r) in enumerate(zip(clips, got, refs)):
            b64, b32 = BC.expected_counts(z, table, W64, None), BC.expected_counts(z, table, W64, None, dtype=np.float32)
            assert abs(b64[0] - r["logz"]) <= 1e-9 * abs(b64[0]) and np.abs(b64[1] - r["succ"]).max() <= 1e-9   # one reference
            a_lz = float(_allowed(yard["logz"], r["logz"]) + _allowed(abs(b32[0] - b64[0]), r["logz"]))
            a_cn = _allowed(yard["succ"], r["succ"]) + _allowed(float(np.abs(b32[1] - b64[1]).max()), r["succ"])
            d_lz, d_cn = abs(float(g["logz"]) - blz[b]), np.abs(g["succ"].astype(np.float64) - bcn[b])
            print(f"{prior} P{P} D{D} T {len(z)}: between the two entries: logz {d_lz:.3e} (allowed {a_lz:.3e}), succ {d_cn.max():.3e} "
                  f"(allowed {a_cn.max():.3e})")
            assert d_lz <= a_lz and (d_cn <= a_cn).all()


@pytest.mark.parametrize("P,D", [(2, 8), (65, 32), (191, 32)])
def test_logz_equals_the_posterior_entry(P, D):
    """wfl_decode_duration_posterior on the search's own path: the two logz agree within the sum of the two allowances."""
    C, table, clips, W, dur, sd, thr, refs, yard = ragged_case(P, D, 1)
    got = TP._run(clips, table, W, dur, sd, thr, C)
    mine = _run(clips, table, W, dur, sd, thr, C)
    W64 = np.asarray(W, np.float64)
    pyard = 0.0
    for z, g in zip(clips, got):
        if len(z):
            _, forced = SD.forced_frames(z, thr)
            a = DP.forward_backward(z, table, W64, dur, sd, forced, g["ids"])[0]
            b = DP.forward_backward(z, table, W64, dur, sd, forced, g["ids"], dtype=np.float32)[0]
            pyard = max(pyard, abs(a - b))
    for z, g, m, r in zip(clips, got, mine, refs):
        assert g["status"] == 0 and m["status"] == 0
        allow = float(_allowed(yard["logz"], r["logz"])) + float(_allowed(pyard, r["logz"])) if len(z) else 0.0
        d = abs(float(m["logz"]) - float(g["logz"][0]))
        print(f"P{P} D{D} T {len(z)}: logz counts {float(m['logz']):.6f} posterior {float(g['logz'][0]):.6f}; differ by {d:.3e}, allowed {allow:.3e}")
        assert d <= allow


@pytest.mark.parametrize("kind", ["minimum", "maximum"])
def test_hard_bounds_give_exact_zeros(kind):
    """tests/test_gpu_decode_duration.py's arrangements, P = 20.  Hard minimum: L(1) = L(2) = -inf gives columns 0 and 1 exactly 0.  Hard
    maximum: everything beyond 3 frames is -inf, the tail included: columns >= 3 and the excess are exactly 0."""
    P, D = 20, (6 if kind == "minimum" else 5)
    C, table = 2 * P + 4, (1, [(2 + 2 * p, 3 + 2 * p) for p in range(P)])
    rng = np.random.default_rng(71 if kind == "minimum" else 72)
    clips = [TP._plant_stretches(T, C, table, rng, (3, 9) if kind == "minimum" else (1, 3), margin=8.0)[0] for T in (150, 61)]
    W = SD.make_trans(P, rng)
    dur = (-2.0 * rng.random((P, D + 1))).astype(np.float32)
    if kind == "minimum":
        dur[:, :2] = -np.inf
    else:
        dur[:, 3:] = -np.inf
    sd = np.arange(P, dtype=np.int32)
    refs, yard = _reference(clips, table, W, dur, sd, 0.0)
    got = _run(clips, table, W, dur, sd, 0.0, C)
    _check_case(f"hard {kind}", clips, W, dur, sd, got, refs, yard)
    for g in got:
        assert g["dur"].any()
        assert not (g["dur"][:, :2].any() if kind == "minimum" else g["dur"][:, 3:].any())


def test_a_long_run_is_counted_once_and_its_excess_by_frames():
    """D = 4 and a planted run of 40 frames of phoneme 2 between two stretches of O (P = 5), sharp enough that its posterior is above
    0.99 (asserted on the reference): column D - 1 holds the run once and column D its 36 frames past the fourth, within the
    reference's own allowance (the planted margin of 30 nats puts every other segmentation below e^-30)."""
    P, D = 5, 4
    C, table = 2 * P + 4, (1, [(2 + 2 * p, 3 + 2 * p) for p in range(P)])
    rng = np.random.default_rng(12)
    ids = np.full(100, 1, np.int32)
    ids[30], ids[31:70] = 6, 7
    z = rng.standard_normal((100, C))
    z[np.arange(100), ids] += 30.0
    z = z.astype(np.float32)
    W = SD.make_trans(P, rng)
    dur = (-2.0 * rng.random((P, D + 1))).astype(np.float32)
    sd = np.arange(P, dtype=np.int32)
    refs, yard = _reference([z], table, W, dur, sd, 0.0)
    post = refs[0]["dur"][2, D - 1]
    assert post > 0.99, post
    assert abs(refs[0]["dur"][2, D] - 36 * post) <= float(_allowed(yard["dur"], refs[0]["dur"][2, D]))
    got = _run([z], table, W, dur, sd, 0.0, C)
    _check_case("long run", [z], W, dur, sd, got, refs, yard)


def test_one_2000_frame_clip():
    """Past one 30 s chunk's 1500 frames: the integer exponent sums and the accumulators over many frames."""
    P, D = 70, 32
    C, table, clips = SD.make_clips(P, 11077, lengths=[2000])
    rng = np.random.default_rng(78)
    W = SD.make_trans(P, rng, 0.3)
    dur, sd = SD.make_dur(P, D, rng)
    refs, yard = _reference(clips, table, W, dur, sd, SD.THRESHOLD)
    _check_case("T2000", clips, W, dur, sd, _run(clips, table, W, dur, sd, SD.THRESHOLD, C), refs, yard)


def test_a_dominant_class_outside_the_grammar():
    """tests/test_gpu_decode_bigram_counts.py's case: a never-chosen class stands 30 nats above everything on every frame, and an I
    class dominates frames where no path can reach it: the frame constants are large; the same rule, and nothing is inf or NaN."""
    P, D = 64, 8
    C, table = SD.make_table(P)
    rng = np.random.default_rng(77)
    a = (rng.standard_normal((200, C)) * 3).astype(np.float32)
    a[:, 0] += 30.0
    b = R.plant(150, C, table, rng, margin=4.0, scale=2.0)[0]
    b[::3, 3] += 30.0
    W = SD.make_trans(P, np.random.default_rng(79), 0.3)
    dur, sd = SD.make_dur(P, D, rng)
    refs, yard = _reference([a, b], table, W, dur, sd, 0.0)
    _check_case("off_grammar", [a, b], W, dur, sd, _run([a, b], table, W, dur, sd, 0.0, C), refs, yard)


def test_a_clip_alone_equals_the_clip_in_a_batch_of_16():
    P, D = 70, 8
    C, table = SD.make_table(P)
    rng = np.random.default_rng(3)
    W = SD.make_trans(P, rng, 0.3)
    dur, sd = SD.make_dur(P, D, rng)
    clips = [(rng.standard_normal((int(rng.integers(1, 200)), C)) * 3).astype(np.float32) for _ in range(16)]
    batch = _run(clips, table, W, dur, sd, 0.0, C)
    for b in (0, 5, 15):
        alone = _run([clips[b]], table, W, dur, sd, 0.0, C)[0]
        assert alone["status"] == batch[b]["status"] == 0
        for k in ("logz", "succ", "dur"):
            assert alone[k].tobytes() == batch[b][k].tobytes(), k
        assert alone["succ"].any() and alone["dur"].any()


def test_symbol_cap_is_status_2_and_needs_no_workspace():
    P, D = 192, 8
    C, table = SD.make_table(P)
    rng = np.random.default_rng(31)
    lg = torch.from_numpy(rng.standard_normal((50, C)).astype(np.float32)).cuda()
    assert DC.duration_counts_workspace_bytes([20, 30], P, D) == 0 and DC.duration_counts_workspace_bytes([20, 30], P - 1, D) > 0
    dur, sd = SD.make_dur(P, D, rng)
    logz, succ, dc, st = DC.duration_expected_counts(lg, [20, 30], table, SD.make_trans(P, rng), dur, sd, 0.0)
    assert st.cpu().tolist() == [DC.STATUS_OVER_CAP] * 2 and logz.cpu().tolist() == [0.0, 0.0]
    assert succ.shape == (2, P + 1, P + 1) and not succ.cpu().numpy().any() and dc.shape == (2, P, D + 1) and not dc.cpu().numpy().any()


def test_class_cap_is_status_2():
    rng = np.random.default_rng(31)
    lg = torch.from_numpy(rng.standard_normal((50, 1025)).astype(np.float32)).cuda()
    pairs = [(2 * p + 1, 2 * p + 2) for p in range(100)]
    dur, sd = SD.make_dur(100, 4, rng)
    logz, succ, dc, st = DC.duration_expected_counts(lg, [20, 30], (0, pairs), SD.make_trans(100, rng), dur, sd, 0.0)
    assert st.cpu().tolist() == [DC.STATUS_OVER_CAP] * 2 and logz.cpu().tolist() == [0.0, 0.0]
    assert not succ.cpu().numpy().any() and not dc.cpu().numpy().any()


def _raw(lg, T, table, W, dur, sd, thr):
    """The ABI entry without the Python entry's checks of dur and sym_dur (for the statuses those checks would pre-empt)."""
    clips = DC._check_clips(lg, T, table, 0.0, thr, None)
    dur = np.ascontiguousarray(dur, np.float32)
    D, nb, n = dur.shape[1] - 1, len(T), len(table[1]) + 1
    logz = torch.empty(nb, dtype=torch.float32, device="cuda")
    succ = torch.full((nb, n, n), -7.0, dtype=torch.float32, device="cuda")
    dc = torch.full((nb, n - 1, D + 1), -7.0, dtype=torch.float32, device="cuda")
    st = torch.empty(nb, dtype=torch.int32, device="cuda")
    DC._call("wfl_decode_duration_counts", lg, clips, (np.ascontiguousarray(W, np.float32), np.ascontiguousarray(sd, np.int32), dur, len(dur),
                                                       D, float(thr)), (logz, succ, dc, st), None, ws_more=(D,))
    torch.cuda.synchronize()
    return logz, succ, dc, st


def test_a_bad_class_table_or_row_is_status_4():
    rng = np.random.default_rng(9)
    C = 141
    z = rng.standard_normal((20, C)).astype(np.float32)
    lg = torch.from_numpy(np.concatenate([z, z])).cuda()
    for pairs in ([(1, 2), (3, 2)], [(1, 2), (0, 4)], [(1, 2), (150, 4)], [(p % 100 + 1, -1) for p in range(150)]):
        P = len(pairs)
        dur, sd = SD.make_dur(P, 4, rng)
        logz, succ, dc, st = DC.duration_expected_counts(lg, [20, 20], (0, pairs), SD.make_trans(P, rng), dur, sd, 0.0)
        assert st.cpu().tolist() == [DC.STATUS_BAD_CLASS] * 2 and logz.cpu().tolist() == [0.0, 0.0], pairs[:3]
        assert not succ.cpu().numpy().any() and not dc.cpu().numpy().any()
    table, W = (0, [(1, 2), (3, 4)]), SD.make_trans(2, rng)
    dur = np.zeros((3, 5), np.float32)
    for sd in ([0, -2], [3, 0]):                 # below -1; n_rows
        logz, succ, dc, st = _raw(lg, [20, 20], table, W, dur, sd, 0.0)
        assert st.cpu().tolist() == [DC.STATUS_BAD_CLASS] * 2 and logz.cpu().tolist() == [0.0, 0.0], sd
        assert not succ.cpu().numpy().any() and not dc.cpu().numpy().any()
    for sd in ([2, -1], [0, 0]):
        assert _raw(lg, [20, 20], table, W, dur, sd, 0.0)[3].cpu().tolist() == [0, 0]


def test_empty_clip_empty_batch_and_a_table_without_phonemes():
    P, D = 65, 8
    C, table = SD.make_table(P)
    rng = np.random.default_rng(2)
    W = SD.make_trans(P, rng, 0.3)
    dur, sd = SD.make_dur(P, D, rng)
    z = (rng.standard_normal((30, C)) * 3).astype(np.float32)
    clips = [z[:10], z[:0], z[10:]]
    got = _run(clips, table, W, dur, sd, 0.0, C)
    refs, yard = _reference(clips, table, W, dur, sd, 0.0)
    _check_case("with_an_empty_clip", clips, W, dur, sd, got, refs, yard)
    assert got[1]["status"] == 0 and got[1]["logz"] == 0 and not got[1]["succ"].any() and not got[1]["dur"].any()
    assert _run([], table, W, dur, sd, 0.0, C) == []
    lg = torch.zeros((0, C), device="cuda")
    logz, succ, dc, st = DC.duration_expected_counts(lg, [0], table, W, dur, sd, 0.0)
    assert st.cpu().tolist() == [0] and logz.cpu().tolist() == [0.0] and not succ.cpu().numpy().any() and not dc.cpu().numpy().any()
    # a table with no phoneme: O everywhere, one path, no run; also without any row of dur
    for d in (dur, np.zeros((0, 4), np.float32)):
        got = _run([z], (1, []), np.zeros((1, 1), np.float32), d, np.zeros(0, np.int32), 0.0, C)
        assert got[0]["status"] == 0 and got[0]["succ"].shape == (1, 1) and got[0]["succ"][0, 0] == 0.0 and got[0]["dur"].size == 0
        assert abs(float(got[0]["logz"]) - float(z[:, 1].astype(np.float64).sum())) <= 1e-4


def test_argument_checks_of_the_python_entry():
    P = 3
    C, table = SD.make_table(P)
    lg = torch.zeros((10, C), device="cuda")
    rng = np.random.default_rng(0)
    W = SD.make_trans(P, rng)
    dur = (-rng.random((2, 5))).astype(np.float32)
    sd = np.array([0, -1, 1], np.int32)
    call = lambda **kw: DC.duration_expected_counts(kw.get("lg", lg), kw.get("T", [10]), table, kw.get("W", W), kw.get("dur", dur),  # noqa: E731
                                                    kw.get("sd", sd), kw.get("thr", 0.0))
    assert call()[3].cpu().tolist() == [0]
    with pytest.raises(ValueError, match="float32 CUDA"):
        call(lg=lg.cpu())
    with pytest.raises(ValueError, match="past the logits"):
        call(T=[11])
    with pytest.raises(ValueError, match="threshold"):
        call(thr=-0.5)
    d = dur.copy()
    d[1, 2] = np.nan
    with pytest.raises(ValueError, match="dur holds a NaN"):
        call(dur=d)
    d = dur.copy()
    d[0, 4] = 0.5
    with pytest.raises(ValueError, match="tail of dur"):
        call(dur=d)
    with pytest.raises(ValueError, match=r"dur must be a \[rows, D \+ 1\]"):
        call(dur=np.zeros((2, 34), np.float32))
    with pytest.raises(ValueError, match="sym_dur must be int32"):
        call(sd=sd.astype(np.int64))
    with pytest.raises(ValueError, match="sym_dur must lie in -1 .. 1"):
        call(sd=np.array([0, 2, 1], np.int32))
    Wb = W.copy()
    Wb[2, 3] = np.nan
    with pytest.raises(ValueError, match="trans holds a NaN"):
        call(W=Wb)
    with pytest.raises(ValueError, match=r"\[4, 4\]"):
        call(W=W[:-1])
