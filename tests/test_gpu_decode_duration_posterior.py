"""-m gpu: wfl_decode_duration_posterior (csrc/decode_duration_posterior.hip) against the float64 semi-Markov forward-backward of
tests/bio_duration_posterior_ref.py, on the seeded logits, transition tables and duration tables of tests/test_gpu_decode_duration.py,
ragged batches.  The path given to the kernel and to the reference is wfl_decode_duration's own output for the same clips, so
near-ties of the search cannot matter.  Every frame of every status-0 clip is compared.

Tolerances (none is a constant here; the rule of tests/test_gpu_decode_bigram_posterior.py, whose helpers are imported): for every
case the float32 log-domain restatement of the reference (renormalised every 16 frames, ring and tail state included, offsets in
float64) is run on the same inputs and the same path; its maximum deviation from float64 over the case -- separately for logz, post
and cls_post -- is the yardstick, and the kernel is allowed 4 x that against float64, plus half an fp32 ulp of the value where that
exceeds the yardstick.  A value the float64 reference puts below 1e-30 may be 0 (the kernel runs in the scaled linear domain).

Seeds: chosen on the CPU so that no frame's largest softmax probability is within MARGIN = 1e-4 of the threshold (asserted) and so
that the float64 posteriors of every ragged case span the range (some < 0.2, some > 0.99, some in (0.3, 0.7); asserted).  The clip
seeds of tests/test_gpu_decode_duration.py do both for every case but those listed in CLIP_SEEDS.

Shapes: the search's own corner set -- LENGTHS, and (P, D) of test_gpu_decode_duration.CASES: (191, 1) keeps the ring in LDS,
(191, 32) puts it in the workspace, 64 / 65 straddle a lane group, T < D is a ring that never fills.

Measured on one MI355X over this file's cases (kernel against float64 | the float32 restatement, the yardstick): post and cls_post
deviate by at most 6.6e-6 (the 6000-frame clip | 6.5e-5) and in no case by more than 0.28 x the yardstick (the tiny clips against the
enumeration: 3.1e-7 | 1.1e-6); the ragged cases lie between 2.6e-7 and 1.2e-6 | 4.8e-6 to 5.2e-5.  logz: at most 6.7e-4, on the
hard-minimum clips, where |logz| is near 2e4 and half an fp32 ulp is 9.8e-4 (| 1.4e-4); on the ragged cases at most 1.5e-5, where the
half ulp decides (| 1.2e-6).  Under the hard minimum and the hard maximum every output is finite and post is within 4.8e-7 of
float64.  With every sym_dur = -1 and with an all-zero table the entry and wfl_decode_bigram_posterior differ by at most 1.3e-6 per
posterior and by 0 in logz (allowed 3.5e-4 and 2e-4).  
"""
import numpy as np
import pytest
import torch

import bio_bigram_posterior_ref as BP
import bio_bigram_ref as RB
import bio_duration_posterior_ref as DP
import bio_duration_ref as R
import bio_posterior_ref as P1
import test_gpu_decode_bigram_posterior as TB
import test_gpu_decode_duration as SD
from wfl_asr_amd import decode as DC

pytestmark = pytest.mark.gpu
MARGIN = SD.MARGIN
KEYS = TB.KEYS
LENGTHS = [1, 2, 15, 16, 17, 0, 31, 32, 33, 300]
CASES = [(1, 1), (2, 32), (2, 8), (64, 8), (65, 2), (65, 32), (191, 1), (191, 32)]
assert LENGTHS == SD.LENGTHS and CASES == SD.CASES
CONFIGS = [(0.0, 0.0), (0.3, SD.THRESHOLD)]                 # (share of forbidden successions, threshold)
# (P, D) -> clip seed (default: test_gpu_decode_duration.SEEDS[P]) and table seed (default: 1000 + 40 P + D; configuration k adds 7 k),
# found on the CPU under both rules.  With one or two phonemes the path's class rarely falls below 0.2 (one table in fifty does it), so
# (1, 1) and (2, 32) have seeds per configuration, (P, D, k) -> seed
CLIP_SEEDS = {(2, 8): 503, (64, 8): 364, (65, 2): 366, (191, 32): 495}
TABLE_SEEDS = {(2, 8): 3088, (64, 8): 4568, (65, 2): 5602, (65, 32): 3632, (191, 1): 8641, (191, 32): 8672}
CLIP_SEEDS_K = {(1, 1, 0): 855, (1, 1, 1): 101, (2, 32, 0): 102, (2, 32, 1): 503}
TABLE_SEEDS_K = {(1, 1, 0): 30007, (1, 1, 1): 30059, (2, 32, 0): 30003, (2, 32, 1): 30000}
_allowed, _deviation, _half_ulp, _layout = TB._allowed, TB._deviation, TB._half_ulp, TB._layout


def case_tables(P, D, k):
    """The tables of configuration k of case (P, D) -> (W, dur, sym_dur, threshold)."""
    rng = np.random.default_rng(TABLE_SEEDS_K.get((P, D, k), TABLE_SEEDS.get((P, D), 1000 + 40 * P + D) + 7 * k))
    forbid, thr = CONFIGS[k]
    W = SD.make_trans(P, rng, forbid)
    dur, sd = SD.make_dur(P, D, rng)
    return W, dur, sd, thr


def _run(clips, table, W, dur, sd, thr, C, scattered=False, ids_edit=None, bigram=False):
    """clips: list of z [T, C] float32 -> per clip dict(ids, score, vstatus, logz, post, cls_post, status), numpy.  The path is
    wfl_decode_duration's (bigram: wfl_decode_bigram's, and wfl_decode_bigram_posterior's outputs as big_*)."""
    T = [len(c) for c in clips]
    offs, host = _layout(clips, C, scattered)
    lg = torch.from_numpy(host).cuda()[:, :C]
    if bigram:
        ids, score, vst = DC.bio_viterbi_bigram(lg, T, table, W, thr, frame_offsets=offs)
    else:
        ids, score, vst = DC.bio_viterbi_duration(lg, T, table, W, dur, sd, thr, frame_offsets=offs)
    if ids_edit is not None:
        ids = ids_edit(ids.clone(), offs)
    logz, post, cls, st = DC.decode_posteriors_duration(lg, T, table, W, dur, sd, thr, ids, frame_offsets=offs)
    outs = [ids, score, vst, logz, post, cls, st]
    if bigram:
        outs += list(DC.decode_posteriors_bigram(lg, T, table, W, thr, ids, frame_offsets=offs))
    torch.cuda.synchronize()
    outs = [x.cpu().numpy() for x in outs]
    ids, score, vst, logz, post, cls, st = outs[:7]
    got = [dict(ids=ids[o:o + t], score=float(score[b]), vstatus=int(vst[b]), logz=np.array([logz[b]], np.float32), post=post[o:o + t],
                cls_post=cls[o:o + t], status=int(st[b])) for b, (o, t) in enumerate(zip(offs, T))]
    if bigram:
        bz, bp, bc, bs = outs[7:]
        for b, (o, t) in enumerate(zip(offs, T)):
            got[b].update(big_logz=np.array([bz[b]], np.float32), big_post=bp[o:o + t], big_cls_post=bc[o:o + t], big_status=int(bs[b]))
    return got


def _check_case(name, clips, table, W, dur, sd, thr, got, brute=False):
    """Every frame of every clip of a case against float64 (brute: against the enumeration of every class string), by the 4 x
    yardstick rule; prints the figures before it asserts.  -> (the float64 post and cls_post of the case, concatenated; forced
    frames; frames; the float64 results per clip; the yardsticks)."""
    yard = {k: 0.0 for k in KEYS}
    refs, n_forced = [], 0
    W64 = np.asarray(W, np.float64)
    for z, g in zip(clips, got):
        assert g["status"] == 0 and g["vstatus"] == 0, (name, g["status"], g["vstatus"])
        assert len(g["post"]) == len(g["cls_post"]) == len(z)
        lse, forced = SD.forced_frames(z, thr)
        n_forced += int(forced.sum())
        assert P1.path_is_legal(g["ids"], table, forced), "the search's path is not a path of the grammar"
        assert RB.forbidden_successions(g["ids"], table, W64) == 0 and R.forbidden_durations(g["ids"], table, dur, sd) == 0
        if brute:
            r64 = dict(zip(KEYS, DP.brute_force(z, table, W64, dur, sd, forced, g["ids"])))
        else:
            r64 = dict(zip(KEYS, DP.forward_backward(z, table, W64, dur, sd, forced, g["ids"])))
        r32 = dict(zip(KEYS, DP.forward_backward(z, table, W64, dur, sd, forced, g["ids"], dtype=np.float32)))
        for k in KEYS:
            ref = np.atleast_1d(np.asarray(r64[k], np.float64))
            if ref.size:
                yard[k] = max(yard[k], float(np.abs(np.atleast_1d(r32[k]) - ref).max()))
        r64["forced"] = forced
        refs.append(r64)
    dev = {k: 0.0 for k in KEYS}
    over = {k: 0.0 for k in KEYS}
    used_ulp = {k: False for k in KEYS}
    for z, g, r64 in zip(clips, got, refs):
        if not len(z):
            assert g["logz"][0] == 0
            continue
        assert np.isfinite(g["logz"]).all() and np.isfinite(g["post"]).all() and np.isfinite(g["cls_post"]).all()
        assert (g["cls_post"] >= 0).all() and (g["cls_post"] <= g["post"]).all() and (g["post"] <= 1).all()
        for k in KEYS:
            ref = np.atleast_1d(np.asarray(r64[k], np.float64))
            d = _deviation(g[k], ref)
            used_ulp[k] |= bool((yard[k] < _half_ulp(ref)).any())
            dev[k] = max(dev[k], float(d.max()))
            over[k] = max(over[k], float((d - _allowed(yard[k], ref)).max()))
        # logZ sums over every legal path, the search's among them
        tol = float(_allowed(yard["logz"], r64["logz"]))
        assert float(g["logz"][0]) >= R.objective(g["ids"], z, table, W64, dur, sd, r64["forced"]) - tol
    for k in KEYS:
        print(f"{name} thr {thr}: {k}: kernel {dev[k]:.3e}, float32 restatement {yard[k]:.3e}, allowed 4 x = {4 * yard[k]:.3e}"
              f"{' (+ half an fp32 ulp where that exceeds the restatement)' if used_ulp[k] else ''}, over by {max(over[k], 0.0):.3e}")
    n = sum(len(z) for z in clips)
    print(f"{name}: {n_forced} of {n} frames forced")
    for k in KEYS:
        assert over[k] <= 0, (name, k, dev[k], yard[k], over[k])
    vals = np.concatenate([r[k] for r in refs for k in ("post", "cls_post")])
    return vals, n_forced, n, refs, yard


@pytest.mark.parametrize("P,D", CASES)
@pytest.mark.parametrize("k", [0, 1])
def test_ragged_batch_against_float64(P, D, k):
    C, table, clips = SD.make_clips(P, CLIP_SEEDS_K.get((P, D, k), CLIP_SEEDS.get((P, D), SD.SEEDS[P])))
    W, dur, sd, thr = case_tables(P, D, k)
    got = _run(clips, table, W, dur, sd, thr, C, scattered=True)
    assert len(got[LENGTHS.index(0)]["post"]) == 0 and got[LENGTHS.index(0)]["status"] == 0
    post, n_forced, n, _, _ = _check_case(f"P{P} D{D} forbid {CONFIGS[k][0]}", clips, table, W, dur, sd, thr, got)
    assert post.min() < 0.2 and post.max() > 0.99 and ((post > 0.3) & (post < 0.7)).any(), "the posteriors do not span [0, 1] (test setup)"
    if thr > 0:
        assert 0 < n_forced < n, "the threshold does not force some but not all frames (test setup)"


@pytest.mark.parametrize("D", [1, 2, 3])
def test_tiny_clips_against_brute_force(D):
    """100 clips of 1 .. 6 frames in one call against the enumeration of every class string: the off-by-one cases of the ring and the
    tail in both sweeps.  (tests/test_gpu_decode_duration.py's inputs: no frame inside MARGIN.)"""
    rng = np.random.default_rng(7300 + D)
    clips = [(rng.standard_normal((int(rng.integers(1, 7)), SD.TINY_C)) * 2).astype(np.float32) for _ in range(100)]
    W = (-3.0 * rng.random((4, 4))).astype(np.float32)
    mask = rng.random((4, 4)) < 0.2
    mask[:, 0] = False
    W[mask] = -np.inf
    dur, sd = SD.make_dur(3, D, rng, forbid=0.25)
    got = _run(clips, SD.TINY, W, dur, sd, SD.THRESHOLD, SD.TINY_C)
    _check_case(f"tiny D{D}", clips, SD.TINY, W, dur, sd, SD.THRESHOLD, got, brute=True)


@pytest.mark.parametrize("prior", ["none", "zero"])
def test_without_a_prior_it_is_wfl_decode_bigram_posterior(prior):
    """Every sym_dur = -1, and an all-zero table, on the bigram search's path: each entry within its own allowance of float64 (one
    reference: the two restatements agree to 1e-10, tests/test_decode_duration_posterior_cpu.py), and the two within the sum."""
    for P, D in ((2, 1), (70, 8), (70, 32)):
        C, table = SD.make_table(P)
        rng = np.random.default_rng(40 + P + D)
        clips = [R.plant(T, C, table, rng, margin=4.0, scale=2.0)[0] for T in (33, 300)]
        W = SD.make_trans(P, rng)
        dur = np.zeros((3, D + 1), np.float32)
        sd = np.full(P, -1, np.int32) if prior == "none" else rng.integers(0, 3, size=P).astype(np.int32)
        got = _run(clips, table, W, dur, sd, 0.0, C, bigram=True)
        _, _, _, refs, yard = _check_case(f"{prior} P{P} D{D}", clips, table, W, dur, sd, 0.0, got)
        big_yard = {k: 0.0 for k in KEYS}
        for z, g, r64 in zip(clips, got, refs):
            r32 = dict(zip(KEYS, BP.forward_backward(z, table, np.asarray(W, np.float64), r64["forced"], g["ids"], dtype=np.float32)))
            for k in KEYS:
                big_yard[k] = max(big_yard[k], float(np.abs(np.atleast_1d(r32[k]) - np.atleast_1d(r64[k])).max()))
        for z, g, r64 in zip(clips, got, refs):
            assert g["big_status"] == 0
            for k in KEYS:
                ref = np.atleast_1d(np.asarray(r64[k], np.float64))
                a_big, a_dur = _allowed(big_yard[k], ref), _allowed(yard[k], ref)
                d_big = _deviation(g["big_" + k], ref)
                d_both = np.abs(g["big_" + k].astype(np.float64) - g[k].astype(np.float64))
                d_both[ref < 1e-30] = 0.0
                print(f"{prior} P{P} D{D} T {len(z)}: {k}: bigram kernel {d_big.max():.3e} (allowed {a_big.max():.3e}), between the two "
                      f"{d_both.max():.3e} (allowed {(a_big + a_dur).max():.3e})")
                assert (d_big <= a_big).all(), k
                assert (d_both <= a_big + a_dur).all(), k


def _plant_stretches(T, C, table, rng, run, margin=50.0):
    """Long O stretches (20 .. 40 frames) between phoneme runs of run[0] .. run[1] frames, planted by `margin`; the clip begins and
    ends in such a stretch."""
    o, pairs = table
    z = rng.standard_normal((T, C))
    ids = np.full(T, o, np.int32)
    t = int(rng.integers(20, 41))
    while True:
        b, i = pairs[int(rng.integers(len(pairs)))]
        n = int(rng.integers(run[0], run[1] + 1))
        if t + n + 20 > T:
            break
        ids[t:t + 1] = b
        ids[t + 1:t + n] = i
        t += n + int(rng.integers(20, 41))
    z[np.arange(T), ids] += margin
    return z.astype(np.float32), ids


@pytest.mark.parametrize("kind", ["minimum", "maximum"])
def test_a_hard_limit_with_confident_frames_stays_finite(kind):
    """L(1 .. D - 1) = -inf for every phoneme (a run has at least D = 8 frames), and L(4 .. D) = tail = -inf (at most 3), on clips with
    long O stretches planted at margin 50 between the runs.  Under the minimum a run's history entries do not show in end[] for seven
    frames while O sits on its floor of 2^-60 per frame: a scale taken from end[] alone lets them overflow.  Every phoneme has an I
    class here and every planted run is one the table allows, so the row maximum always belongs to a class that carries mass."""
    P, D = 20, 8
    C, table = 2 * P + 4, (1, [(2 + 2 * p, 3 + 2 * p) for p in range(P)])
    rng = np.random.default_rng(71 if kind == "minimum" else 72)
    run = (D, 2 * D) if kind == "minimum" else (1, 3)
    clips = [_plant_stretches(T, C, table, rng, run)[0] for T in (400, 150, 61)]
    W = SD.make_trans(P, rng)
    dur = (-2.0 * rng.random((P, D + 1))).astype(np.float32)
    if kind == "minimum":
        dur[:, :D - 1] = -np.inf
    else:
        dur[:, 3:] = -np.inf
    sd = np.arange(P, dtype=np.int32)
    got = _run(clips, table, W, dur, sd, 0.0, C)
    _check_case(f"hard {kind}", clips, table, W, dur, sd, 0.0, got)
    runs = [k for g in got for _, _, k in R.run_lengths(g["ids"], table)]
    assert runs and (min(runs) >= D if kind == "minimum" else max(runs) <= 3)


def test_one_6000_frame_clip():
    P, D = 70, 32
    C, table, clips = SD.make_clips(P, 11077, lengths=[6000])
    rng = np.random.default_rng(78)
    W = SD.make_trans(P, rng, 0.3)
    dur, sd = SD.make_dur(P, D, rng)
    _check_case("T6000", clips, table, W, dur, sd, SD.THRESHOLD, _run(clips, table, W, dur, sd, SD.THRESHOLD, C))


def test_a_clip_alone_equals_the_clip_in_a_batch_of_16():
    P, D = 70, 8
    C, table = SD.make_table(P)
    rng = np.random.default_rng(3)
    W = SD.make_trans(P, rng, 0.3)
    dur, sd = SD.make_dur(P, D, rng)
    clips = [(rng.standard_normal((int(rng.integers(1, 200)), C)) * 3).astype(np.float32) for _ in range(16)]
    batch = _run(clips, table, W, dur, sd, 0.0, C)
    _check_case("batch_of_16", clips, table, W, dur, sd, 0.0, batch)
    for b in (0, 5, 15):
        alone = _run([clips[b]], table, W, dur, sd, 0.0, C)[0]
        assert (alone["ids"] == batch[b]["ids"]).all() and alone["status"] == batch[b]["status"] == 0
        for k in KEYS:
            assert alone[k].tobytes() == batch[b][k].tobytes(), k


def test_scattered_rows_and_padded_columns_are_not_touched():
    """Clips 13 rows apart in a buffer with 19 more columns, filler 1e30: the results are those of the clips back to back, bit for
    bit, and no row of post / cls_post outside a clip is written."""
    P, D = 65, 8
    C, table, clips = SD.make_clips(P, SD.SEEDS[P])
    W, dur, sd, thr = case_tables(P, D, 1)
    dense = _run(clips, table, W, dur, sd, thr, C)
    scat = _run(clips, table, W, dur, sd, thr, C, scattered=True)
    for a, b in zip(dense, scat):
        assert (a["ids"] == b["ids"]).all() and a["status"] == b["status"] == 0
        for k in KEYS:
            assert a[k].tobytes() == b[k].tobytes(), k
    T = [len(c) for c in clips]
    offs, host = _layout(clips, C, True)
    lg = torch.from_numpy(host).cuda()[:, :C]
    ids = DC.bio_viterbi_duration(lg, T, table, W, dur, sd, thr, frame_offsets=offs)[0]
    clips_ = DC._check_clips(lg, T, table, 0.0, thr, offs)
    per_frame = torch.full((2, lg.shape[0]), -7.0, device="cuda")
    logz = torch.empty(len(T), device="cuda")
    st = torch.empty(len(T), dtype=torch.int32, device="cuda")
    DC._call("wfl_decode_duration_posterior", lg, clips_, (W, sd, dur, len(dur), D, float(thr), ids), (logz, per_frame[0], per_frame[1], st),
             None, ws_more=(D,))
    torch.cuda.synchronize()
    inside = np.zeros(lg.shape[0], bool)
    for o, t in zip(offs, T):
        inside[o:o + t] = True
    pf = per_frame.cpu().numpy()
    assert (pf[:, ~inside] == -7.0).all() and (pf[:, inside] >= 0).all() and st.cpu().tolist() == [0] * len(T)


def test_ids_that_are_no_path_are_status_8_for_that_clip_only():
    """Hand-edited paths are refused, not scored: wfl_decode_bigram_posterior's cases, and a run whose length has L = -inf, in mid-clip
    and as the clip's last run.  The neighbours in the batch are bit for bit what they were."""
    P, D = 20, 4
    C, table = 2 * P + 4, (1, [(2 + 2 * p, 3 + 2 * p) for p in range(P)])        # O = 1, B-p = 2 + 2p, I-p = 3 + 2p
    rng = np.random.default_rng(5)
    W = SD.make_trans(P, np.random.default_rng(6), 0.3)
    dur = (-2.0 * rng.random((P, D + 1))).astype(np.float32)
    dur[:, 1] = -np.inf                                         # no run of exactly two frames
    sd = np.arange(P, dtype=np.int32)
    clips = [_plant_stretches(150, C, table, rng, (3, 6), margin=12.0)[0] for _ in range(6)]
    clips.append((rng.standard_normal((90, C)) * 3).astype(np.float32))
    thr = SD.THRESHOLD
    base = _run(clips, table, W, dur, sd, thr, C)
    assert [g["status"] for g in base] == [0] * 7
    forced6 = R.prepass(clips[6], thr)[1]
    assert forced6.any() and float(np.abs(R.prepass(clips[6], thr)[2] - thr).min()) > MARGIN
    assert not any(R.prepass(clips[b], thr)[1].any() for b in range(6))
    shut = int(np.nonzero(np.isneginf(W[0, 1:]))[0][0])
    for g in base[:6]:                                          # the planted clips begin and end in a long O stretch
        assert (g["ids"][:5] == 1).all() and (g["ids"][-5:] == 1).all()

    def edit(ids, offs):
        h = ids.cpu().numpy()
        h[offs[0] + 2] = 3                                      # clip 0: I-0 after O
        h[offs[1] + 2], h[offs[1] + 3] = 2, 5                   # clip 1: I-1 after B-0
        h[offs[2] + 2] = 2 + 2 * shut                           # clip 2: O, B-q, O through a -inf succession
        h[offs[2] + 3:offs[2] + 5] = 3 + 2 * shut               # (three frames: the length is allowed)
        h[offs[3] + 2], h[offs[3] + 3] = 2, 3                   # clip 3: a run of two frames in mid-clip
        h[offs[4] + 148], h[offs[4] + 149] = 2, 3               # clip 4: a run of two frames as the clip's last run
        h[offs[6] + int(np.nonzero(forced6)[0][0])] = 2         # clip 6: B-0 on a forced frame
        return torch.from_numpy(h).cuda()
    assert np.isfinite(W[0, 1]) or shut == 0, "W[O][0] must be finite for the run-length edits (test setup)"
    got = _run(clips, table, W, dur, sd, thr, C, ids_edit=edit)
    assert [g["status"] for g in got] == [8, 8, 8, 8, 8, 0, 8]
    for b in (0, 1, 2, 3, 4, 6):
        assert got[b]["logz"][0] == 0 and not got[b]["post"].any() and not got[b]["cls_post"].any()
    for k in KEYS:
        assert got[5][k].tobytes() == base[5][k].tobytes(), k


def test_symbol_cap_is_status_2_and_the_neighbours_are_untouched():
    rng = np.random.default_rng(31)
    C, big = SD.make_table(192)
    _, table = SD.make_table(70)
    W, Wbig = SD.make_trans(70, rng), SD.make_trans(192, rng)
    dur, sd = SD.make_dur(70, 8, rng)
    dbig, sbig = SD.make_dur(192, 8, rng)
    T = [200, 150, 90]
    lg = torch.from_numpy(rng.standard_normal((sum(T), C)).astype(np.float32) * 3).cuda()
    ids = DC.bio_viterbi_duration(lg, T, table, W, dur, sd, 0.0)[0]
    whole = DC.decode_posteriors_duration(lg, T, table, W, dur, sd, 0.0, ids)
    assert whole[3].cpu().tolist() == [0, 0, 0]
    nb = lambda: DC.decode_posteriors_duration(lg, [T[0], T[2]], table, W, dur, sd, 0.0, ids, frame_offsets=[0, T[0] + T[1]])   # noqa: E731
    before = nb()
    logz, post, cls, st = DC.decode_posteriors_duration(lg, [T[1]], big, Wbig, dbig, sbig, 0.0, ids, frame_offsets=[T[0]])
    after = nb()
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [DC.STATUS_OVER_CAP] and logz.cpu().tolist() == [0.0]
    mid = slice(T[0], T[0] + T[1])
    assert not post[mid].cpu().numpy().any() and not cls[mid].cpu().numpy().any()
    assert DC.duration_posterior_workspace_bytes([T[1]], 192, 8) == 0 and DC.duration_posterior_workspace_bytes([T[1]], 191, 8) > 0
    for got in (before, after):
        assert got[3].cpu().tolist() == [0, 0]
        assert got[0].cpu().numpy().tobytes() == whole[0][[0, 2]].cpu().numpy().tobytes()
        for a in (slice(0, T[0]), slice(T[0] + T[1], sum(T))):
            assert torch.equal(got[1][a], whole[1][a]) and torch.equal(got[2][a], whole[2][a])
    # 191 phonemes are inside the cap at the largest D
    _, t191 = SD.make_table(191)
    d191, s191 = SD.make_dur(191, 32, rng)
    W191 = SD.make_trans(191, rng)
    i191 = DC.bio_viterbi_duration(lg, [T[0]], t191, W191, d191, s191, 0.0)[0]
    assert DC.decode_posteriors_duration(lg, [T[0]], t191, W191, d191, s191, 0.0, i191)[3].cpu().tolist() == [0]


def _raw(lg, T, table, W, dur, sd, thr, ids):
    """The ABI entry without the Python entry's checks of dur and sym_dur (for the statuses those checks would pre-empt)."""
    clips = DC._check_clips(lg, T, table, 0.0, thr, None)
    dur = np.ascontiguousarray(dur, np.float32)
    D = dur.shape[1] - 1
    return DC._posteriors("wfl_decode_duration_posterior", lg, clips, (np.ascontiguousarray(W, np.float32), np.ascontiguousarray(sd, np.int32),
                                                                      dur, len(dur), D, float(thr)), ids, None, ws_more=(D,))


def test_a_bad_class_table_or_row_is_status_4():
    rng = np.random.default_rng(9)
    C = 141
    z = rng.standard_normal((20, C)).astype(np.float32)
    lg = torch.from_numpy(np.concatenate([z, z])).cuda()
    ids = torch.zeros(40, dtype=torch.int32, device="cuda")
    for pairs in ([(1, 2), (C + 3, 4)], [(1, 2), (3, C)], [(1, 2), (3, -2)], [(1, 2), (3, 2)], [(1, 2), (0, 4)],
                  [(p + 1, -1) for p in range(C - 1)] + [(5, -1)]):
        P = len(pairs)
        dur, sd = SD.make_dur(P, 4, rng)
        logz, post, cls, st = DC.decode_posteriors_duration(lg, [20, 20], (0, pairs), SD.make_trans(P, rng), dur, sd, 0.0, ids)
        assert st.cpu().tolist() == [DC.STATUS_BAD_CLASS] * 2 and logz.cpu().tolist() == [0.0, 0.0], pairs[:3]
        assert not post.cpu().numpy().any() and not cls.cpu().numpy().any()
    table, W = (0, [(1, 2), (3, 4)]), SD.make_trans(2, rng)
    dur = np.zeros((3, 5), np.float32)
    for sd in ([0, -2], [3, 0]):                 # below -1; n_rows
        logz, post, cls, st = _raw(lg, [20, 20], table, W, dur, sd, 0.0, ids)
        assert st.cpu().tolist() == [DC.STATUS_BAD_CLASS] * 2 and logz.cpu().tolist() == [0.0, 0.0], sd
        assert not post.cpu().numpy().any() and not cls.cpu().numpy().any()
    for sd in ([2, -1], [0, 0]):                 # (all-O is a path of every table)
        assert _raw(lg, [20, 20], table, W, dur, sd, 0.0, ids)[3].cpu().tolist() == [0, 0]


def test_empty_batch_empty_clip_and_a_table_without_phonemes():
    P, D = 65, 8
    C, table = SD.make_table(P)
    rng = np.random.default_rng(2)
    W = SD.make_trans(P, rng, 0.3)
    dur, sd = SD.make_dur(P, D, rng)
    z = (rng.standard_normal((30, C)) * 3).astype(np.float32)
    clips = [z[:10], z[:0], z[10:]]
    got = _run(clips, table, W, dur, sd, 0.0, C)
    _check_case("with_an_empty_clip", clips, table, W, dur, sd, 0.0, got)
    assert got[1]["status"] == 0 and got[1]["logz"][0] == 0 and len(got[1]["post"]) == 0
    assert _run([], table, W, dur, sd, 0.0, C) == []
    lg = torch.zeros((0, C), device="cuda")
    logz, post, cls, st = DC.decode_posteriors_duration(lg, [0], table, W, dur, sd, 0.0, torch.zeros(0, dtype=torch.int32, device="cuda"))
    assert st.cpu().tolist() == [0] and logz.cpu().tolist() == [0.0] and post.numel() == 0 and cls.numel() == 0
    # a table with no phoneme: O everywhere, one path, every posterior 1; also without any row of dur
    for d in (dur, np.zeros((0, 4), np.float32)):
        none = (1, [])
        got = _run([z], none, np.zeros((1, 1), np.float32), d, np.zeros(0, np.int32), 0.0, C)
        # (the one path's posterior is 1 and logz the sum of O's logits: both within the rule, _check_case; fp32 products of the two
        # sweeps do not round to exactly 1 on every frame, and nothing is above it)
        _, _, _, refs, _ = _check_case("no phonemes", [z], none, np.zeros((1, 1), np.float32), np.zeros((1, d.shape[1]), np.float32),
                                       np.zeros(0, np.int32), 0.0, got)
        assert got[0]["status"] == 0 and np.abs(refs[0]["post"] - 1).max() <= 1e-12 and np.abs(refs[0]["cls_post"] - 1).max() <= 1e-12
        assert abs(refs[0]["logz"] - float(z[:, 1].astype(np.float64).sum())) <= 1e-9
        assert (got[0]["post"] <= 1).all() and (got[0]["post"] == got[0]["cls_post"]).all()


def test_a_workspace_one_byte_too_small_is_refused():
    P, D = 7, 4
    C, table = SD.make_table(P)
    rng = np.random.default_rng(4)
    W = SD.make_trans(P, rng)
    dur, sd = SD.make_dur(P, D, rng)
    lg = torch.from_numpy(rng.standard_normal((50, C)).astype(np.float32)).cuda()
    ids = DC.bio_viterbi_duration(lg, [50], table, W, dur, sd, 0.0)[0]
    from wfl_asr_amd import _lib
    lib = _lib.load()
    need = DC.duration_posterior_workspace_bytes([50], P, D)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    d_pairs, d_w, d_sd, d_dur = dev(np.asarray(table[1], np.int32)), dev(W), dev(sd), dev(dur)
    logz, st = torch.empty(1, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    post, cls = torch.empty(50, device="cuda"), torch.empty(50, device="cuda")
    T, F0 = np.array([50], np.int32), np.array([0], np.int64)
    hp, p = _lib.host_ptr, _lib.ptr

    def call(n_bytes):
        return lib.wfl_decode_duration_posterior(p(lg), C, C, table[0], hp(F0), hp(T), 1, p(d_pairs), P, p(d_w), p(d_sd), p(d_dur), len(dur), D,
                                                 0.0, p(ids), p(ws), n_bytes, p(logz), p(post), p(cls), p(st), None)
    assert call(need - 1) < 0 and b"workspace too small" in lib.wfl_last_error()
    assert call(need) == 0
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0]


def test_argument_checks_of_the_python_entry():
    P = 3
    C, table = SD.make_table(P)
    lg = torch.zeros((10, C), device="cuda")
    ids = torch.ones(10, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(0)
    W = SD.make_trans(P, rng)
    dur = (-rng.random((2, 5))).astype(np.float32)
    sd = np.array([0, -1, 1], np.int32)
    call = lambda **kw: DC.decode_posteriors_duration(kw.get("lg", lg), kw.get("T", [10]), table, kw.get("W", W), kw.get("dur", dur),  # noqa: E731
                                                      kw.get("sd", sd), kw.get("thr", 0.0), kw.get("ids", ids))
    assert call()[3].cpu().tolist() == [0]
    with pytest.raises(ValueError, match="float32 CUDA"):
        call(lg=lg.cpu())
    with pytest.raises(ValueError, match="past the logits"):
        call(T=[11])
    with pytest.raises(ValueError, match="threshold"):
        call(thr=-0.5)
    for bad, what in ((np.nan, "dur holds a NaN"), (np.inf, r"dur holds \+inf")):
        d = dur.copy()
        d[1, 2] = bad
        with pytest.raises(ValueError, match=what):
            call(dur=d)
    d = dur.copy()
    d[0, 4] = 0.5
    with pytest.raises(ValueError, match="tail of dur"):
        call(dur=d)
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
    with pytest.raises(ValueError, match=r"\[4, 4\]"):
        call(W=W[:-1])
    for bad in (ids.cpu(), ids.long(), ids[:9], ids.view(5, 2), ids.cpu().numpy()):
        with pytest.raises(ValueError, match="ids must be"):
            call(ids=bad)
