"""-m gpu: wfl_decode_bigram (csrc/decode_bigram.hip) against the float64 numpy recurrence of tests/bio_bigram_ref.py on seeded logits
and seeded transition tables, ragged batches.

Criterion and bounds are those of tests/test_gpu_decode.py (the arithmetic is the same: fp32 sums of logits and weights, renormalised
every 16 frames, the offset carried in a double): the kernel's path is legal, every forced frame is O, no opened run takes a -inf
entry, the float64 objective of the kernel's path is >= the reference optimum - 1e-3, and |score - reference score| <= 1e-3 T.
The largest measured figures belong here; they have not been recorded yet.  The bounds were fixed before any run and stay as they are.

Forced frames: the MARGIN = 1e-4 rule of tests/test_gpu_decode.py.  The seeds are chosen so that NO frame of any input is inside that
margin (asserted), so every frame the float64 pre-pass forces must be O, none is excused.

"""
import numpy as np
import pytest
import torch

import bio_bigram_ref as R
from wfl_asr_amd import decode as DC

pytestmark = pytest.mark.gpu
MARGIN = 1e-4
LENGTHS = [1, 2, 15, 16, 17, 0, 31, 32, 33, 300]
PHONEMES = [1, 2, 63, 64, 65, 70, 191]


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


SEEDS = {1: 101, 2: 102, 63: 163, 64: 164, 65: 165, 70: 170, 191: 1291}      # chosen on the CPU: no frame inside MARGIN at 0.5
THRESHOLD = 0.5


def _run(clips, table, W, thr, C):
    """clips: list of z [T, C] float32 -> numpy (ids, score, status) per clip."""
    z = np.concatenate(clips) if clips else np.zeros((0, C), np.float32)
    lg = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    T = [len(c) for c in clips]
    ids, score, status = DC.bio_viterbi_bigram(lg, T, table, W, thr)
    torch.cuda.synchronize()
    ids, score, status = ids.cpu().numpy(), score.cpu().numpy(), status.cpu().numpy()
    out, pos = [], 0
    for b, t in enumerate(T):
        out.append((ids[pos:pos + t], float(score[b]), int(status[b])))
        pos += t
    return out


def forced_frames(z, thr):
    """The float64 pre-pass; asserts that no frame is inside MARGIN of the threshold and that fp32 would agree."""
    lse, forced, pmax = R.prepass(z, thr)
    if thr > 0 and len(z):
        _, f32, p32 = R.prepass(z, thr, np.float32)
        dev = float(np.abs(p32.astype(np.float64) - pmax).max())
        gap = float(np.abs(pmax - thr).min())
        print(f"forced frames: {int(forced.sum())} of {len(z)}; min |p - thr| {gap:.3e}; max |p32 - p64| {dev:.3e}")
        assert dev <= MARGIN / 4, dev
        assert gap > MARGIN, "a frame of the test input is inside the margin of the threshold: choose another seed"
        assert (f32 == forced).all()
    return lse, forced


def _check(z, table, W, thr, got, planted=None):
    ids, score, status = got
    T = len(z)
    assert status == 0
    assert len(ids) == T
    if T == 0:
        assert score == 0.0
        return
    lse, forced = forced_frames(z, thr)
    ref, ref_obj = R.viterbi(z, table, W, forced)
    assert R.legal(ids, table), "the kernel's path is not a legal path"
    assert (ids[forced] == table[0]).all(), "a forced frame is not O"
    assert R.forbidden_successions(ids, table, W) == 0, "the kernel's path takes a forbidden succession"
    mine = R.objective(ids, z, table, W, forced)
    ref_score = ref_obj - float(lse.sum())
    print(f"T {T} P {len(table[1])} thr {thr}: objective {mine:.6f} ref {ref_obj:.6f} (gap {ref_obj - mine:.3e}); "
          f"score {score:.4f} ref {ref_score:.4f} (diff {abs(score - ref_score):.3e})")
    assert abs(R.objective(ref, z, table, W, forced) - ref_obj) <= 1e-9 * max(1.0, abs(ref_obj)), "the reference's own path (test setup)"
    assert mine >= ref_obj - 1e-3, (mine, ref_obj)
    assert abs(score - ref_score) <= 1e-3 * T, (score, ref_score)
    if planted is not None:
        assert (ref == planted).all(), "the planted path is not the reference's optimum (test setup)"
        assert (ids == planted).all()


@pytest.mark.parametrize("P", PHONEMES)
def test_ragged_batch_against_float64_recurrence(P):
    C, table, clips = make_clips(P, SEEDS[P])
    rng = np.random.default_rng(1000 + P)
    for forbid, thr in ((0.0, 0.0), (0.3, THRESHOLD)):
        W = make_trans(P, rng, forbid)
        got = _run(clips, table, W, thr, C)
        assert len(got[LENGTHS.index(0)][0]) == 0
        for z, g in zip(clips, got):
            _check(z, table, W, thr, g)


@pytest.mark.parametrize("forbid", [0.0, 0.3])
def test_one_6000_frame_clip(forbid):
    P = 70
    C, table, clips = make_clips(P, 11077, lengths=[6000])
    W = make_trans(P, np.random.default_rng(78), forbid)
    got = _run(clips, table, W, THRESHOLD, C)
    _check(clips[0], table, W, THRESHOLD, got[0])


@pytest.mark.parametrize("P", [2, 65, 191])
def test_a_planted_path_whose_successions_are_the_only_cheap_ones_is_recovered(P):
    """A planted margin of 1 per frame, and a table in which the planted path's successions cost 0.5 nats and every other one 30 (more
    than a whole planted run is worth, so a table read transposed or shifted would merge runs): the reference's optimum is the planted
    path, and so is the kernel's."""
    C, table = make_table(P)
    rng = np.random.default_rng(500 + P)
    sym, kind = R._symbols(table)
    clips, plants = [], []
    W = np.full((P + 1, P + 1), -30.0, np.float32)
    for T in (40, 300):
        z, ids = R.plant(T, C, table, rng, margin=1.0, scale=0.05)
        prev = 0
        for c in ids:
            if kind[int(c)] == 1 or (kind[int(c)] == 0 and prev != 0):
                W[prev, sym[int(c)]] = -0.5
            prev = sym[int(c)]
        clips.append(z)
        plants.append(ids)
    got = _run(clips, table, W, 0.0, C)
    for z, pl, g in zip(clips, plants, got):
        _check(z, table, W, 0.0, g, pl)


@pytest.mark.parametrize("lam", [0.0, 2.0])
def test_a_flat_table_is_wfl_decode(lam):
    """W = -lambda everywhere: the objective is wfl_decode's.  Planted inputs (no ties): the same ids; both scores are within the
    bound of the float64 reference, so within twice the bound of each other."""
    for P in (2, 70):
        C, table = make_table(P)
        rng = np.random.default_rng(40 + P)
        clips = [R.plant(T, C, table, rng)[0] for T in (33, 300)]
        W = np.full((P + 1, P + 1), -lam, np.float32)
        got = _run(clips, table, W, 0.0, C)
        lg = torch.from_numpy(np.concatenate(clips)).cuda()
        ids, score, st = DC.bio_viterbi(lg, [len(c) for c in clips], table, lam, 0.0)
        assert st.cpu().tolist() == [0, 0]
        ids, score, pos = ids.cpu().numpy(), score.cpu().numpy(), 0
        for b, z in enumerate(clips):
            _check(z, table, W, 0.0, got[b])
            assert (got[b][0] == ids[pos:pos + len(z)]).all()
            assert abs(got[b][1] - float(score[b])) <= 2e-3 * len(z)
            pos += len(z)


def test_symbol_cap_is_reported_and_the_neighbours_are_untouched():
    """The number of phonemes is an argument of the call, so a clip over the cap cannot share a call with feasible ones; they share the
    logits buffer instead.  Three clips lie back to back in one buffer.  The middle one decoded with 192 phonemes is status 2, all O,
    score 0; its neighbours, decoded with 70 phonemes before and after that call, are bit for bit what they are when all three clips
    are decoded with 70 phonemes."""
    assert DC.MAX_BIGRAM_SYMBOLS == 192
    rng = np.random.default_rng(31)
    C, big = make_table(192)
    _, table = make_table(70)
    W = make_trans(70, rng)
    Wbig = make_trans(192, rng)
    T = [200, 150, 90]
    lg = torch.from_numpy(rng.standard_normal((sum(T), C)).astype(np.float32) * 3).cuda()
    all_ids, all_score, all_st = DC.bio_viterbi_bigram(lg, T, table, W, 0.0)
    assert all_st.cpu().tolist() == [0, 0, 0]
    nb = lambda: DC.bio_viterbi_bigram(lg, [T[0], T[2]], table, W, 0.0, frame_offsets=[0, T[0] + T[1]])   # noqa: E731
    before = nb()
    ids, score, st = DC.bio_viterbi_bigram(lg, [T[1]], big, Wbig, 0.0, frame_offsets=[T[0]])
    after = nb()
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [DC.STATUS_OVER_CAP] and score.cpu().tolist() == [0.0]
    assert (ids[T[0]:T[0] + T[1]].cpu().numpy() == big[0]).all()
    for got in (before, after):
        assert got[2].cpu().tolist() == [0, 0]
        for a in (slice(0, T[0]), slice(T[0] + T[1], sum(T))):
            assert torch.equal(got[0][a], all_ids[a])
        assert got[1].cpu().numpy().tobytes() == all_score[[0, 2]].cpu().numpy().tobytes()
    # 191 phonemes are inside the cap
    _, t191 = make_table(191)
    st = DC.bio_viterbi_bigram(lg, [T[0]], t191, make_trans(191, rng), 0.0)[2]
    assert st.cpu().tolist() == [0]


def test_a_bad_class_table_is_status_4():
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
        W = make_trans(len(pairs), rng)
        ids, score, status = DC.bio_viterbi_bigram(lg, [20, 20], (0, pairs), W, 0.0)
        assert status.cpu().tolist() == [DC.STATUS_BAD_CLASS] * 2, pairs[:3]
        assert (ids.cpu().numpy() == 0).all() and score.cpu().tolist() == [0.0, 0.0]
    ids, score, status = DC.bio_viterbi_bigram(lg, [20, 20], (0, [(1, 2), (3, 4)]), make_trans(2, rng), 0.0)
    assert status.cpu().tolist() == [0, 0]


def test_empty_batch_and_a_table_without_phonemes():
    C, table = make_table(2)
    W = make_trans(2, np.random.default_rng(1))
    assert _run([], table, W, 0.0, C) == []
    ids, score, status = DC.bio_viterbi_bigram(torch.zeros((0, C), device="cuda"), [0], table, W, 0.0)
    assert status.cpu().tolist() == [0] and ids.numel() == 0 and score.cpu().tolist() == [0.0]
    z = np.random.default_rng(2).standard_normal((30, C)).astype(np.float32)
    got = _run([z], (1, []), np.zeros((1, 1), np.float32), 0.0, C)      # no phoneme: O everywhere
    assert got[0][2] == 0 and (got[0][0] == 1).all()


def test_a_clip_alone_equals_the_clip_in_a_batch_of_16():
    P = 70
    C, table = make_table(P)
    rng = np.random.default_rng(3)
    W = make_trans(P, rng, 0.3)
    clips = [rng.standard_normal((int(rng.integers(1, 400)), C)).astype(np.float32) * 3 for _ in range(16)]
    batch = _run(clips, table, W, 0.0, C)
    for b in (0, 5, 15):
        alone = _run([clips[b]], table, W, 0.0, C)[0]
        assert (alone[0] == batch[b][0]).all()
        assert np.float32(alone[1]).tobytes() == np.float32(batch[b][1]).tobytes() and alone[2] == batch[b][2] == 0


def test_argument_checks_of_the_python_entry():
    P = 3
    C, table = make_table(P)
    lg = torch.zeros((10, C), device="cuda")
    W = make_trans(P, np.random.default_rng(0))
    for bad, what in ((np.nan, "NaN"), (np.inf, r"\+inf")):
        Wb = W.copy()
        Wb[2, 3] = bad
        with pytest.raises(ValueError, match=what):
            DC.bio_viterbi_bigram(lg, [10], table, Wb, 0.0)
    with pytest.raises(ValueError, match="table"):
        DC.bio_viterbi_bigram(lg, [10], table, W[:3, :3], 0.0)
    with pytest.raises(ValueError, match="float32"):
        DC.bio_viterbi_bigram(lg, [10], table, W.astype(np.float64), 0.0)
    Wb = W.copy()
    Wb[2, 0] = -np.inf
    with pytest.raises(ValueError, match=r"\[p\]\[O\]"):
        DC.bio_viterbi_bigram(lg, [10], table, Wb, 0.0)
    with pytest.raises(ValueError, match="threshold"):
        DC.bio_viterbi_bigram(lg, [10], table, W, -0.5)
    Wb = W.copy()
    Wb[0, 0] = -np.inf                       # [O][O] is never read: -inf there is fine
    assert DC.bio_viterbi_bigram(lg, [10], table, Wb, 0.0)[2].cpu().tolist() == [0]
