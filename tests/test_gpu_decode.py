"""-m gpu: wfl_decode (csrc/decode.hip) against the float64 numpy recurrence of tests/bio_viterbi_ref.py on seeded logits, ragged
batches.

Bounds (set before the kernel ran, from tests/test_gpu_align.py:69-70, which checks the same arithmetic -- fp32 sums of logits,
renormalised every 16 frames): the float64 objective of the kernel's path is >= the reference optimum - 1e-3, and
|score - reference score| <= 1e-3 T.  Measured on the MI355X, largest figures over every case: objective gap 0 (bound 1e-3);
score difference 4.1e-3 at T = 15 000 (bound 15), 3.3e-4 at T = 1500 (bound 1.5); the float32 numpy restatement of the recurrence
is off by 9.4e-4 / 3.3e-4 on the same inputs.  Both bounds hold as taken over, none was widened.

Forced frames: the kernel's pre-pass computes the largest softmax probability in fp32.  An fp32 sum of C <= 1023 terms in (0, 1] with
a correctly rounded exp carries a relative error of at most about C 2^-24 = 6e-5, so a frame whose float64 probability is within
MARGIN = 1e-4 of the threshold may legitimately fall on either side.  The seeds below are chosen so that NO frame of any input is
inside that margin (asserted, with the float32 numpy restatement's own deviation from float64 asserted to be below MARGIN / 4), so
every frame the float64 pre-pass forces must be O, none is excused.
"""
import numpy as np
import pytest
import torch

import bio_viterbi_ref as R
from wfl_asr_amd import decode as DC

pytestmark = pytest.mark.gpu
MARGIN = 1e-4


def _table(C, n_both, n_b_only=0):
    """O = 0; phoneme p < n_both: (2p + 1, 2p + 2); then n_b_only phonemes with a B class alone; the classes above are never chosen."""
    pairs = [(2 * p + 1, 2 * p + 2) for p in range(n_both)]
    pairs += [(2 * n_both + 1 + q, -1) for q in range(n_b_only)]
    assert max(max(p) for p in pairs) < C
    return (0, pairs)


TABLES = {"C141": (141, _table(141, 70)),                 # 2 slots per lane
          "C401": (401, _table(401, 150, 50)),            # 4 slots, 50 classes never chosen
          "C1023": (1023, _table(1023, 511)),             # 8 slots
          "C1023_b_only": (1023, _table(1023, 423, 176))}  # 16 slots (599 phonemes)


def _run(clips, table, lam, thr, C):
    """clips: list of z [T, C] float32 -> numpy (ids, score, status) per clip."""
    z = np.concatenate(clips) if clips else np.zeros((0, C), np.float32)
    lg = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    T = [len(c) for c in clips]
    ids, score, status = DC.bio_viterbi(lg, T, table, lam, thr)
    torch.cuda.synchronize()
    ids, score, status = ids.cpu().numpy(), score.cpu().numpy(), status.cpu().numpy()
    out, pos = [], 0
    for b, t in enumerate(T):
        out.append((ids[pos:pos + t], float(score[b]), int(status[b])))
        pos += t
    return out


def _forced(z, thr):
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


def _check(z, table, lam, thr, got, planted=None):
    ids, score, status = got
    T = len(z)
    assert status == 0
    assert len(ids) == T
    if T == 0:
        assert score == 0.0
        return
    lse, forced = _forced(z, thr)
    ref, ref_obj = R.viterbi(z, table, lam, forced)
    assert R.legal(ids, table), "the kernel's path is not a legal path"
    assert (ids[forced] == table[0]).all(), "a forced frame is not O"
    mine = R.objective(ids, z, table, lam, forced)
    ref_score = ref_obj - float(lse.sum())
    print(f"T {T} lambda {lam} thr {thr}: objective {mine:.6f} ref {ref_obj:.6f} (gap {ref_obj - mine:.3e}); "
          f"score {score:.4f} ref {ref_score:.4f} (diff {abs(score - ref_score):.3e})")
    assert mine >= ref_obj - 1e-3, (mine, ref_obj)
    assert abs(score - ref_score) <= 1e-3 * T, (score, ref_score)
    if planted is not None:
        assert (ref == planted).all(), "the planted path is not the reference's optimum (test setup)"
        assert (ids == planted).all()


LENGTHS = [1, 2, 17, 64, 333, 700, 1500]


@pytest.mark.parametrize("name", list(TABLES))
@pytest.mark.parametrize("lam", [0.0, 2.0, 4.0])
def test_ragged_batch_against_float64_recurrence(name, lam):
    C, table = TABLES[name]
    rng = np.random.default_rng(20 + C)
    clips, plants = [], []
    for j, T in enumerate(LENGTHS):
        if j % 2 == 0:
            clips.append(rng.standard_normal((T, C)).astype(np.float32) * 3)
            plants.append(None)
        else:
            z, ids = R.plant(T, C, table, rng)
            clips.append(z)
            plants.append(ids)
    for thr in (0.0, 0.5):
        got = _run(clips, table, lam, thr, C)
        for z, pl, g in zip(clips, plants, got):
            _check(z, table, lam, thr, g, pl)


@pytest.mark.parametrize("lam,thr", [(0.0, 0.0), (2.0, 0.5), (4.0, 0.0)])
def test_one_15000_frame_clip(lam, thr):
    C, table = TABLES["C141"]
    rng = np.random.default_rng(8)
    z, ids = R.plant(15000, C, table, rng)
    zr = rng.standard_normal((15000, C)).astype(np.float32) * 3
    got = _run([z, zr], table, lam, thr, C)
    _check(z, table, lam, thr, got[0], ids)
    _check(zr, table, lam, thr, got[1])


def test_class_cap_is_reported_and_the_neighbours_are_untouched():
    """C is an argument of the call, so a clip over the cap cannot share a call with feasible ones; they share the logits buffer
    instead.  Three clips lie back to back in one [rows, 1025] buffer.  The middle one decoded with all 1025 columns is status 2, all
    O, score 0; its neighbours, decoded from the same buffer through the 1023-column view before and after that call, are bit for
    bit what they are when all three clips are decoded through the view."""
    rng = np.random.default_rng(31)
    table = TABLES["C1023"][1]
    T = [200, 150, 90]
    lg = torch.from_numpy(rng.standard_normal((sum(T), 1025)).astype(np.float32) * 3).cuda()
    view = lg[:, :1023]
    all_ids, all_score, all_st = DC.bio_viterbi(view, T, table, 2.0, 0.0)
    assert all_st.cpu().tolist() == [0, 0, 0]
    nb = lambda: DC.bio_viterbi(view, [T[0], T[2]], table, 2.0, 0.0, frame_offsets=[0, T[0] + T[1]])   # noqa: E731
    before = nb()
    ids, score, st = DC.bio_viterbi(lg, [T[1]], table, 2.0, 0.0, frame_offsets=[T[0]])
    after = nb()
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [DC.STATUS_OVER_CAP] and score.cpu().tolist() == [0.0]
    assert (ids[T[0]:T[0] + T[1]].cpu().numpy() == table[0]).all()
    for got in (before, after):
        assert got[2].cpu().tolist() == [0, 0]
        for a, b in ((slice(0, T[0]), slice(0, T[0])), (slice(T[0] + T[1], sum(T)), slice(T[0] + T[1], sum(T)))):
            assert torch.equal(got[0][a], all_ids[b])
        assert got[1].cpu().numpy().tobytes() == all_score[[0, 2]].cpu().numpy().tobytes()
    z = view.cpu().numpy()
    _check(z[:T[0]], table, 2.0, 0.0, (all_ids[:T[0]].cpu().numpy(), float(all_score[0]), 0))


def test_a_bad_class_table_is_status_4():
    rng = np.random.default_rng(9)
    C = 141
    z = rng.standard_normal((20, C)).astype(np.float32)
    lg = torch.from_numpy(np.concatenate([z, z])).cuda()
    good = TABLES["C141"][1]
    for pairs in ([(1, 2), (C + 3, 4)],          # a B class out of range
                  [(1, 2), (3, C)],              # an I class out of range
                  [(1, 2), (3, -2)],             # -1 alone means "no I class"
                  [(1, 2), (3, 2)],              # a class used twice
                  [(1, 2), (0, 4)],              # the O class used as a B class
                  [(p % 100 + 1, -1) for p in range(1100)]):   # more phonemes than classes
        ids, score, status = DC.bio_viterbi(lg, [20, 20], (0, pairs), 1.0, 0.0)
        assert status.cpu().tolist() == [DC.STATUS_BAD_CLASS] * 2, pairs[:3]
        assert (ids.cpu().numpy() == 0).all() and score.cpu().tolist() == [0.0, 0.0]
    ids, score, status = DC.bio_viterbi(lg, [20, 20], good, 1.0, 0.0)
    assert status.cpu().tolist() == [0, 0]


def test_empty_clip_and_empty_batch():
    C, table = TABLES["C141"]
    rng = np.random.default_rng(2)
    z = rng.standard_normal((30, C)).astype(np.float32) * 3
    got = _run([z[:10], z[:0], z[10:]], table, 2.0, 0.0, C)
    _check(z[:10], table, 2.0, 0.0, got[0])
    assert got[1][1:] == (0.0, 0) and len(got[1][0]) == 0
    _check(z[10:], table, 2.0, 0.0, got[2])
    assert _run([], table, 2.0, 0.0, C) == []
    ids, score, status = DC.bio_viterbi(torch.zeros((0, C), device="cuda"), [0], table, 0.0, 0.0)
    assert status.cpu().tolist() == [0] and ids.numel() == 0
    # a table with no phoneme: O everywhere
    got = _run([z], (0, []), 1.0, 0.0, C)
    assert got[0][2] == 0 and (got[0][0] == 0).all()


def test_a_clip_alone_equals_the_clip_in_a_batch_of_16():
    C, table = TABLES["C141"]
    rng = np.random.default_rng(3)
    clips = [rng.standard_normal((int(rng.integers(1, 1500)), C)).astype(np.float32) * 3 for _ in range(16)]
    batch = _run(clips, table, 2.0, 0.5, C)
    for b in (0, 5, 15):
        alone = _run([clips[b]], table, 2.0, 0.5, C)[0]
        assert (alone[0] == batch[b][0]).all()
        assert np.float32(alone[1]).tobytes() == np.float32(batch[b][1]).tobytes() and alone[2] == batch[b][2] == 0


def test_argument_checks_of_the_python_entry():
    C, table = TABLES["C141"]
    lg = torch.zeros((10, C), device="cuda")
    with pytest.raises(ValueError, match="float32 CUDA"):
        DC.bio_viterbi(lg.cpu(), [10], table, 0.0, 0.0)
    with pytest.raises(ValueError, match="past the logits"):
        DC.bio_viterbi(lg, [11], table, 0.0, 0.0)
    with pytest.raises(ValueError, match="switch_penalty"):
        DC.bio_viterbi(lg, [10], table, -1.0, 0.0)
    with pytest.raises(ValueError, match="threshold"):
        DC.bio_viterbi(lg, [10], table, 0.0, -0.5)
    with pytest.raises(ValueError, match="o_id"):
        DC.bio_viterbi(lg, [10], (C, table[1]), 0.0, 0.0)
