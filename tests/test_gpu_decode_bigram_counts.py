"""-m gpu: wfl_decode_bigram_counts (csrc/decode_bigram_counts.hip) against the float64 expected successions of
tests/bio_bigram_counts_ref.py, on the seeded logits and seeded transition tables of tests/test_gpu_decode_bigram.py, ragged batches.
Every entry of every status-0 clip's table is compared.

Tolerances (none is a constant here; the rule of tests/test_gpu_decode_bigram_posterior.py): for every case the float32 log-domain
restatement of the reference (alpha, beta and the running counts in fp32, renormalised every 16 frames, offsets in float64) is run on the
same inputs; its maximum deviation from float64 over the case -- separately for logz, for the tables' entries and for the tables'
totals -- is the yardstick, and the kernel is allowed 4 x that against float64, plus half an fp32 ulp of the value where that half ulp
exceeds the yardstick (no fp32 output could do without it).  The figures are printed before anything is asserted.

Seeds: the clip seeds of tests/test_gpu_decode_bigram.py (no frame within MARGIN of the threshold; forced_frames asserts it) and table
seeds 2000 + P, as the posterior test.  The float64 counts of every ragged case must hold an entry below 1e-3, an entry above 0.5 and,
with forbid > 0, a forbidden entry (asserted on the reference alone): the 2 x 2 table of P = 1 has a table seed of its own, found on the
CPU under that rule (it forbids p after p).

Phoneme counts: N = P + 1 symbols go to four wave slices of ceil(N / 4) and to lanes in groups of 64, and the kernel is instantiated
per number of lane groups: 1 and 2 leave slices empty, 63 fills the first instantiation, 64 and 65 are the second's smallest, 70 is not
divisible by four, 191 is the cap (the third)."""
import functools

import numpy as np
import pytest
import torch

import bio_bigram_counts_ref as BC
import bio_bigram_posterior_ref as BP
import bio_bigram_ref as R
import test_gpu_decode_bigram as SB
from test_gpu_decode_bigram_posterior import _allowed, _layout
from wfl_asr_amd import decode as DC

pytestmark = pytest.mark.gpu
LENGTHS, PHONEMES, THRESHOLD = SB.LENGTHS, SB.PHONEMES, SB.THRESHOLD
assert PHONEMES == [1, 2, 63, 64, 65, 70, 191]
TABLE_SEEDS = {(1, 0.3): 3007}                  # default: 2000 + P


def _run(clips, table, W, thr, C, scattered=False):
    """clips: list of z [T, C] float32 -> per clip dict(logz, counts, status), numpy."""
    T = [len(c) for c in clips]
    offs, host = _layout(clips, C, scattered)
    lg = torch.from_numpy(host).cuda()[:, :C]
    logz, counts, st = DC.bigram_expected_counts(lg, T, table, W, thr, frame_offsets=offs)
    torch.cuda.synchronize()
    logz, counts, st = logz.cpu().numpy(), counts.cpu().numpy(), st.cpu().numpy()
    n = len(table[1]) + 1
    assert counts.shape == (len(clips), n, n) and counts.dtype == np.float32
    return [dict(logz=np.float32(logz[b]), counts=counts[b], status=int(st[b])) for b in range(len(clips))]


def _reference(clips, table, W, thr):
    """-> (per clip (logz, counts) in float64, yardsticks dict(logz, counts, total))."""
    W64 = np.asarray(W, np.float64)
    refs, yard = [], dict(logz=0.0, counts=0.0, total=0.0)
    for z in clips:
        _, forced = SB.forced_frames(z, thr)
        r64 = BC.expected_counts(z, table, W64, forced)
        r32 = BC.expected_counts(z, table, W64, forced, dtype=np.float32)
        yard["logz"] = max(yard["logz"], abs(r32[0] - r64[0]))
        yard["counts"] = max(yard["counts"], float(np.abs(r32[1] - r64[1]).max()))
        yard["total"] = max(yard["total"], abs(float(r32[1].sum()) - float(r64[1].sum())))
        refs.append(r64)
    return refs, yard


def _check_case(name, clips, W, got, refs, yard):
    """Every clip of a case against float64 by the 4 x yardstick rule; prints the figures before it asserts.  -> what logz was allowed,
    per clip."""
    shut = np.isneginf(np.asarray(W, np.float64))
    dev = dict(logz=0.0, counts=0.0, total=0.0)
    over = dict(logz=-np.inf, counts=-np.inf, total=-np.inf)
    allowed_logz = []
    for z, g, (lz, cn) in zip(clips, got, refs):
        assert g["status"] == 0, (name, g["status"])
        mine = g["counts"].astype(np.float64)
        assert np.isfinite(mine).all() and np.isfinite(g["logz"]), name
        assert (mine >= 0).all() and mine[0, 0] == 0.0 and (mine[shut] == 0.0).all(), name
        if not len(z):
            assert g["logz"] == 0 and not mine.any()
            allowed_logz.append(0.0)
            continue
        for k, m, r in (("logz", float(g["logz"]), lz), ("counts", mine, cn), ("total", float(mine.sum()), float(cn.sum()))):
            d = np.abs(np.asarray(m, np.float64) - r)
            dev[k] = max(dev[k], float(d.max()))
            over[k] = max(over[k], float((d - _allowed(yard[k], r)).max()))
        allowed_logz.append(float(_allowed(yard["logz"], lz)))
    for k in dev:
        print(f"{name}: {k}: kernel {dev[k]:.3e}, float32 restatement {yard[k]:.3e}, allowed 4 x = {4 * yard[k]:.3e} (+ half an fp32 ulp "
              f"where that exceeds the restatement), over by {max(over[k], 0.0):.3e}")
    for k in dev:
        assert over[k] <= 0, (name, k, dev[k], yard[k], over[k])
    return allowed_logz


@functools.lru_cache(maxsize=None)
def ragged_case(P, forbid, thr):
    """The inputs of a ragged case and their references, computed once: (C, table, clips, W, refs, yard)."""
    C, table, clips = SB.make_clips(P, SB.SEEDS[P])
    W = SB.make_trans(P, np.random.default_rng(TABLE_SEEDS.get((P, forbid), 2000 + P)), forbid)
    refs, yard = _reference(clips, table, W, thr)
    return C, table, clips, W, refs, yard


CASES = [(0.0, 0.0), (0.3, THRESHOLD)]


@pytest.mark.parametrize("P", PHONEMES)
@pytest.mark.parametrize("forbid,thr", CASES)
def test_ragged_batch_against_float64(P, forbid, thr):
    C, table, clips, W, refs, yard = ragged_case(P, forbid, thr)
    # the condition on the inputs, on the reference alone
    allc = np.concatenate([cn.ravel() for (_, cn), z in zip(refs, clips) if len(z)])
    shut = np.isneginf(W)
    shut[0, 0] = False
    assert ((allc > 0) & (allc < 1e-3)).any() and allc.max() > 0.5, "the counts do not span the range (test setup)"
    if forbid > 0:
        assert shut.any(), "no forbidden entry (test setup)"
    got = _run(clips, table, W, thr, C, scattered=True)
    assert got[LENGTHS.index(0)]["status"] == 0 and not got[LENGTHS.index(0)]["counts"].any()
    _check_case(f"P{P} forbid {forbid} thr {thr}", clips, W, got, refs, yard)


@pytest.mark.parametrize("P", [2, 70, 191])
def test_logz_equals_the_posterior_entry(P):
    """wfl_decode_bigram_posterior on the same clips, its path from wfl_decode_bigram: the two logz agree within the sum of the two
    allowances (each its own fp32 restatement against float64)."""
    forbid, thr = 0.3, THRESHOLD
    C, table, clips, W, refs, yard = ragged_case(P, forbid, thr)
    T = [len(c) for c in clips]
    offs, host = _layout(clips, C, False)
    lg = torch.from_numpy(host).cuda()
    ids, _, vst = DC.bio_viterbi_bigram(lg, T, table, W, thr, frame_offsets=offs)
    plogz, _, _, pst = DC.decode_posteriors_bigram(lg, T, table, W, thr, ids, frame_offsets=offs)
    clogz, _, cst = DC.bigram_expected_counts(lg, T, table, W, thr, frame_offsets=offs)
    torch.cuda.synchronize()
    assert not vst.cpu().numpy().any() and not pst.cpu().numpy().any() and not cst.cpu().numpy().any()
    ids, plogz, clogz = ids.cpu().numpy(), plogz.cpu().numpy().astype(np.float64), clogz.cpu().numpy().astype(np.float64)
    W64 = np.asarray(W, np.float64)
    pyard = 0.0
    for z, o in zip(clips, offs):
        if len(z):
            _, forced = SB.forced_frames(z, thr)
            a = BP.forward_backward(z, table, W64, forced, ids[o:o + len(z)])[0]
            b = BP.forward_backward(z, table, W64, forced, ids[o:o + len(z)], dtype=np.float32)[0]
            pyard = max(pyard, abs(a - b))
    for b, (z, (lz, _)) in enumerate(zip(clips, refs)):
        allow = float(_allowed(yard["logz"], lz)) + float(_allowed(pyard, lz)) if len(z) else 0.0
        print(f"P{P} T {len(z)}: logz counts {clogz[b]:.6f} posterior {plogz[b]:.6f} float64 {lz:.6f}; differ by "
              f"{abs(clogz[b] - plogz[b]):.3e}, allowed {allow:.3e}")
        assert abs(clogz[b] - plogz[b]) <= allow


@pytest.mark.parametrize("forbid", [0.0, 0.3])
def test_one_6000_frame_clip(forbid):
    P = 70
    C, table, clips = SB.make_clips(P, 11077, lengths=[6000])
    W = SB.make_trans(P, np.random.default_rng(78), forbid)
    refs, yard = _reference(clips, table, W, 0.0)
    _check_case(f"T6000 forbid {forbid}", clips, W, _run(clips, table, W, 0.0, C), refs, yard)


def test_a_dominant_class_outside_the_grammar():
    """The posterior test's case: a never-chosen class stands 30 nats above everything on every frame, and an I class dominates frames
    where no path can reach it.  Every state of the grammar is then e^-30 of the row maximum, the frame constant large: the same rule,
    and no NaN or inf anywhere in the outputs."""
    P = 64
    C, table = SB.make_table(P)                             # class 0 and the last two are never chosen; I-0 is class 3
    rng = np.random.default_rng(77)
    a = (rng.standard_normal((200, C)) * 3).astype(np.float32)
    a[:, 0] += 30.0
    b = R.plant(150, C, table, rng, margin=4.0, scale=2.0)[0]
    b[::3, 3] += 30.0                                       # I-0, mostly where neither B-0 nor I-0 precedes
    for forbid in (0.0, 0.3):
        W = SB.make_trans(P, np.random.default_rng(79), forbid)
        refs, yard = _reference([a, b], table, W, 0.0)
        got = _run([a, b], table, W, 0.0, C)
        for g in got:
            assert np.isfinite(g["counts"]).all() and np.isfinite(g["logz"])
        _check_case(f"off_grammar forbid {forbid}", [a, b], W, got, refs, yard)


def test_a_clip_alone_equals_the_clip_in_a_batch_of_16():
    P = 65
    C, table = SB.make_table(P)
    rng = np.random.default_rng(3)
    W = SB.make_trans(P, rng, 0.3)
    clips = [(rng.standard_normal((int(rng.integers(1, 200)), C)) * 3).astype(np.float32) for _ in range(16)]
    batch = _run(clips, table, W, 0.0, C)
    for b in (0, 5, 15):
        alone = _run([clips[b]], table, W, 0.0, C)[0]
        assert alone["status"] == batch[b]["status"] == 0
        assert alone["logz"].tobytes() == batch[b]["logz"].tobytes()
        assert alone["counts"].tobytes() == batch[b]["counts"].tobytes() and alone["counts"].any()


def test_symbol_cap_is_status_2_and_needs_no_workspace():
    P = 192
    C, table = SB.make_table(P)
    rng = np.random.default_rng(31)
    lg = torch.from_numpy(rng.standard_normal((50, C)).astype(np.float32)).cuda()
    assert DC.bigram_counts_workspace_bytes([20, 30], P) == 0 and DC.bigram_counts_workspace_bytes([20, 30], P - 1) > 0
    logz, counts, st = DC.bigram_expected_counts(lg, [20, 30], table, SB.make_trans(P, rng), 0.0)
    assert st.cpu().tolist() == [DC.STATUS_OVER_CAP] * 2 and logz.cpu().tolist() == [0.0, 0.0]
    assert counts.shape == (2, P + 1, P + 1) and not counts.cpu().numpy().any()


def test_class_cap_is_status_2():
    rng = np.random.default_rng(31)
    lg = torch.from_numpy(rng.standard_normal((50, 1025)).astype(np.float32)).cuda()
    pairs = [(2 * p + 1, 2 * p + 2) for p in range(100)]
    logz, counts, st = DC.bigram_expected_counts(lg, [20, 30], (0, pairs), SB.make_trans(100, rng), 0.0)
    assert st.cpu().tolist() == [DC.STATUS_OVER_CAP] * 2 and logz.cpu().tolist() == [0.0, 0.0]
    assert not counts.cpu().numpy().any()


def test_a_bad_class_table_is_status_4():
    rng = np.random.default_rng(9)
    lg = torch.from_numpy(rng.standard_normal((40, 141)).astype(np.float32)).cuda()
    # a class used twice; O used as a B class; a class out of range; more pairs than classes (under the symbol cap)
    for pairs in ([(1, 2), (3, 2)], [(1, 2), (0, 4)], [(1, 2), (150, 4)], [(p % 100 + 1, -1) for p in range(150)]):
        W = SB.make_trans(len(pairs), rng)
        logz, counts, st = DC.bigram_expected_counts(lg, [20, 20], (0, pairs), W, 0.0)
        assert st.cpu().tolist() == [DC.STATUS_BAD_CLASS] * 2 and logz.cpu().tolist() == [0.0, 0.0], pairs[:3]
        assert not counts.cpu().numpy().any()


def test_empty_clip_and_empty_batch():
    P = 65
    C, table = SB.make_table(P)
    rng = np.random.default_rng(2)
    W = SB.make_trans(P, rng, 0.3)
    z = (rng.standard_normal((30, C)) * 3).astype(np.float32)
    clips = [z[:10], z[:0], z[10:]]
    got = _run(clips, table, W, 0.0, C)
    refs, yard = _reference(clips, table, W, 0.0)
    _check_case("with_an_empty_clip", clips, W, got, refs, yard)
    assert got[1]["status"] == 0 and got[1]["logz"] == 0 and not got[1]["counts"].any()
    assert _run([], table, W, 0.0, C) == []
    lg = torch.zeros((0, C), device="cuda")
    logz, counts, st = DC.bigram_expected_counts(lg, [0], table, W, 0.0)
    assert st.cpu().tolist() == [0] and logz.cpu().tolist() == [0.0] and not counts.cpu().numpy().any()
    # a table with no phoneme: O everywhere, one path, no succession
    got = _run([z], (1, []), np.zeros((1, 1), np.float32), 0.0, C)
    assert got[0]["status"] == 0 and got[0]["counts"].shape == (1, 1) and got[0]["counts"][0, 0] == 0.0
    assert abs(float(got[0]["logz"]) - float(z[:, 1].astype(np.float64).sum())) <= 1e-4


def test_argument_checks_of_the_python_entry():
    P = 65
    C, table = SB.make_table(P)
    W = SB.make_trans(P, np.random.default_rng(1))
    lg = torch.zeros((10, C), device="cuda")
    with pytest.raises(ValueError, match="float32 CUDA"):
        DC.bigram_expected_counts(lg.cpu(), [10], table, W, 0.0)
    with pytest.raises(ValueError, match="float32 CUDA"):
        DC.bigram_expected_counts(lg.double(), [10], table, W, 0.0)
    with pytest.raises(ValueError, match="past the logits"):
        DC.bigram_expected_counts(lg, [11], table, W, 0.0)
    with pytest.raises(ValueError, match="threshold"):
        DC.bigram_expected_counts(lg, [10], table, W, -0.5)
    with pytest.raises(ValueError, match="o_id"):
        DC.bigram_expected_counts(lg, [10], (C, table[1]), W, 0.0)
    with pytest.raises(ValueError, match=r"\[66, 66\]"):
        DC.bigram_expected_counts(lg, [10], table, W[:-1], 0.0)
    with pytest.raises(ValueError, match="float32"):
        DC.bigram_expected_counts(lg, [10], table, W.astype(np.float64), 0.0)
    Wb = W.copy()
    Wb[3, 4] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        DC.bigram_expected_counts(lg, [10], table, Wb, 0.0)
    Wb = W.copy()
    Wb[3, 0] = -np.inf
    with pytest.raises(ValueError, match=r"\[p\]\[O\]"):
        DC.bigram_expected_counts(lg, [10], table, Wb, 0.0)
