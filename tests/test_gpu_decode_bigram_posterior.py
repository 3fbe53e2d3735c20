"""-m gpu: wfl_decode_bigram_posterior (csrc/decode_bigram_posterior.hip) against the float64 forward-backward of
tests/bio_bigram_posterior_ref.py, on the seeded logits and seeded transition tables of tests/test_gpu_decode_bigram.py, ragged batches.
The path given to the kernel and to the reference is wfl_decode_bigram's own output for the same clips, so near-ties of the search
cannot matter.  Every frame of every status-0 clip is compared.

Tolerances (none is a constant here; the rule of tests/test_gpu_decode_posterior.py): for every case the float32 log-domain restatement
of the reference (renormalised every 16 frames, offsets in float64) is run on the same inputs and the same path; its maximum deviation
from float64 over the case -- separately for logz, post and cls_post -- is the yardstick, and the kernel is allowed 4 x that against
float64.  The outputs are fp32: for a value whose half unit in the last place in that format is larger than the yardstick itself, that
half ulp is added, because no fp32 output could do without it.  The kernel runs in the scaled linear domain, where a posterior that
underflows fp32 is reported as 0: a value the float64 reference puts below 1e-30 may be 0.

Seeds: those of tests/test_gpu_decode_bigram.py, chosen on the CPU so that no frame's largest softmax probability is within MARGIN =
1e-4 of the threshold (asserted), so the kernel's fp32 pre-pass and the float64 one force the same frames.  The float64 posteriors of
every ragged case must also span the range (some < 0.2, some > 0.99, some in (0.3, 0.7); asserted): with one or two phonemes the
path's class rarely falls below 0.2, so P = 1 and 2 have clip seeds of their own, found on the CPU under both rules, and P = 64 with
forbidden entries a table seed of its own.

Phoneme counts: N = P + 1 symbols go to four wave slices of ceil(N / 4) and to lanes in groups of 64: 1 and 2 leave slices empty, 63,
64 and 65 stand on both sides of a lane group's edge, 70 is not divisible by four, 191 is the cap."""
import numpy as np
import pytest
import torch

import bio_bigram_posterior_ref as BP
import bio_bigram_ref as R
import bio_posterior_ref as P1
import test_gpu_decode_bigram as SB
from wfl_asr_amd import decode as DC

pytestmark = pytest.mark.gpu
MARGIN = SB.MARGIN
KEYS = ("logz", "post", "cls_post")
LENGTHS = [1, 2, 15, 16, 17, 0, 31, 32, 33, 300]
PHONEMES = [1, 2, 63, 64, 65, 70, 191]
assert LENGTHS == SB.LENGTHS and PHONEMES == SB.PHONEMES
CLIP_SEEDS = {**SB.SEEDS, 1: 855, 2: 608}
TABLE_SEEDS = {(64, 0.3): 3000}                 # default: 2000 + P


def _layout(clips, C, scattered):
    """-> (first row of every clip, the logits as a host array, columns to keep)."""
    T = [len(c) for c in clips]
    if scattered:
        offs, pos = [], 7
        for t in T:
            offs.append(pos)
            pos += t + 13
        big = np.full((pos, C + 19), 1e30, np.float32)      # anything read outside a clip's rows or columns would show
        for o, c in zip(offs, clips):
            big[o:o + len(c), :C] = c
        return offs, big
    offs = [int(x) for x in np.concatenate([[0], np.cumsum(T)[:-1]])] if clips else []
    return offs, np.ascontiguousarray(np.concatenate(clips) if clips else np.zeros((0, C), np.float32))


def _run(clips, table, W, thr, C, scattered=False, ids_edit=None, flat_lambda=None):
    """clips: list of z [T, C] float32 -> per clip dict(ids, score, vstatus, logz, post, cls_post, status), numpy.  flat_lambda: also
    wfl_decode_posterior at that penalty on the same ids, as flat_logz, flat_post, flat_cls_post, flat_status."""
    T = [len(c) for c in clips]
    offs, host = _layout(clips, C, scattered)
    lg = torch.from_numpy(host).cuda()[:, :C]
    ids, score, vst = DC.bio_viterbi_bigram(lg, T, table, W, thr, frame_offsets=offs)
    if ids_edit is not None:
        ids = ids_edit(ids.clone(), offs)
    logz, post, cls, st = DC.decode_posteriors_bigram(lg, T, table, W, thr, ids, frame_offsets=offs)
    outs = [ids, score, vst, logz, post, cls, st]
    if flat_lambda is not None:
        outs += list(DC.decode_posteriors(lg, T, table, flat_lambda, thr, ids, frame_offsets=offs))
    torch.cuda.synchronize()
    outs = [x.cpu().numpy() for x in outs]
    ids, score, vst, logz, post, cls, st = outs[:7]
    got = [dict(ids=ids[o:o + t], score=float(score[b]), vstatus=int(vst[b]), logz=np.array([logz[b]], np.float32), post=post[o:o + t],
                cls_post=cls[o:o + t], status=int(st[b])) for b, (o, t) in enumerate(zip(offs, T))]
    if flat_lambda is not None:
        fz, fp, fc, fs = outs[7:]
        for b, (o, t) in enumerate(zip(offs, T)):
            got[b].update(flat_logz=np.array([fz[b]], np.float32), flat_post=fp[o:o + t], flat_cls_post=fc[o:o + t], flat_status=int(fs[b]))
    return got


def _half_ulp(ref):
    return 0.5 * np.spacing(np.abs(np.asarray(ref, np.float64)).astype(np.float32)).astype(np.float64)


def _allowed(yard, ref):
    """What a kernel may deviate from the float64 value `ref`: 4 x the yardstick, plus half an fp32 ulp where that exceeds the yardstick."""
    h = _half_ulp(ref)
    return 4 * yard + np.where(yard < h, h, 0.0)


def _deviation(mine, ref):
    mine = mine.astype(np.float64)
    d = np.abs(mine - ref)
    d[(mine == 0) & (ref < 1e-30)] = 0.0                    # (the linear domain: an underflowed posterior is reported as 0)
    return d


def _check_case(name, clips, table, W, thr, got):
    """Every frame of every clip of a case against float64, by the 4 x yardstick rule; prints the figures before it asserts.
    -> (the float64 post and cls_post of every frame of the case, concatenated, forced frames, frames, the float64 results per clip,
    the yardsticks)."""
    yard = {k: 0.0 for k in KEYS}
    refs, n_forced = [], 0
    W64 = np.asarray(W, np.float64)
    for z, g in zip(clips, got):
        assert g["status"] == 0 and g["vstatus"] == 0, (name, g["status"], g["vstatus"])
        assert len(g["post"]) == len(g["cls_post"]) == len(z)
        lse, forced = SB.forced_frames(z, thr)
        n_forced += int(forced.sum())
        assert P1.path_is_legal(g["ids"], table, forced), "wfl_decode_bigram's path is not a path of the grammar"
        assert R.forbidden_successions(g["ids"], table, W64) == 0, "wfl_decode_bigram's path takes a forbidden succession"
        r64 = dict(zip(KEYS, BP.forward_backward(z, table, W64, forced, g["ids"])))
        r32 = dict(zip(KEYS, BP.forward_backward(z, table, W64, forced, g["ids"], dtype=np.float32)))
        for k in KEYS:
            ref = np.atleast_1d(np.asarray(r64[k], np.float64))
            if ref.size:
                yard[k] = max(yard[k], float(np.abs(np.atleast_1d(r32[k]) - ref).max()))
        r64["lse"] = float(lse.sum())
        r64["forced"] = forced
        refs.append(r64)
    dev = {k: 0.0 for k in KEYS}
    over = {k: 0.0 for k in KEYS}
    used_ulp = {k: False for k in KEYS}
    fin = W64[np.isfinite(W64)]
    w_top = max(0.0, float(fin.max())) if fin.size else 0.0
    for z, g, r64 in zip(clips, got, refs):
        if not len(z):
            assert g["logz"][0] == 0
            continue
        assert (g["cls_post"] >= 0).all() and (g["cls_post"] <= g["post"]).all() and (g["post"] <= 1).all()
        for k in KEYS:
            ref = np.atleast_1d(np.asarray(r64[k], np.float64))
            d = _deviation(g[k], ref)
            used_ulp[k] |= bool((yard[k] < _half_ulp(ref)).any())
            dev[k] = max(dev[k], float(d.max()))
            over[k] = max(over[k], float((d - _allowed(yard[k], ref)).max()))
        # logZ sums over every legal path, the search's among them, and over no more than every class string with the largest weight
        tol = float(_allowed(yard["logz"], r64["logz"]))
        assert float(g["logz"][0]) >= R.objective(g["ids"], z, table, W64, r64["forced"]) - tol
        assert float(g["logz"][0]) <= r64["lse"] + w_top * len(z) + tol + float(_half_ulp(r64["lse"]))
    for k in KEYS:
        print(f"{name} thr {thr}: {k}: kernel {dev[k]:.3e}, float32 restatement {yard[k]:.3e}, allowed 4 x = {4 * yard[k]:.3e}"
              f"{' (+ half an fp32 ulp where that exceeds the restatement)' if used_ulp[k] else ''}, over by {max(over[k], 0.0):.3e}")
    n = sum(len(z) for z in clips)
    print(f"{name}: {n_forced} of {n} frames forced")
    for k in KEYS:
        assert over[k] <= 0, (name, k, dev[k], yard[k], over[k])
    vals = np.concatenate([r[k] for r in refs for k in ("post", "cls_post")])
    return vals, n_forced, n, refs, yard


@pytest.mark.parametrize("P", PHONEMES)
@pytest.mark.parametrize("forbid,thr", [(0.0, 0.0), (0.3, SB.THRESHOLD)])
def test_ragged_batch_against_float64(P, forbid, thr):
    C, table, clips = SB.make_clips(P, CLIP_SEEDS[P])
    W = SB.make_trans(P, np.random.default_rng(TABLE_SEEDS.get((P, forbid), 2000 + P)), forbid)
    got = _run(clips, table, W, thr, C, scattered=True)
    assert len(got[LENGTHS.index(0)]["post"]) == 0 and got[LENGTHS.index(0)]["status"] == 0
    post, n_forced, n, _, _ = _check_case(f"P{P} forbid {forbid}", clips, table, W, thr, got)
    # (float64 reference values of post and cls_post together)
    assert post.min() < 0.2 and post.max() > 0.99 and ((post > 0.3) & (post < 0.7)).any(), "the posteriors do not span [0, 1] (test setup)"
    if thr > 0:
        assert 0 < n_forced < n, "the threshold does not force some but not all frames (test setup)"


@pytest.mark.parametrize("lam", [0.0, 1.5])
def test_a_flat_table_equals_the_flat_posterior(lam):
    """trans identically -lambda: the same ids to both posterior kernels; each within its own allowance of float64 (one reference:
    the two restatements agree to 1e-12, tests/test_decode_bigram_posterior_cpu.py), and the two within the sum of the allowances."""
    P = 70
    C, table, clips = SB.make_clips(P, SB.SEEDS[P])
    W = np.full((P + 1, P + 1), -lam, np.float32)
    got = _run(clips, table, W, SB.THRESHOLD, C, flat_lambda=lam)
    _, _, _, refs, yard = _check_case(f"flat lambda {lam}", clips, table, W, SB.THRESHOLD, got)
    flat_yard = {k: 0.0 for k in KEYS}
    for z, g, r64 in zip(clips, got, refs):
        r32 = dict(zip(KEYS, P1.forward_backward(z, table, lam, r64["forced"], g["ids"], dtype=np.float32)))
        for k in KEYS:
            ref = np.atleast_1d(np.asarray(r64[k], np.float64))
            if ref.size:
                flat_yard[k] = max(flat_yard[k], float(np.abs(np.atleast_1d(r32[k]) - ref).max()))
    for z, g, r64 in zip(clips, got, refs):
        assert g["flat_status"] == 0
        if not len(z):
            continue
        for k in KEYS:
            ref = np.atleast_1d(np.asarray(r64[k], np.float64))
            a_flat, a_big = _allowed(flat_yard[k], ref), _allowed(yard[k], ref)
            d_flat = _deviation(g["flat_" + k], ref)
            d_both = np.abs(g["flat_" + k].astype(np.float64) - g[k].astype(np.float64))
            d_both[(ref < 1e-30)] = 0.0
            print(f"flat lambda {lam} T {len(z)}: {k}: flat kernel {d_flat.max():.3e} (allowed {a_flat.max():.3e}), "
                  f"between the two {d_both.max():.3e} (allowed {(a_flat + a_big).max():.3e})")
            assert (d_flat <= a_flat).all(), k
            assert (d_both <= a_flat + a_big).all(), k


@pytest.mark.parametrize("forbid", [0.0, 0.3])
def test_one_6000_frame_clip(forbid):
    P = 70
    C, table, clips = SB.make_clips(P, 11077, lengths=[6000])
    W = SB.make_trans(P, np.random.default_rng(78), forbid)
    _check_case(f"T6000 forbid {forbid}", clips, table, W, 0.0, _run(clips, table, W, 0.0, C))


def test_a_dominant_class_outside_the_grammar():
    """The emissions are taken relative to the row maximum over all C classes.  A class that is never chosen stands 30 nats above
    everything on every frame (and an I class dominates frames where no path can reach it): every state of the grammar is then e^-30
    of the maximum, well inside what the scaled sums carry, and the outputs keep to the same rule."""
    P = 64
    C, table = SB.make_table(P)                             # class 0 and the last two are never chosen; I-0 is class 3
    rng = np.random.default_rng(77)
    a = (rng.standard_normal((200, C)) * 3).astype(np.float32)
    a[:, 0] += 30.0
    b = R.plant(150, C, table, rng, margin=4.0, scale=2.0)[0]
    b[::3, 3] += 30.0                                       # I-0, mostly where neither B-0 nor I-0 precedes
    for forbid in (0.0, 0.3):
        W = SB.make_trans(P, np.random.default_rng(79), forbid)
        got = _run([a, b], table, W, 0.0, C)
        vals = _check_case(f"off_grammar forbid {forbid}", [a, b], table, W, 0.0, got)[0]
        assert vals.min() < 0.5 and vals.max() > 0.9, "the posteriors are all alike (test setup)"


def test_a_clip_alone_equals_the_clip_in_a_batch_of_16():
    P = 65
    C, table = SB.make_table(P)
    rng = np.random.default_rng(3)
    W = SB.make_trans(P, rng, 0.3)
    clips = [(rng.standard_normal((int(rng.integers(1, 200)), C)) * 3).astype(np.float32) for _ in range(16)]
    batch = _run(clips, table, W, 0.0, C)
    _check_case("batch_of_16", clips, table, W, 0.0, batch)
    for b in (0, 5, 15):
        alone = _run([clips[b]], table, W, 0.0, C)[0]
        assert (alone["ids"] == batch[b]["ids"]).all() and alone["status"] == batch[b]["status"] == 0
        for k in KEYS:
            assert alone[k].tobytes() == batch[b][k].tobytes(), k


def test_symbol_cap_is_status_2_and_needs_no_workspace():
    P = 192
    C, table = SB.make_table(P)
    rng = np.random.default_rng(31)
    lg = torch.from_numpy(rng.standard_normal((50, C)).astype(np.float32)).cuda()
    ids = torch.ones(50, dtype=torch.int32, device="cuda")
    assert DC.bigram_posterior_workspace_bytes([20, 30], P) == 0 and DC.bigram_posterior_workspace_bytes([20, 30], P - 1) > 0
    logz, post, cls, st = DC.decode_posteriors_bigram(lg, [20, 30], table, SB.make_trans(P, rng), 0.0, ids)
    assert st.cpu().tolist() == [DC.STATUS_OVER_CAP] * 2 and logz.cpu().tolist() == [0.0, 0.0]
    assert not post.cpu().numpy().any() and not cls.cpu().numpy().any()


def test_class_cap_is_status_2():
    rng = np.random.default_rng(31)
    lg = torch.from_numpy(rng.standard_normal((50, 1025)).astype(np.float32)).cuda()
    ids = torch.zeros(50, dtype=torch.int32, device="cuda")
    pairs = [(2 * p + 1, 2 * p + 2) for p in range(100)]
    logz, post, cls, st = DC.decode_posteriors_bigram(lg, [20, 30], (0, pairs), SB.make_trans(100, rng), 0.0, ids)
    assert st.cpu().tolist() == [DC.STATUS_OVER_CAP] * 2 and logz.cpu().tolist() == [0.0, 0.0]
    assert not post.cpu().numpy().any() and not cls.cpu().numpy().any()


def test_a_bad_class_table_is_status_4():
    rng = np.random.default_rng(9)
    lg = torch.from_numpy(rng.standard_normal((40, 141)).astype(np.float32)).cuda()
    ids = torch.zeros(40, dtype=torch.int32, device="cuda")
    # a class used twice; O used as a B class; a class out of range; more pairs than classes (under the symbol cap)
    for pairs in ([(1, 2), (3, 2)], [(1, 2), (0, 4)], [(1, 2), (150, 4)], [(p % 100 + 1, -1) for p in range(150)]):
        W = SB.make_trans(len(pairs), rng)
        logz, post, cls, st = DC.decode_posteriors_bigram(lg, [20, 20], (0, pairs), W, 0.0, ids)
        assert st.cpu().tolist() == [DC.STATUS_BAD_CLASS] * 2 and logz.cpu().tolist() == [0.0, 0.0], pairs[:3]
        assert not post.cpu().numpy().any() and not cls.cpu().numpy().any()


def test_ids_that_are_no_path_are_status_8_for_that_clip_only():
    """Plain argument refusals: a hand-edited path is refused, not scored 0 / 0."""
    P = 64
    C, table = SB.make_table(P)                             # O = 1, B-p = 2 + 2p, I-0 = 3; class 0 is never chosen
    rng = np.random.default_rng(5)
    W = SB.make_trans(P, np.random.default_rng(6), 0.3)
    clips = [R.plant(120, C, table, rng, margin=12.0)[0] for _ in range(4)] + [(rng.standard_normal((90, C)) * 3).astype(np.float32)]
    # clip 4 gets a threshold-forced frame edited; the planted clips (largest probability near 1) have no forced frame
    thr = SB.THRESHOLD
    base = _run(clips, table, W, thr, C)
    assert [g["status"] for g in base] == [0] * 5
    forced4 = R.prepass(clips[4], thr)[1]
    assert forced4.any() and float(np.abs(R.prepass(clips[4], thr)[2] - thr).min()) > MARGIN
    assert not any(R.prepass(clips[b], thr)[1].any() for b in range(4))

    def o_between_o(ids):                                   # the first O frame between two O frames, or None
        at = np.nonzero((ids[1:-1] == 1) & (ids[:-2] == 1) & (ids[2:] == 1))[0] + 1
        return int(at[0]) if len(at) else None
    have = [b for b in range(4) if o_between_o(base[b]["ids"]) is not None]
    assert len(have) >= 2, "fewer than two planted clips with an O frame between O frames (test setup)"
    b_i, b_w = have[:2]                                     # the clips edited to I-0 after O / to a run through trans[O][q]
    b_c, b_keep = [b for b in range(4) if b not in (b_i, b_w)]      # a never-chosen class / left as it is
    t_i, t_w = o_between_o(base[b_i]["ids"]), o_between_o(base[b_w]["ids"])
    shut = np.nonzero(np.isneginf(W[0, 1:]))[0]
    open_ = np.nonzero(np.isfinite(W[0, 1:]))[0]
    assert len(shut) and len(open_)

    def edit(q):
        def f(ids, offs):
            h = ids.cpu().numpy()
            h[offs[b_i] + t_i] = 3                          # I-0 after O
            h[offs[b_c] + 50] = 0                           # a class that is never chosen
            h[offs[b_w] + t_w] = 2 + 2 * q                  # O, B-q, O: a run opened through trans[O][q]
            h[offs[4] + int(np.nonzero(forced4)[0][0])] = 2     # clip 4: B-0 on a forced frame
            return torch.from_numpy(h).cuda()
        return f
    got = _run(clips, table, W, thr, C, ids_edit=edit(int(shut[0])))
    assert [got[b]["status"] for b in (b_i, b_c, b_w, 4, b_keep)] == [8, 8, 8, 8, 0]
    for b in (b_i, b_c, b_w, 4):
        assert got[b]["logz"][0] == 0 and not got[b]["post"].any() and not got[b]["cls_post"].any()
    for k in KEYS:
        assert got[b_keep][k].tobytes() == base[b_keep][k].tobytes(), k
    # the same edit through a succession the table allows is a path (not the best one): it is scored
    got = _run(clips, table, W, thr, C, ids_edit=edit(int(open_[0])))
    assert [got[b]["status"] for b in (b_i, b_c, b_w, 4, b_keep)] == [8, 8, 0, 8, 0]
    assert got[b_w]["logz"][0] == base[b_w]["logz"][0] and got[b_w]["post"][t_w] < 0.5


def test_empty_clip_and_empty_batch():
    P = 65
    C, table = SB.make_table(P)
    rng = np.random.default_rng(2)
    W = SB.make_trans(P, rng, 0.3)
    z = (rng.standard_normal((30, C)) * 3).astype(np.float32)
    clips = [z[:10], z[:0], z[10:]]
    got = _run(clips, table, W, 0.0, C)
    _check_case("with_an_empty_clip", clips, table, W, 0.0, got)
    assert got[1]["status"] == 0 and got[1]["logz"][0] == 0 and len(got[1]["post"]) == 0
    assert _run([], table, W, 0.0, C) == []
    lg = torch.zeros((0, C), device="cuda")
    logz, post, cls, st = DC.decode_posteriors_bigram(lg, [0], table, W, 0.0, torch.zeros(0, dtype=torch.int32, device="cuda"))
    assert st.cpu().tolist() == [0] and logz.cpu().tolist() == [0.0] and post.numel() == 0 and cls.numel() == 0
    # a table with no phoneme: O everywhere, one path, every posterior 1
    got = _run([z], (1, []), np.zeros((1, 1), np.float32), 0.0, C)
    assert got[0]["status"] == 0 and (got[0]["post"] == 1).all() and (got[0]["cls_post"] == 1).all()
    assert abs(float(got[0]["logz"][0]) - float(z[:, 1].astype(np.float64).sum())) <= 1e-4


def test_argument_checks_of_the_python_entry():
    P = 65
    C, table = SB.make_table(P)
    W = SB.make_trans(P, np.random.default_rng(1))
    lg = torch.zeros((10, C), device="cuda")
    ids = torch.ones(10, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="float32 CUDA"):
        DC.decode_posteriors_bigram(lg.cpu(), [10], table, W, 0.0, ids)
    with pytest.raises(ValueError, match="float32 CUDA"):
        DC.decode_posteriors_bigram(lg.double(), [10], table, W, 0.0, ids)
    with pytest.raises(ValueError, match="past the logits"):
        DC.decode_posteriors_bigram(lg, [11], table, W, 0.0, ids)
    with pytest.raises(ValueError, match="threshold"):
        DC.decode_posteriors_bigram(lg, [10], table, W, -0.5, ids)
    with pytest.raises(ValueError, match="o_id"):
        DC.decode_posteriors_bigram(lg, [10], (C, table[1]), W, 0.0, ids)
    with pytest.raises(ValueError, match=r"\[66, 66\]"):
        DC.decode_posteriors_bigram(lg, [10], table, W[:-1], 0.0, ids)
    with pytest.raises(ValueError, match="float32"):
        DC.decode_posteriors_bigram(lg, [10], table, W.astype(np.float64), 0.0, ids)
    Wb = W.copy()
    Wb[3, 4] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        DC.decode_posteriors_bigram(lg, [10], table, Wb, 0.0, ids)
    Wb = W.copy()
    Wb[3, 0] = -np.inf
    with pytest.raises(ValueError, match=r"\[p\]\[O\]"):
        DC.decode_posteriors_bigram(lg, [10], table, Wb, 0.0, ids)
    for bad in (ids.cpu(), ids.long(), ids[:9], ids.view(5, 2), ids.cpu().numpy()):
        with pytest.raises(ValueError, match="ids must be"):
            DC.decode_posteriors_bigram(lg, [10], table, W, 0.0, bad)
