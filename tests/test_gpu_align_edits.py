"""-m gpu: wfl_align_edits (csrc/align_edits.hip) against the float64 closed form of tests/align_edits_ref.py, which
tests/test_align_edits_cpu.py holds against the definition (logZ of every edited transcript).

edits -- tolerances (none is a constant here; the rule of tests/test_gpu_align_posterior.py): for every case the float32 restatement
of align_edits_ref is run on the same inputs; its maximum deviation from float64 over the finite entries of the case is the
yardstick, and the kernel is allowed 4 x that against float64, plus half an fp32 ulp of the value where the yardstick is smaller
than that half ulp (the outputs are fp32).  An entry that is -inf in the reference must be -inf.  The figures are printed before the
assertion.

logz -- by definition wfl_align_posterior's (wfl_align_posterior_windowed's) logz of the same batch, and held to that: asserted equal
to alignment_posteriors' logz on the same PackedClips within that test's logz bound (4 x the restatement's logz deviation over the
case, plus the half ulp where that is larger).  Observed on the MI355X: bit for bit equal on every clip of every case here -- the
forward sweep is the posterior's arithmetic.  The deviation of logz from float64 is printed beside the restatement's, not asserted a
second time: it is the posterior kernel's own, and on clips with few paths (windows) it sits at the fp32 output's own rounding, e.g.
the windowed case: kernel 2.94e-5 at logz = -785 (half an fp32 ulp there: 3.05e-5), restatement 2.7e-6."""
import numpy as np
import pytest
import torch

import align_edits_ref as E
import test_align_edits_cpu as CPU
from wfl_asr_amd import align as AL

pytestmark = pytest.mark.gpu
O_ID = 0


def _pairs(C):
    return [(2 * p - 1, 2 * p) for p in range(1, (C - 1) // 2 + 1)]


def _alts(N, C, rng, n_alt=1, repeat=False):
    ph = _pairs(C)
    out = []
    for k in range(N):
        if repeat and k % 3 == 1:
            out.append(out[-1])                       # the same token twice in a row
            continue
        out.append([ph[int(j)] for j in rng.choice(len(ph), size=n_alt, replace=False)])
    return out


def _clip(T, N, C, rng, n_alt=1, repeat=False, boost=4.0, windows=None, gaps=(O_ID,)):
    """-> (z, alternatives, gaps, windows); windows: None, or a half-width w: (start - w, start + w) around an increasing random
    sequence of starts (always feasible)."""
    alts = _alts(N, C, rng, n_alt, repeat)
    z = E.P.planted_logits(T, N, C, alts, list(gaps), rng, boost)
    wins = None
    if windows is not None and N:
        st = np.sort(rng.choice(T, N, replace=False))
        wins = [(max(int(s) - windows, 0), min(int(s) + windows, T - 1)) for s in st]
    return z, alts, list(gaps), wins


def _run(clips, subs, scattered=False, with_posterior=True):
    """clips: [(z, alts, gaps, windows)] -> per clip dict(logz, edits, status, plogz).  All clips of a call are windowed or none is."""
    T = [len(c[0]) for c in clips]
    C = clips[0][0].shape[1]
    if scattered:
        offs, pos = [], 7
        for t in T:
            offs.append(pos)
            pos += t + 13
        big = np.full((pos, C + 19), 1e30, np.float32)      # anything read outside a clip's rows or columns would show
        for o, c in zip(offs, clips):
            big[o:o + len(c[0]), :C] = c[0]
        lg = torch.from_numpy(big).cuda()[:, :C]
    else:
        offs = list(np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int64))
        lg = torch.from_numpy(np.ascontiguousarray(np.concatenate([c[0] for c in clips]))).cuda()
    windowed = any(c[3] is not None for c in clips)
    args = (lg, T, [c[1] for c in clips], [c[2] for c in clips])
    packed = AL.pack_clips(*args, frame_offsets=offs, windows=[c[3] for c in clips] if windowed else None)
    assert (packed.d_win is not None) == windowed
    logz, edits, status = AL.edit_scores(*args, O_ID, subs, frame_offsets=offs, packed=packed)
    plogz = None
    if with_posterior:                                     # the search and both scores share one PackedClips
        _, tok, _, vst = AL.viterbi_align(*args, O_ID, frame_offsets=offs, packed=packed)
        plogz, _, _, _, pst = AL.alignment_posteriors(*args, O_ID, tok, frame_offsets=offs, packed=packed)
        plogz, pst, vst = plogz.cpu().numpy(), pst.cpu().numpy(), vst.cpu().numpy()
    torch.cuda.synchronize()
    logz, edits, status = logz.cpu().numpy(), edits.cpu().numpy(), status.cpu().numpy()
    assert edits.shape == (sum(len(c[1]) for c in clips), len(subs) + 1)
    out, k0 = [], 0
    for b, c in enumerate(clips):
        n = len(c[1])
        g = dict(logz=logz[b], edits=edits[k0:k0 + n], status=int(status[b]))
        if with_posterior:
            # (the search's status; the posterior's too where the search found a path -- without one its `tok` is no path, status 8)
            assert int(vst[b]) == g["status"] and (g["status"] != 0 or int(pst[b]) == 0), (b, pst[b], vst[b], g["status"])
            g["plogz"] = plogz[b]
        out.append(g)
        k0 += n
    return out


def _half_ulp(ref):
    return 0.5 * np.spacing(np.abs(np.asarray(ref, np.float64)).astype(np.float32)).astype(np.float64)


def _check_case(name, clips, subs, got):
    yard = {"logz": 0.0, "edits": 0.0}
    refs = []
    for (z, alts, gaps, wins), g in zip(clips, got):
        r64 = E.edit_scores(z, alts, gaps, subs, wins)
        if g["status"] != 0:
            assert r64 is None, (name, g["status"])
            assert g["logz"] == 0 and not g["edits"].any()
            refs.append(None)
            continue
        assert r64 is not None, name
        r32 = E.edit_scores(z, alts, gaps, subs, wins, dtype=np.float32)
        fin = np.isfinite(r64["edits"])
        assert (np.isfinite(r32["edits"]) == fin).all()
        yard["logz"] = max(yard["logz"], abs(r32["logz"] - r64["logz"]))
        if fin.any():
            yard["edits"] = max(yard["edits"], float(np.abs(r32["edits"][fin] - r64["edits"][fin]).max()))
        refs.append(r64)
    dev = {"logz": 0.0, "edits": 0.0}
    over = {"logz": -np.inf, "edits": -np.inf}
    bitwise, n_inf, pover = True, 0, -np.inf
    for g, r64 in zip(got, refs):
        if r64 is None:
            continue
        fin = np.isfinite(r64["edits"])
        assert (g["edits"][~fin] == -np.inf).all(), (name, "an entry that is -inf in the reference")
        assert np.isfinite(g["edits"][fin]).all(), name
        n_inf += int((~fin).sum())
        for key, val, ref in (("logz", np.array([g["logz"]]), np.array([r64["logz"]])), ("edits", g["edits"][fin], r64["edits"][fin])):
            if not ref.size:
                continue
            d = np.abs(val.astype(np.float64) - ref)
            h = _half_ulp(ref)
            allowed = 4 * yard[key] + np.where(yard[key] < h, h, 0.0)
            dev[key] = max(dev[key], float(d.max()))
            over[key] = max(over[key], float((d - allowed).max()))
        if "plogz" in g:
            bitwise &= np.float32(g["logz"]).tobytes() == np.float32(g["plogz"]).tobytes()
            h = float(_half_ulp(r64["logz"]))
            pover = max(pover, abs(float(g["plogz"]) - float(g["logz"])) - (4 * yard["logz"] + (h if yard["logz"] < h else 0.0)))
    for key in ("logz", "edits"):
        print(f"{name}: {key}: kernel {dev[key]:.3e}, float32 restatement {yard[key]:.3e}, allowed 4 x = {4 * yard[key]:.3e} "
              f"(+ half an fp32 ulp where that exceeds the restatement), over by {max(over[key], 0.0):.3e}")
    print(f"{name}: {n_inf} entries -inf in the reference and in the kernel; logz bit for bit alignment_posteriors': {bitwise} "
          f"(logz against float64 is over its own 4 x bound by {max(over['logz'], 0.0):.3e}: the posterior kernel's figure)")
    assert pover <= 0, (name, "logz against alignment_posteriors' logz", pover)
    assert over["edits"] <= 0, (name, dev["edits"], yard["edits"], over["edits"])


C_SMALL = 31
SUBS6 = _pairs(C_SMALL)[:6]


@pytest.mark.parametrize("T,N", [(1, 1), (3, 3), (9, 0), (11, 2), (11, 3), (17, 3), (129, 3), (257, 3)])
def test_small_shapes(T, N):
    """One frame, T == N, no token, the thread boundary at R = 2 (N = 2, 3), the renormalisation period and the stage / block seams
    in T."""
    rng = np.random.default_rng(100 * T + N)
    clips = [_clip(T, N, C_SMALL, rng, boost=4.0), _clip(T, N, C_SMALL, rng, boost=0.0)]
    _check_case(f"T{T}_N{N}", clips, SUBS6, _run(clips, SUBS6))


def test_the_configuration_switch():
    """N = 127 (64 threads) and N = 128 (256 threads) at T = 140, each with and without a planted path, one case."""
    clips = []
    for N in (127, 128):
        rng = np.random.default_rng(N)
        clips += [_clip(140, N, C_SMALL, rng, boost=4.0, repeat=True), _clip(140, N, C_SMALL, rng, boost=0.0)]
    _check_case("cfg_switch", clips, SUBS6, _run(clips, SUBS6))


def test_more_than_two_stages_of_the_logits_ring():
    rng = np.random.default_rng(7)
    clips = [_clip(70, 9, 141, rng, n_alt=2, boost=4.0, gaps=(O_ID, 137, 138)), _clip(70, 30, 141, rng, boost=0.0, gaps=(O_ID, 137))]
    subs = _pairs(141)[:6]
    _check_case("C141_T70", clips, subs, _run(clips, subs))


@pytest.mark.parametrize("P", [0, 1, 64, 65, 130])
def test_table_sizes(P):
    """No substitute (the deletion column alone), one, a full wave, one more, and 130 on a label set of 261 classes."""
    C = 261 if P == 130 else 141
    rng = np.random.default_rng(P)
    subs = _pairs(C)[:P]
    assert len(subs) == P
    clips = [_clip(40, 5, C, rng, boost=4.0), _clip(23, 4, C, rng, n_alt=3, boost=0.0)]
    _check_case(f"P{P}", clips, subs, _run(clips, subs))


def test_multi_alternative_and_repeated_tokens():
    rng = np.random.default_rng(11)
    clips = [_clip(60, 20, C_SMALL, rng, n_alt=4, boost=4.0), _clip(60, 20, C_SMALL, rng, n_alt=2, repeat=True, boost=4.0),
             _clip(50, 12, C_SMALL, rng, n_alt=1, repeat=True, boost=0.0)]
    _check_case("multi_alt_repeat", clips, SUBS6, _run(clips, SUBS6))


def test_single_alternative_in_the_table_scores_zero():
    """The first invariant: a token whose one alternative is row p of the table has edits[k][p] = 0 up to rounding."""
    rng = np.random.default_rng(12)
    alts, gaps = [[SUBS6[k % 6]] for k in range(8)], [O_ID]
    z = E.P.planted_logits(50, 8, C_SMALL, alts, gaps, rng, 4.0)
    clips = [(z, alts, gaps, None), (E.P.planted_logits(50, 8, C_SMALL, alts, gaps, rng, 0.0), alts, gaps, None)]
    got = _run(clips, SUBS6)
    _check_case("own_phoneme", clips, SUBS6, got)
    r64 = E.edit_scores(z, alts, gaps, SUBS6)              # (exactly 0 by definition; _check_case has held the kernel to it)
    assert max(abs(r64["edits"][k, k % 6]) for k in range(8)) < 1e-9
    print("own phoneme: kernel", [float(got[0]["edits"][k, k % 6]) for k in range(8)])


def ragged_clips():
    rng = np.random.default_rng(21)
    clips = [_clip(T, N, C_SMALL, rng, n_alt=na, repeat=rep, boost=b) for T, N, na, rep, b in
             [(1, 1, 1, False, 0.0), (40, 3, 1, False, 4.0), (150, 130, 2, True, 4.0), (10, 12, 1, False, 0.0), (620, 600, 1, False, 4.0),
              (90, 30, 4, False, 0.0), (300, 127, 1, True, 4.0), (1100, 1030, 1, False, 4.0)]]
    return clips


def test_ragged_scattered_batch_mixing_configurations():
    """Clips of four configurations at scattered frame offsets of a logits tensor with a larger row stride and 1e30 outside the clips;
    one clip has fewer frames than tokens (status 1, zeros)."""
    clips = ragged_clips()
    got = _run(clips, SUBS6, scattered=True)
    assert [g["status"] for g in got] == [0, 0, 0, 1, 0, 0, 0, 0]
    _check_case("ragged", clips, SUBS6, got)
    alone = _run([clips[2]], SUBS6)[0]                     # a clip alone equals the clip in the batch
    assert alone["edits"].tobytes() == got[2]["edits"].tobytes() and alone["logz"] == got[2]["logz"]


def test_windowed_clips_share_the_packed_batch_with_the_search():
    """Pinned, +-2 and wide windows, beside a clip whose windows no path satisfies (status 1)."""
    rng = np.random.default_rng(31)
    clips = [_clip(60, 12, C_SMALL, rng, boost=4.0, windows=0), _clip(60, 12, C_SMALL, rng, boost=4.0, windows=2),
             _clip(150, 129, C_SMALL, rng, boost=0.0, windows=2), _clip(80, 10, C_SMALL, rng, n_alt=2, boost=4.0, windows=30)]
    z, alts, gaps, _ = _clip(30, 4, C_SMALL, rng)
    clips.append((z, alts, gaps, [(5, 4)] * 4))             # lo > hi: never
    got = _run(clips, SUBS6)
    assert [g["status"] for g in got] == [0, 0, 0, 0, 1]
    _check_case("windowed", clips, SUBS6, got)


def test_a_substitute_class_out_of_range_is_status_4_for_every_clip():
    rng = np.random.default_rng(41)
    clips = [_clip(20, 3, C_SMALL, rng), _clip(30, 5, C_SMALL, rng)]
    got = _run(clips, SUBS6[:2] + [(C_SMALL, 2)], with_posterior=False)
    assert [g["status"] for g in got] == [4, 4]
    assert all(g["logz"] == 0 and not g["edits"].any() for g in got)
    bad = [list(a) for a in clips[1][1]]
    bad[2] = [(C_SMALL + 3, 4)]                            # a token's class out of range: that clip alone
    got = _run([clips[0], (clips[1][0], bad, clips[1][2], None)], SUBS6, with_posterior=False)
    assert [g["status"] for g in got] == [0, 4] and not got[1]["edits"].any() and got[0]["edits"].any()


@pytest.mark.parametrize("seed", CPU.SWAP_SEEDS)
def test_a_planted_substitution_is_found(seed):
    z, alts, gaps, subs, j, planted = CPU.swap_case(seed)
    got = _run([(z, alts, gaps, None)], subs)[0]
    print(f"seed {seed}: token {j}, planted column {planted}: {got['edits'][j, planted]:.3f}; largest elsewhere "
          f"{np.delete(got['edits'], j, 0).max():.3f}")
    CPU.assert_swap_verdict(got["edits"], j, planted, alts, subs)


@pytest.mark.parametrize("seed", CPU.INSERT_SEEDS)
def test_a_planted_insertion_is_found(seed):
    z, alts, gaps, subs, j = CPU.insert_case(seed)
    got = _run([(z, alts, gaps, None)], subs)[0]
    print(f"seed {seed}: inserted token {j}: deletion ratio {got['edits'][j, -1]:.3f}")
    assert got["edits"][j, -1] > 0
