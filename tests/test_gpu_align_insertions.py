"""-m gpu: wfl_align_insertions (csrc/align_edits.hip) against the float64 closed form of tests/align_insertions_ref.py, which
tests/test_align_insertions_cpu.py holds against the definition (logZ of every transcript with one token inserted).

ins -- tolerances: the rule of tests/test_gpu_align_edits.py, no constant of its own.  For every case the float32 restatement of
align_insertions_ref is run on the same inputs; its maximum deviation from float64 over the finite entries of the case is the
yardstick, and the kernel is allowed 4 x that against float64, plus half an fp32 ulp of the value where the yardstick is smaller
than that half ulp (the outputs are fp32).  An entry that is -inf in the reference must be -inf.  The figures are printed before the
assertion.

logz -- wfl_align_posterior's (wfl_align_posterior_windowed's) logz of the same batch: asserted equal to alignment_posteriors' logz on
the same PackedClips within test_gpu_align_edits' logz bound.

The identity that gives the scores their meaning: if token k of a transcript has the single alternative subs[p], inserting p at place k
of the transcript WITHOUT k rebuilds the transcript, so ins(shortened)[k][p] = -edits(full)[k][deletion column]; held here between the
two kernels.  wfl_align_edits itself is held to its output on the commit before this entry joined its translation unit
(tests/golden/align_edits_parent.npz), byte for byte."""
import os

import numpy as np
import pytest
import torch

import align_edits_ref as E
import align_insertions_ref as R
import test_gpu_align_edits as GE
from wfl_asr_amd import align as AL

pytestmark = pytest.mark.gpu
O_ID = 0
C_SMALL = GE.C_SMALL
SUBS6 = GE.SUBS6
_clip, _pairs, _half_ulp = GE._clip, GE._pairs, GE._half_ulp


def _run(clips, subs, scattered=False, with_posterior=True):
    """clips: [(z, alts, gaps, windows)] -> per clip dict(logz, ins [N + 1, P], status, plogz); GE._run for insertion_scores."""
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
    logz, ins, status = AL.insertion_scores(*args, O_ID, subs, frame_offsets=offs, packed=packed)
    plogz = None
    if with_posterior:                                     # the search and the scores share one PackedClips
        _, tok, _, vst = AL.viterbi_align(*args, O_ID, frame_offsets=offs, packed=packed)
        plogz, _, _, _, pst = AL.alignment_posteriors(*args, O_ID, tok, frame_offsets=offs, packed=packed)
        plogz, pst, vst = plogz.cpu().numpy(), pst.cpu().numpy(), vst.cpu().numpy()
    torch.cuda.synchronize()
    logz, ins, status = logz.cpu().numpy(), ins.cpu().numpy(), status.cpu().numpy()
    assert ins.shape == (sum(len(c[1]) for c in clips) + len(clips), len(subs))
    out, k0 = [], 0
    for b, c in enumerate(clips):
        n = len(c[1]) + 1                                  # clip b's rows start at (its first token's row) + b
        g = dict(logz=logz[b], ins=ins[k0:k0 + n], status=int(status[b]))
        if with_posterior:
            assert int(vst[b]) == g["status"] and (g["status"] != 0 or int(pst[b]) == 0), (b, pst[b], vst[b], g["status"])
            g["plogz"] = plogz[b]
        out.append(g)
        k0 += n
    return out


def _yardsticks(clips, subs, got, name):
    """-> (refs: float64 result or None per clip, yard: dict(logz, ins) of the float32 restatement's deviations over the case)."""
    yard = {"logz": 0.0, "ins": 0.0}
    refs = []
    for (z, alts, gaps, wins), g in zip(clips, got):
        r64 = R.insertion_scores(z, alts, gaps, subs, wins)
        if g["status"] != 0:
            assert r64 is None, (name, g["status"])
            assert g["logz"] == 0 and not g["ins"].any()
            refs.append(None)
            continue
        assert r64 is not None, name
        r32 = R.insertion_scores(z, alts, gaps, subs, wins, dtype=np.float32)
        fin = np.isfinite(r64["ins"])
        assert (np.isfinite(r32["ins"]) == fin).all()
        yard["logz"] = max(yard["logz"], abs(r32["logz"] - r64["logz"]))
        if fin.any():
            yard["ins"] = max(yard["ins"], float(np.abs(r32["ins"][fin] - r64["ins"][fin]).max()))
        refs.append(r64)
    return refs, yard


def _allowed(yard, ref):
    h = _half_ulp(ref)
    return 4 * yard + np.where(yard < h, h, 0.0)


def _check_case(name, clips, subs, got):
    refs, yard = _yardsticks(clips, subs, got, name)
    dev = {"logz": 0.0, "ins": 0.0}
    over = {"logz": -np.inf, "ins": -np.inf}
    bitwise, n_inf, n_fin, pover = True, 0, 0, -np.inf
    for g, r64 in zip(got, refs):
        if r64 is None:
            continue
        fin = np.isfinite(r64["ins"])
        assert (g["ins"][~fin] == -np.inf).all(), (name, "an entry that is -inf in the reference")
        assert np.isfinite(g["ins"][fin]).all(), name
        n_inf += int((~fin).sum())
        n_fin += int(fin.sum())
        for key, val, ref in (("logz", np.array([g["logz"]]), np.array([r64["logz"]])), ("ins", g["ins"][fin], r64["ins"][fin])):
            if not ref.size:
                continue
            d = np.abs(val.astype(np.float64) - ref)
            dev[key] = max(dev[key], float(d.max()))
            over[key] = max(over[key], float((d - _allowed(yard[key], ref)).max()))
        if "plogz" in g:
            bitwise &= np.float32(g["logz"]).tobytes() == np.float32(g["plogz"]).tobytes()
            pover = max(pover, abs(float(g["plogz"]) - float(g["logz"])) - float(_allowed(yard["logz"], r64["logz"])))
    for key in ("logz", "ins"):
        print(f"{name}: {key}: kernel {dev[key]:.3e}, float32 restatement {yard[key]:.3e}, allowed 4 x = {4 * yard[key]:.3e} "
              f"(+ half an fp32 ulp where that exceeds the restatement), over by {max(over[key], 0.0):.3e}")
    print(f"{name}: {n_fin} finite entries, {n_inf} -inf in the reference and in the kernel; logz bit for bit alignment_posteriors': "
          f"{bitwise}")
    assert pover <= 0, (name, "logz against alignment_posteriors' logz", pover)
    assert over["ins"] <= 0, (name, dev["ins"], yard["ins"], over["ins"])
    return n_fin, n_inf


@pytest.mark.parametrize("T,N", [(5, 0), (6, 6), (7, 6)])
def test_no_token_as_many_tokens_as_frames_and_one_frame_to_spare(T, N):
    """N = 0: one place.  T = N: status 0, every entry -inf.  T = N + 1: every place has exactly one frame."""
    rng = np.random.default_rng(100 * T + N)
    clips = [_clip(T, N, C_SMALL, rng, boost=4.0), _clip(T, N, C_SMALL, rng, boost=0.0)]
    got = _run(clips, SUBS6)
    assert [g["status"] for g in got] == [0, 0]
    n_fin, n_inf = _check_case(f"T{T}_N{N}", clips, SUBS6, got)
    assert (n_fin == 0) if T == N else (n_inf == 0)


@pytest.mark.parametrize("T,Ns", [(70, (63, 64)), (140, (127, 128))])
def test_row_width_and_configuration_switch(T, Ns):
    """N = 63 / 64: round64(N + 1) crosses a row width.  N = 127 / 128: configuration 0 -> 1, and at N = 127 slot N is the last
    thread's last slot."""
    clips = []
    for N in Ns:
        rng = np.random.default_rng(N)
        clips += [_clip(T, N, C_SMALL, rng, boost=4.0, repeat=True), _clip(T, N, C_SMALL, rng, boost=0.0)]
    n_fin, n_inf = _check_case(f"T{T}_N{Ns[0]}_{Ns[1]}", clips, SUBS6, _run(clips, SUBS6))
    assert n_inf == 0


def test_the_largest_configuration():
    """N = 2050 at T = 2100, P = 2: the 512 x 9 configuration."""
    rng = np.random.default_rng(2050)
    clips = [_clip(2100, 2050, C_SMALL, rng, boost=4.0)]
    _check_case("N2050", clips, SUBS6[:2], _run(clips, SUBS6[:2]))


@pytest.mark.parametrize("P", [0, 1, 64, 65])
def test_table_sizes(P):
    """No substitute (no column: logz and status alone), one, a full wave, one more."""
    rng = np.random.default_rng(P)
    subs = _pairs(141)[:P]
    assert len(subs) == P
    clips = [_clip(40, 5, 141, rng, boost=4.0), _clip(23, 4, 141, rng, n_alt=3, boost=0.0)]
    _check_case(f"P{P}", clips, subs, _run(clips, subs))


@pytest.mark.parametrize("T", [15, 16, 17, 33, 35])
def test_renormalisation_staging_boundary_and_group_tail(T):
    """The renormalisation period (16), the staging boundary at 32 frames, the four-frame group's tail."""
    rng = np.random.default_rng(T)
    clips = [_clip(T, 4, C_SMALL, rng, n_alt=2, boost=4.0), _clip(T, 9, C_SMALL, rng, repeat=True, boost=0.0)]
    n_fin, n_inf = _check_case(f"T{T}", clips, SUBS6, _run(clips, SUBS6))
    assert n_inf == 0


def test_windows_of_half_width_three_and_zero_in_one_batch():
    rng = np.random.default_rng(31)
    clips = [_clip(100, 40, C_SMALL, rng, boost=4.0, windows=3), _clip(100, 40, C_SMALL, rng, boost=4.0, windows=0),
             _clip(100, 40, C_SMALL, rng, n_alt=2, boost=0.0, windows=0)]
    got = _run(clips, SUBS6)
    assert [g["status"] for g in got] == [0, 0, 0]
    n_fin, n_inf = _check_case("windowed", clips, SUBS6, got)
    assert n_fin > 0 and n_inf > 0                         # (pinned neighbours that follow each other at once leave no frame between them)


def ragged_clips():
    rng = np.random.default_rng(21)
    return [_clip(T, N, C_SMALL, rng, n_alt=na, repeat=rep, boost=b) for T, N, na, rep, b in
            [(1, 0, 1, False, 0.0), (40, 3, 1, False, 4.0), (150, 130, 2, True, 4.0), (10, 12, 1, False, 0.0), (90, 30, 4, False, 0.0)]]


def test_ragged_scattered_batch():
    """Five clips of two configurations at scattered frame offsets of a logits tensor with a larger row stride and 1e30 outside the
    clips; one has fewer frames than tokens (status 1, zeros in its N + 1 rows).  Clip b's rows start at tok_off[b] + b."""
    clips = ragged_clips()
    got = _run(clips, SUBS6, scattered=True)
    assert [g["status"] for g in got] == [0, 0, 0, 1, 0]
    _check_case("ragged", clips, SUBS6, got)
    alone = _run([clips[2]], SUBS6)[0]                     # a clip alone equals the clip in the batch
    assert alone["ins"].tobytes() == got[2]["ins"].tobytes() and alone["logz"] == got[2]["logz"]


def test_a_substitute_class_out_of_range_is_status_4_for_every_clip():
    rng = np.random.default_rng(41)
    clips = [_clip(20, 3, C_SMALL, rng), _clip(30, 5, C_SMALL, rng)]
    got = _run(clips, SUBS6[:2] + [(C_SMALL, 2)], with_posterior=False)
    assert [g["status"] for g in got] == [4, 4]
    assert all(g["logz"] == 0 and not g["ins"].any() for g in got)


def test_inserting_a_deleted_token_again_is_minus_its_deletion():
    """ins(transcript without k)[k][p] = -edits(transcript)[k][deletion], token k's one alternative being subs[p].  Allowed: the sum of
    the two entries' bounds for the case (each 4 x its float32 restatement's deviation, plus the half ulp), plus what the two float64
    references themselves differ by."""
    rng = np.random.default_rng(51)
    N, T = 9, 50
    alts, gaps = [[SUBS6[int(p)]] for p in rng.integers(0, 6, N)], [O_ID]
    z = E.P.planted_logits(T, N, C_SMALL, alts, gaps, rng, 4.0)
    full = (z, alts, gaps, None)
    g_ed = GE._run([full], SUBS6, with_posterior=False)[0]
    e64 = E.edit_scores(z, alts, gaps, SUBS6)["edits"]
    e32 = E.edit_scores(z, alts, gaps, SUBS6, dtype=np.float32)["edits"]
    yard_e = float(np.abs(e32 - e64).max())
    short = [(z, alts[:k] + alts[k + 1:], gaps, None) for k in range(N)]
    g_in = _run(short, SUBS6, with_posterior=False)
    refs, yard = _yardsticks(short, SUBS6, g_in, "identity")
    worst = -np.inf
    for k in range(N):
        p = SUBS6.index(alts[k][0])
        ri, re = refs[k]["ins"][k, p], e64[k, -1]
        allowed = float(_allowed(yard["ins"], ri)) + float(_allowed(yard_e, re)) + abs(ri + re)
        d = abs(float(g_in[k]["ins"][k, p]) + float(g_ed["edits"][k, -1]))
        print(f"identity: token {k}: insertion {g_in[k]['ins'][k, p]:.6f}, deletion {g_ed['edits'][k, -1]:.6f}, sum {d:.3e}, allowed "
              f"{allowed:.3e} (float64 references differ by {abs(ri + re):.1e})")
        worst = max(worst, d - allowed)
    assert worst <= 0, worst


# ---- wfl_align_edits is what it was
def edits_golden_clips():
    """test_gpu_align_edits.test_multi_alternative_and_repeated_tokens' case."""
    rng = np.random.default_rng(11)
    return [_clip(60, 20, C_SMALL, rng, n_alt=4, boost=4.0), _clip(60, 20, C_SMALL, rng, n_alt=2, repeat=True, boost=4.0),
            _clip(50, 12, C_SMALL, rng, n_alt=1, repeat=True, boost=0.0)]


WS_CASES = [(5, 0), (6, 6), (7, 6), (70, 63), (70, 64), (140, 127), (140, 128), (2100, 2050), (40, 5), (23, 4), (15, 4), (16, 9), (17, 4),
            (33, 9), (35, 4), (100, 40), (1, 0), (150, 130), (10, 12), (90, 30)]


def test_wfl_align_edits_is_byte_for_byte_the_parents(golden_dir):
    want = np.load(os.path.join(golden_dir, "align_edits_parent.npz"))
    got = GE._run(edits_golden_clips(), SUBS6, with_posterior=False)
    assert np.concatenate([g["edits"] for g in got]).tobytes() == want["edits"].tobytes()
    assert np.array([g["logz"] for g in got], np.float32).tobytes() == want["logz"].tobytes()
    assert [g["status"] for g in got] == list(want["status"])
    assert [list(c) for c in want["ws_cases"]] == [list(c) for c in WS_CASES]
    assert [AL.edits_workspace_bytes([T], [N]) for T, N in WS_CASES] == list(want["ws_bytes"])
