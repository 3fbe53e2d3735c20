"""-m gpu: wfl_align_min_duration_posterior (csrc/align_posterior.h with MIND; the chain is csrc/lattice.h chain_out / chain_shift and,
for beta, chain_in / chain_shift_back) against the float64 forward-backward over the expanded states of tests/duration_posterior_ref.py.
`tok` is what wfl_align_min_duration returned for the same PackedClips.

Tolerances follow the rule of tests/test_gpu_align_posterior.py (none is a constant here): for every case the float32 restatement of
the reference (same renormalisation period as the kernel) is run on the same inputs; its maximum deviation from float64 over the case --
separately for logz, tok_post, start_mean and start_sd -- is the yardstick, and the kernel is allowed 4 x that against float64.  Where
the yardstick is below half an fp32 ulp of the value itself (the outputs are fp32), that half ulp is added.  The figures are printed
before anything is asserted."""
import numpy as np
import pytest
import torch

import duration_posterior_ref as DP
import posterior_ref as P
import viterbi_min_ref as M
from wfl_asr_amd import align as AL

pytestmark = pytest.mark.gpu
C = 141
O_ID = 0
GAP_POOL = [O_ID, 137, 138, 139, 140, 135, 136, 133]
KEYS = ("logz", "tok_post", "start_mean", "start_sd")
CYCLE = (1, 1, 2, 3, 5, 8)


def _alts(N, rng, n_alt=1, repeat=False):
    out = []
    for k in range(N):
        if repeat and k % 3 == 1:
            out.append(out[-1])                       # the same token twice in a row
            continue
        ph = rng.choice(np.arange(1, 66), size=n_alt, replace=False)
        out.append([(int(2 * p - 1), int(2 * p)) for p in ph])
    return out


def _clip(T, N, D, rng, n_alt=1, n_gap=3, boost=0.0, repeat=False, wins=None):
    """-> (z, alternatives, gaps, D, windows or None)"""
    alts = _alts(N, rng, n_alt, repeat)
    return P.planted_logits(T, N, C, alts, GAP_POOL[:n_gap], rng, boost), alts, GAP_POOL[:n_gap], list(D), wins


def _upload(clips, scattered):
    T = [len(c[0]) for c in clips]
    if scattered:
        offs, pos = [], 7
        for t in T:
            offs.append(pos)
            pos += t + 13
        big = np.full((pos, C + 19), 1e30, np.float32)      # anything read outside a clip's rows or columns would show
        for o, c in zip(offs, clips):
            big[o:o + len(c[0]), :C] = c[0]
        return torch.from_numpy(big).cuda()[:, :C], T, offs
    offs = list(np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int64))
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([c[0] for c in clips]))).cuda(), T, offs


def _run(clips, scattered=False, tok_edit=None, search_without=False):
    """-> per clip dict(tok, score, vstatus, logz, tok_post, start_mean, start_sd, status, plain_logz).  One PackedClips for the search
    and the sums.  tok_edit(tok, offs): edits the device tok before the sums; search_without: tok comes from the search WITHOUT
    durations.  plain_logz: alignment_posteriors' logz of the same clips without durations (windows kept)."""
    lg, T, offs = _upload(clips, scattered)
    wins = [c[4] for c in clips]
    wins = wins if any(w is not None for w in wins) else None
    args = (lg, T, [c[1] for c in clips], [c[2] for c in clips])
    packed = AL.pack_clips(*args, offs, windows=wins, min_frames=[c[3] for c in clips])
    plain = AL.pack_clips(*args, offs, windows=wins)
    _, tok, score, vst = AL.viterbi_align(*args, O_ID, packed=plain if search_without else packed)
    _, ptok, _, pst = (None, tok, None, vst) if search_without else AL.viterbi_align(*args, O_ID, packed=plain)
    if tok_edit is not None:
        tok = tok_edit(tok.clone(), offs)
    logz, tp, mu, sd, st = AL.duration_posteriors(*args, O_ID, tok, packed=packed)
    plz = AL.alignment_posteriors(*args, O_ID, ptok, packed=plain)[0]
    torch.cuda.synchronize()
    tok, score, vst, logz, tp, mu, sd, st, plz, pst = (x.cpu().numpy() for x in (tok, score, vst, logz, tp, mu, sd, st, plz, pst))
    out, k0 = [], 0
    for b, (o, t) in enumerate(zip(offs, T)):
        n = len(clips[b][1])
        out.append(dict(tok=tok[o:o + t], score=float(score[b]), vstatus=int(vst[b]), logz=np.array([logz[b]], np.float32),
                        tok_post=tp[k0:k0 + n], start_mean=mu[k0:k0 + n], start_sd=sd[k0:k0 + n], status=int(st[b]),
                        plain_logz=float(plz[b]) if pst[b] == 0 else None))
        k0 += n
    return out


def _half_ulp(ref):
    return 0.5 * np.spacing(np.abs(np.asarray(ref, np.float64)).astype(np.float32)).astype(np.float64)


def _zeros(g):
    return g["logz"][0] == 0 and not g["tok_post"].any() and not g["start_mean"].any() and not g["start_sd"].any()


def _check_case(name, clips, got, refs=None):
    """Every clip of a case against float64, by the 4 x yardstick rule; prints the figures before it asserts.  Also the subset
    property: logz <= the logz of the lattice without durations, logz >= the float64 score of the min-duration Viterbi path, both up to
    the logz tolerance.  refs: a dict that keeps the float64 references (by clip index) for the caller."""
    yard = {k: 0.0 for k in KEYS}
    r64s = []
    for b, ((z, alts, gaps, D, wins), g) in enumerate(zip(clips, got)):
        assert g["status"] == g["vstatus"], (name, b, g["status"], g["vstatus"])
        if g["status"] != 0:
            assert _zeros(g), (name, b)
            r64s.append(None)
            continue
        assert (M.run_lengths([3 * k + 2 if k >= 0 else 0 for k in g["tok"]], len(alts)) >= np.array(D)).all(), (name, b)
        r64 = DP.forward_backward(z, alts, gaps, D, tok=g["tok"], windows=wins)
        r32 = DP.forward_backward(z, alts, gaps, D, tok=g["tok"], windows=wins, dtype=np.float32)
        assert (g["tok_post"] >= 0).all() and (g["tok_post"] <= 1 + 1e-6).all() and (g["start_sd"] >= 0).all()
        for k in KEYS:
            ref = np.atleast_1d(np.asarray(r64[k], np.float64))
            if ref.size:
                yard[k] = max(yard[k], float(np.abs(np.atleast_1d(r32[k]) - ref).max()))
        r64s.append(r64)
        if refs is not None:
            refs[b] = r64
    dev = {k: 0.0 for k in KEYS}
    over = {k: 0.0 for k in KEYS}
    used_ulp = {k: False for k in KEYS}
    above_path, below_plain = np.inf, np.inf
    for (z, alts, gaps, D, wins), g, r64 in zip(clips, got, r64s):
        if r64 is None:
            continue
        for k in KEYS:
            ref = np.atleast_1d(np.asarray(r64[k], np.float64))
            if not ref.size:
                continue
            d = np.abs(g[k].astype(np.float64) - ref)
            h = _half_ulp(ref)
            allowed = 4 * yard[k] + np.where(yard[k] < h, h, 0.0)
            used_ulp[k] |= bool((yard[k] < h).any())
            dev[k] = max(dev[k], float(d.max()))
            over[k] = max(over[k], float((d - allowed).max()))
        hz = float(_half_ulp(r64["logz"]))
        tol = 4 * yard["logz"] + (hz if yard["logz"] < hz else 0.0)
        above_path = min(above_path, float(g["logz"][0]) - DP.path_score(z, alts, gaps, g["tok"]) + tol)
        if g["plain_logz"] is not None:
            below_plain = min(below_plain, g["plain_logz"] - float(g["logz"][0]) + tol)
    for k in KEYS:
        print(f"{name}: {k}: kernel {dev[k]:.3e}, float32 restatement {yard[k]:.3e}, allowed 4 x = {4 * yard[k]:.3e}"
              f"{' (+ half an fp32 ulp where that exceeds the restatement)' if used_ulp[k] else ''}, over by {max(over[k], 0.0):.3e}")
    print(f"{name}: logz - float64 path score + tolerance >= {above_path:.3e}; logz without durations - logz + tolerance >= "
          f"{below_plain:.3e}")
    assert above_path >= 0 and below_plain >= 0, (name, above_path, below_plain)
    for k in KEYS:
        assert over[k] <= 0, (name, k, dev[k], yard[k], over[k])
    return yard, r64s


# ------------------------------------------------------------------------------------------------ 1. exactly one path
def _exact_clip(T_less=0):
    rng = np.random.default_rng(40)
    N = 40
    D = [CYCLE[k % 6] for k in range(N)]
    return _clip(sum(D) - T_less, N, D, rng, n_gap=3)


def test_exactly_one_path():
    clips = [_exact_clip(), _exact_clip(1)]
    assert len(clips[0][0]) == sum(clips[0][3]) == len(clips[1][0]) + 1
    got = _run(clips)
    refs = {}
    _check_case("exact", clips, got, refs)
    one, short = got
    assert one["status"] == 0 and short["status"] == 1 and _zeros(short)
    # the one path: every token for exactly D_k frames, no gap.  The reference says posterior 1, spread 0, logZ = the path's score
    assert (one["tok"] == np.repeat(np.arange(40), clips[0][3])).all()
    s64 = DP.path_score(*clips[0][:3], one["tok"])
    assert abs(refs[0]["logz"] - s64) < 1e-9 and np.allclose(refs[0]["tok_post"], 1.0, atol=1e-12) and not refs[0]["start_sd"].any()
    print(f"exact: logz {one['logz'][0]:.6f}, float64 path score {s64:.6f}; tok_post in [{one['tok_post'].min():.7f}, "
          f"{one['tok_post'].max():.7f}], start_sd <= {one['start_sd'].max():.3e}")


# ------------------------------------------------------------------------------------------------ 2. a ragged batch
def ragged_clips():
    rng = np.random.default_rng(23)
    clips = []
    # (T, N, alternatives per token, gap classes, equal neighbours, boost, durations)
    for T, N, na, ng, rep, boost, dur in [(1, 1, 1, 1, False, 0, "1"), (40, 1, 1, 3, False, 4, "8"), (60, 12, 1, 8, True, 4, "mix"),
                                          (90, 20, 4, 3, False, 4, "mix"), (90, 20, 4, 1, False, 0, "mix"), (300, 40, 2, 5, True, 0, "mix"),
                                          (200, 45, 1, 3, False, 4, "1"), (700, 150, 1, 4, False, 0, "mix"),
                                          (1500, 300, 1, 3, False, 4, "mix"), (1000, 128, 3, 6, False, 4, "mix"),
                                          (513, 100, 1, 2, True, 0, "mix"), (77, 5, 1, 3, False, 0, "9")]:
        D = {"1": [1] * N, "8": [8] * N, "9": [2, 3, 9, 1, 1][:N]}.get(dur) or [int(x) for x in rng.choice(CYCLE, N)]
        if dur != "9" and T > 1:                             # many paths, not a few (the one-frame clip has its one path)
            assert sum(D) <= T - N / 4, (T, N, sum(D))
        clips.append(_clip(T, N, D, rng, na, ng, float(boost), rep))
    return clips


def test_ragged_batch_against_float64():
    clips = ragged_clips()
    got = _run(clips, scattered=True)
    assert got[-1]["status"] == 4 and sum(g["status"] == 0 for g in got) == len(clips) - 1
    _check_case("ragged", clips, got)
    tp = np.concatenate([g["tok_post"] for g in got if g["status"] == 0])
    assert tp.min() < 0.2 and tp.max() > 0.99 and ((tp > 0.3) & (tp < 0.7)).any(), "the posteriors do not span [0, 1] (test setup)"


# ------------------------------------------------------------------------------------------------ 3. seams
def seam_clip():
    """T = 300, N = 20 (64 threads x 2 slots; 7 logits rows per stage at C = 141).  Token 8 (a thread's first slot) has D = 8 and may
    open only at frames 121 .. 127, token 13 (slot 2 * 6 + 1, a thread's last: its chain meets the neighbour exchange) D = 8 and
    frames 249 .. 255: each run's way from B through the chain into I straddles a 128-frame checkpoint, a 16-frame renormalisation and
    a 7-row stage boundary."""
    rng = np.random.default_rng(300)
    T, N = 300, 20
    D = [int(x) for x in rng.choice((1, 2, 3, 5), N)]
    D[8] = D[13] = 8
    wins = [AL.OPEN_WINDOW] * N
    wins[8], wins[13] = (121, 127), (249, 255)
    assert AL.windows_feasible(T, wins, D)
    for lo, hi in (wins[8], wins[13]):                       # a run opened at s: B at s, the chain at s + 1 .. s + 6, I from s + 7
        assert all(s // 128 != (s + 7) // 128 and s // 16 != (s + 7) // 16 and s // 7 != (s + 7) // 7 for s in range(lo, hi + 1))
    return _clip(T, N, D, rng, n_gap=3, boost=0.0, wins=wins)


def test_chains_across_checkpoint_renormalisation_and_stage():
    clips = [seam_clip()]
    got = _run(clips)
    assert got[0]["status"] == 0
    _check_case("seams", clips, got)
    for k, (lo, hi) in ((8, (121, 127)), (13, (249, 255))):
        first = int(np.nonzero(got[0]["tok"] == k)[0][0])
        assert lo <= first <= hi and lo - first <= got[0]["start_mean"][k] <= hi - first


# ------------------------------------------------------------------------------------------------ 4. each configuration
@pytest.mark.parametrize("N", [100, 300, 600, 1100, 2100])
def test_each_configuration(N):
    rng = np.random.default_rng(N)
    clips = [_clip(4 * N, N, [CYCLE[k % 6] for k in range(N)], rng, n_gap=3, boost=4.0)]
    got = _run(clips)
    assert got[0]["status"] == 0
    _check_case(f"config_N{N}", clips, got)


# ------------------------------------------------------------------------------------------------ 5. all D = 1
def test_all_ones_against_the_entry_without_durations():
    rng = np.random.default_rng(11)
    shapes = [(30, 12, 2), (300, 127, 1), (500, 300, 1), (800, 600, 1), (1300, 1100, 1), (2300, 2100, 1)]    # every configuration
    clips = [_clip(T, N, [1] * N, rng, na, 3, 4.0 * (i % 2)) for i, (T, N, na) in enumerate(shapes)]
    got = _run(clips)
    # (the reference with D = 1 is posterior_ref's: test_align_duration_posterior_cpu)
    yard, r64s = _check_case("all_ones", clips, got)
    lg, T, offs = _upload(clips, False)
    args = (lg, T, [c[1] for c in clips], [c[2] for c in clips], O_ID)
    _, tok, _, _ = AL.viterbi_align(*args)
    plain = [x.cpu().numpy() for x in AL.alignment_posteriors(*args, tok)]
    mine = [np.concatenate([g[k] for g in got]) for k in KEYS] + [np.array([g["status"] for g in got])]
    print("all_ones: bit-equal to wfl_align_posterior:", [bool(a.tobytes() == b.astype(a.dtype).tobytes()) for a, b in zip(plain, mine)])
    k0 = 0
    for b, c in enumerate(clips):                          # against each other, by the case's tolerance rule
        n = len(c[1])
        for j, k in enumerate(KEYS):
            ref = np.atleast_1d(np.asarray(r64s[b][k], np.float64))
            h = _half_ulp(ref)
            theirs = plain[j][b:b + 1] if k == "logz" else plain[j][k0:k0 + n]
            assert (np.abs(theirs.astype(np.float64) - got[b][k]) <= 4 * yard[k] + np.where(yard[k] < h, h, 0.0)).all(), (b, k)
        k0 += n


# ------------------------------------------------------------------------------------------------ 6. status 8
def test_a_tok_that_is_no_path_of_the_duration_lattice():
    rng = np.random.default_rng(8)
    clips = [_clip(120, 20, [int(x) for x in rng.choice(CYCLE, 20)], rng, boost=4.0) for _ in range(3)]
    clips[1][3][7] = 5
    good = _run(clips)
    assert all(g["status"] == 0 for g in good)
    run7 = np.nonzero(good[1]["tok"] == 7)[0]
    assert len(run7) >= 5                                   # token 7 of clip 1 keeps 4 frames, one fewer than its D_k = 5

    def shorten(tok, offs):
        tok[int(offs[1]) + int(run7[4]):int(offs[1]) + int(run7[-1]) + 1] = -1
        return tok
    bad = _run(clips, tok_edit=shorten)
    assert bad[1]["status"] == 8 and _zeros(bad[1])
    for b in (0, 2):                                        # the other clips of the batch are unchanged
        assert bad[b]["status"] == 0 and all(bad[b][k].tobytes() == good[b][k].tobytes() for k in KEYS)
    # a tok from the search WITHOUT durations in which a run really is shorter than its D_k (chosen on the host)
    rng = np.random.default_rng(9)
    for _ in range(20):
        clip = _clip(150, 30, [8 if k % 2 else 1 for k in range(30)], rng, boost=0.0)
        path, _ = M.viterbi(clip[0], clip[1], clip[2], [1] * 30)
        if (M.run_lengths(path, 30) < np.array(clip[3])).any():
            break
    else:
        raise AssertionError("no clip whose unconstrained path breaks a duration (test setup)")
    got = _run([clip, clips[0]], search_without=True)
    if (M.run_lengths([3 * k + 2 if k >= 0 else 0 for k in got[0]["tok"]], 30) < np.array(clip[3])).any():   # (the kernel's own path)
        assert got[0]["status"] == 8 and _zeros(got[0])
    else:
        pytest.fail("the search without durations met every duration: the host's choice of clip does not hold for the kernel's path")


# ------------------------------------------------------------------------------------------------ 7. batching
def test_a_clip_alone_equals_the_clip_in_a_batch_of_16():
    rng = np.random.default_rng(3)
    clips = []
    for b in range(16):
        N = int(rng.integers(1, 400))
        D = [int(x) for x in rng.choice((1, 1, 2, 3), N)]
        T = sum(D) + int(rng.integers(N // 4 + 1, N + 100))
        clips.append(_clip(T, N, D, rng, int(rng.integers(1, 5)), int(rng.integers(1, 9)), 4.0 * (b % 2)))
    batch = _run(clips)
    _check_case("batch_of_16", clips, batch)
    for b in (0, 5, 15):
        alone = _run([clips[b]])[0]
        assert alone["status"] == batch[b]["status"] == 0
        for k in KEYS:
            assert alone[k].tobytes() == batch[b][k].tobytes(), (b, k)
