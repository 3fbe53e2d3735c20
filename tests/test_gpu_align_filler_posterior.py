"""-m gpu: wfl_align_filler_posterior (csrc/align_filler_posterior.hip) against the float64 forward-backward over the filler lattice of
tests/filler_posterior_ref.py.  `tok` is what wfl_align_filler returned for the same clips, flags and penalty.

Tolerances are the rule of tests/test_gpu_align_posterior.py and tests/test_gpu_align_optional_posterior.py, restated here for the six
float outputs (end_mean and end_sd fall under it like the rest): for every case the float32 restatement of the reference (same
renormalisation period as the kernel) is run on the same inputs; its maximum deviation from float64 over the case, per output, is the
yardstick, and the kernel is allowed 4 x that against float64; where the yardstick is below half an fp32 ulp of the value itself, that
half ulp is added (the outputs are fp32).  Every clip and token of every case is compared, and the figures are printed before
anything is asserted.  The one bit-for-bit assertion is "a clip alone equals the clip in a batch": same kernel, same arithmetic."""
import ctypes

import numpy as np
import pytest
import torch

import filler_posterior_ref as FP
import viterbi_filler_ref as R
from wfl_asr_amd import align as AL

pytestmark = pytest.mark.gpu
C = 141
O_ID = 0
GAPS = [O_ID, 137, 138]
KEYS = FP.OUTPUTS
SLOTS = ((127, 2), (511, 2), (1023, 4), (2047, 8), (4096, 9))          # csrc/lattice.h: token cap of a configuration, its R
BLOCK = 128                                                            # csrc/align_posterior.h POST_W: frames per recomputed block
OPEN = (0, 2 ** 31 - 1)


def _slots(N):
    return next(r for cap, r in SLOTS if N <= cap)


def _alts(N, rng, fill=None):
    """Random phonemes, none equal to either of the two before it; a filler's entry is the placeholder pair."""
    ph = []
    for k in range(N):
        while True:
            p = int(rng.integers(1, 68))
            if p not in ph[-2:]:
                break
        ph.append(p)
    return [[(O_ID, O_ID)] if fill is not None and fill[k] else [(2 * p - 1, 2 * p)] for k, p in enumerate(ph)]


def _run(clips, phi, windows=None, tok_edit=None, post_windows="same"):
    """clips: list of (z [T, C] float32, alternatives, flags) -> per clip a dict of the search's tok / status and the entry's outputs."""
    T = [len(c[0]) for c in clips]
    lg = torch.from_numpy(np.ascontiguousarray(np.concatenate([c[0] for c in clips]))).cuda()
    args = (lg, T, [c[1] for c in clips], [GAPS] * len(clips), O_ID, [c[2] for c in clips])
    _, tok, _, vst = AL.viterbi_align_filler(*args, phi, windows=windows)
    if tok_edit is not None:
        tok = tok_edit(tok.clone())
    out = AL.filler_posteriors(*args, tok, phi, windows=windows if post_windows == "same" else post_windows)
    torch.cuda.synchronize()
    tok, vst = tok.cpu().numpy(), vst.cpu().numpy()
    logz, tp, mu, sd, emu, esd, st = (x.cpu().numpy() for x in out)
    res, pos, k0 = [], 0, 0
    for b, t in enumerate(T):
        n = len(clips[b][1])
        res.append(dict(tok=tok[pos:pos + t], vstatus=int(vst[b]), logz=np.array([logz[b]], np.float32), tok_post=tp[k0:k0 + n],
                        start_mean=mu[k0:k0 + n], start_sd=sd[k0:k0 + n], end_mean=emu[k0:k0 + n], end_sd=esd[k0:k0 + n],
                        status=int(st[b])))
        pos += t
        k0 += n
    return res


def _zeros(g):
    return g["logz"][0] == 0 and not any(g[k].any() for k in KEYS[1:])


def _half_ulp(ref):
    return 0.5 * np.spacing(np.abs(np.asarray(ref, np.float64)).astype(np.float32)).astype(np.float64)


REFS = {}                                   # a reference is computed once per (case, clip) and left unchanged


def _refs(key, z, alts, fill, phi, tok, win):
    if key not in REFS:
        REFS[key] = (FP.forward_backward(z, alts, GAPS, fill, phi, tok=tok, windows=win),
                     FP.forward_backward(z, alts, GAPS, fill, phi, tok=tok, windows=win, dtype=np.float32))
    return REFS[key]


def _check_case(name, clips, phi, got, windows=None, keys=KEYS):
    """Every clip of a case against float64, by the 4 x yardstick rule; prints the figures before it asserts."""
    yard = {k: 0.0 for k in keys}
    refs = []
    for b, ((z, alts, fill), g) in enumerate(zip(clips, got)):
        win = windows[b] if windows is not None else None
        assert g["status"] == g["vstatus"], (name, b, g["status"], g["vstatus"])
        if g["status"] != 0:
            assert _zeros(g)
            if g["status"] == 1:
                assert FP.forward_backward(z, alts, GAPS, fill, phi, windows=win) is None
            refs.append(None)
            continue
        r64, r32 = _refs((name, b, phi), z, alts, fill, phi, g["tok"], win)
        assert r64 is not None, (name, b)
        assert (g["tok_post"] >= 0).all() and (g["tok_post"] <= 1).all() and (g["start_sd"] >= 0).all() and (g["end_sd"] >= 0).all()
        for k in keys:
            ref = np.atleast_1d(np.asarray(r64[k], np.float64))
            if ref.size:
                yard[k] = max(yard[k], float(np.abs(np.atleast_1d(r32[k]) - ref).max()))
        refs.append(r64)
    dev = {k: 0.0 for k in keys}
    over = {k: -np.inf for k in keys}
    for g, r64 in zip(got, refs):
        if r64 is None:
            continue
        for k in keys:
            ref = np.atleast_1d(np.asarray(r64[k], np.float64))
            if not ref.size:
                continue
            d = np.abs(g[k].astype(np.float64) - ref)
            h = _half_ulp(ref)
            allowed = 4 * yard[k] + np.where(yard[k] < h, h, 0.0)
            dev[k] = max(dev[k], float(d.max()))
            over[k] = max(over[k], float((d - allowed).max()))
    for k in keys:
        print(f"{name}: {k}: kernel {dev[k]:.3e}, float32 restatement {yard[k]:.3e}, allowed 4 x = {4 * yard[k]:.3e} (+ half an fp32 ulp "
              f"where that exceeds the restatement), over by {max(over[k], 0.0):.3e}")
    for k in keys:
        assert over[k] <= 0, (name, k, dev[k], yard[k], over[k])
    return refs


# ------------------------------------------------------------------------------------ one shape per launch configuration, boundaries
def _boundary_tokens(N, R_):
    """Slots R - 1, 0 and 1 of a thread, and the first token of the second wave: where alpha reads the left thread's last slot and
    beta (and leave) the right thread's first.  Never two in a row."""
    return [k for k in (10 * R_ - 1, 13 * R_, 17 * R_ + 1, 64 * R_) if 0 < k < N - 1]


def _block_runs(T, N, fill, rng):
    """Runs (gap frames in front, frames) per token, about 1.3 frames a token, a filler 4 frames, laid out so that at the boundaries of
    the recomputed blocks one token's run ends on the block's last frame and the next token is the single first frame of the next
    block: the two places where leave_k crosses from one block into the other."""
    runs, t, single = [], 0, False
    spare = T - N - 3 * int(np.sum(fill)) - 8                # frames beyond one per token (a filler: four)
    for k in range(N):
        nxt = (t // BLOCK + 1) * BLOCK
        if single:                                           # the single first frame of a block
            g, d, single = 0, 1, False
        else:
            g = int(spare > 0 and rng.random() < 0.15)
            d = 4 if fill[k] else 1 + int(spare > 0 and rng.random() < 0.2)
            if not fill[k] and k + 1 < N and not fill[k + 1] and nxt - t <= 3 and spare >= 2:
                g, d, single = 0, nxt - t, True              # ends on the block's last frame
        spare -= g + d - (4 if fill[k] else 1)
        runs.append((g, d))
        t += g + d
    assert sum(g + d for g, d in runs) <= T
    return runs


def _planted_clip(N, seed, stretch=1.3, margin=4.0):
    """T about 1.3 N + 37 (several 128-frame blocks, no multiple of 16), fillers on the boundary slots."""
    rng = np.random.default_rng(seed)
    R_ = _slots(N)
    T = int(stretch * N) + 37
    T += T % 16 == 0
    fill = np.zeros(N, np.int32)
    bnd = _boundary_tokens(N, R_)
    fill[bnd] = 1
    alts = _alts(N, rng, fill)
    z, _ = R.plant(T, N, C, alts, GAPS, rng, fill=fill, runs=_block_runs(T, N, fill, rng), margin=margin, scale=1.5)
    return (z, alts, fill), bnd


def _last_frames(tok, N):
    return np.array([int(np.nonzero(tok == k)[0][-1]) for k in range(N)])


CONFIG_N = (100, 300, 700, 1500, 2500)


def test_one_shape_per_launch_configuration():
    made = [_planted_clip(N, N) for N in CONFIG_N]
    clips = [m[0] for m in made]
    got = _run(clips, 0.7)
    _check_case("configurations", clips, 0.7, got)
    for (clip, bnd), g in zip(made, got):
        assert g["status"] == 0 and len(bnd) >= 3 and clip[2][bnd].all()
        last = _last_frames(g["tok"], len(clip[1]))
        assert (last % BLOCK == BLOCK - 1).any(), "no run ends on the last frame of a block"
        assert (last[last >= BLOCK] % BLOCK == 0).any(), "no run ends on the first frame of a block"
        assert (g["tok_post"][bnd] > 0).all()


# ------------------------------------------------------------------------------------------------------------------ start and end
def _small(T, N, fill, seed, runs=None, margin=2.0):
    rng = np.random.default_rng(seed)
    fill = np.asarray(fill, np.int32)
    alts = _alts(N, rng, fill)
    z, _ = R.plant(T, N, C, alts, GAPS, rng, fill=fill, runs=runs, margin=margin, scale=1.5)
    return z, alts, fill


def test_a_filler_first_last_and_alone():
    clips = [_small(23, 4, [1, 0, 0, 0], 1),                                      # the first token: frame 0 may be its B
             _small(23, 4, [0, 0, 0, 1], 2, runs=[(1, 3), (0, 4), (1, 4), (2, 8)]),  # the last one, the clip ends inside it: omega at T - 1
             _small(9, 1, [1], 3, runs=[(2, 7)]),                                 # the only token, to the clip's end
             _small(9, 1, [1], 4, runs=[(2, 4)]),                                 # the only token, a gap behind it
             _small(1, 1, [1], 5)]                                                # one frame
    got = _run(clips, 0.7)
    _check_case("first, last, alone", clips, 0.7, got)
    assert all(g["status"] == 0 for g in got)
    assert got[1]["tok"][-1] == 3 and got[2]["tok"][-1] == 0


def test_as_many_frames_as_tokens_and_fewer():
    """T == N: one path, every posterior 1 and every moment 0.  T < N: status 1 and zeros, beside healthy clips."""
    exact = _small(7, 7, [0, 1, 0, 0, 1, 0, 0], 11)
    rng = np.random.default_rng(12)
    few = (rng.standard_normal((3, C)).astype(np.float32), _alts(5, rng), np.array([0, 1, 0, 0, 0], np.int32))
    healthy = _small(40, 6, [0, 1, 0, 1, 0, 0], 13)
    clips = [healthy, exact, few]
    got = _run(clips, 0.7)
    _check_case("T == N and T < N", clips, 0.7, got)
    assert [g["status"] for g in got] == [0, 0, 1] and _zeros(got[2])
    assert np.abs(got[1]["tok_post"] - 1).max() < 1e-5 and not got[1]["end_mean"].any() and not got[1]["start_mean"].any()


@pytest.mark.parametrize("phi", [0.0, 0.7, 50.0])
def test_the_penalty(phi):
    clips = [_planted_clip(140, 31)[0], _small(50, 9, [0, 1, 1, 0, 1, 0, 0, 1, 0], 32), _small(20, 12, [1, 0] * 6, 33, margin=1.0)]
    got = _run(clips, phi)
    _check_case(f"penalty {phi}", clips, phi, got)
    assert all(g["status"] == 0 for g in got)


def test_logz_falls_with_the_penalty():
    clip = _small(50, 9, [0, 1, 1, 0, 1, 0, 0, 1, 0], 32)
    lo, hi = _run([clip], 0.5)[0], _run([clip], 2.0)[0]
    assert lo["status"] == hi["status"] == 0 and lo["logz"][0] > hi["logz"][0]


# ------------------------------------------------------------------------------------------------------------------------ windows
def test_windows_and_an_empty_window_on_a_filler():
    a = _small(40, 6, [0, 1, 0, 1, 0, 0], 61)
    b = _small(40, 6, [0, 1, 0, 1, 0, 0], 62)
    free = _run([a], 0.7)[0]["tok"]
    s1, s3 = (int(np.nonzero(free == k)[0][0]) for k in (1, 3))
    wins = [[OPEN, (max(s1 - 2, 0), s1 + 1), (0, 30), (s3 + 1, s3 + 6), OPEN, OPEN], [OPEN, (5, 4), OPEN, OPEN, OPEN, OPEN]]
    got = _run([a, b], 0.7, windows=wins)
    _check_case("windows", [a, b], 0.7, got, windows=wins)
    assert got[0]["status"] == 0
    assert got[1]["status"] == 1 and _zeros(got[1]) and got[1]["logz"][0] == 0 and not np.isnan(got[1]["logz"][0])


# ------------------------------------------------------------------------------------------------------------------- all flags 0
def test_with_every_flag_0_the_outputs_are_wfl_align_posteriors():
    made = [_planted_clip(N, 50 + N)[0] for N in (90, 280)]
    clips = [(z, _alts(len(a), np.random.default_rng(len(a))), np.zeros(len(a), np.int32)) for z, a, _ in made]
    wins = [[OPEN] * len(a) for _, a, _ in clips]
    for k in range(0, 90, 7):
        wins[0][k] = (max(0, int(1.3 * k) - 25), int(1.3 * k) + 60)
    for name, w in (("flags 0", None), ("flags 0, windows", wins)):
        got = _run(clips, 1.3, windows=w)
        _check_case(name, clips, 1.3, got, windows=w)
        T = [len(c[0]) for c in clips]
        lg = torch.from_numpy(np.ascontiguousarray(np.concatenate([c[0] for c in clips]))).cuda()
        args = (lg, T, [c[1] for c in clips], [GAPS] * len(clips), O_ID)
        packed = AL.pack_clips(*args[:4], windows=w)
        _, tok, _, _ = AL.viterbi_align(*args, packed=packed)
        plain = [x.cpu().numpy() for x in AL.alignment_posteriors(*args, tok, packed=packed)]
        k0, same = 0, True
        for b, g in enumerate(got):
            n = len(clips[b][1])
            assert (g["tok"] == tok.cpu().numpy()[sum(T[:b]):sum(T[:b + 1])]).all() and plain[4][b] == 0
            theirs = dict(logz=plain[0][b:b + 1], tok_post=plain[1][k0:k0 + n], start_mean=plain[2][k0:k0 + n], start_sd=plain[3][k0:k0 + n])
            same &= all((theirs[k] == g[k]).all() for k in theirs)
            k0 += n
            # wfl_align_posterior's outputs meet the same yardstick against the same float64 reference
            _check_case(f"{name}: wfl_align_posterior's own, clip {b}", [clips[b]], 1.3,
                        [dict(theirs, status=0, vstatus=0, tok=g["tok"], end_sd=g["end_sd"])], windows=[w[b]] if w else None,
                        keys=tuple(theirs))
        print(f"{name}: bit-identical to wfl_align_posterior{'_windowed' if w else ''}: {same}")


# ------------------------------------------------------------------------------------------------------------------------- status
def test_a_flag_of_2_is_status_4():
    a = _small(40, 6, [0, 1, 0, 1, 0, 0], 81)
    b = _small(40, 6, [0, 1, 0, 1, 0, 0], 82)
    b = (b[0], b[1], np.array([0, 2, 0, 1, 0, 0], np.int32))
    got = _run([a, b], 0.7)
    assert got[0]["status"] == 0 and got[1]["status"] == 4 and _zeros(got[1])


def test_a_tok_with_a_token_erased_is_status_8_beside_a_healthy_clip():
    healthy = _small(40, 6, [0, 1, 0, 1, 0, 0], 71)
    victim = _small(44, 7, [0, 0, 1, 1, 0, 0, 0], 72)
    T0 = len(healthy[0])

    def erase(tok):
        t = tok.cpu().numpy()
        seg = t[T0:]
        seg[seg == 4] = -1
        return torch.from_numpy(t).cuda()
    solo = _run([healthy], 0.7)[0]
    got = _run([healthy, victim], 0.7, tok_edit=erase)
    assert got[1]["status"] == 8 and _zeros(got[1])
    assert got[0]["status"] == 0
    for k in KEYS:
        assert (solo[k] == got[0][k]).all(), k


def _raw_call(clip, phi, d_fill="own", end_mean="own", ws_short=0):
    """The C entry itself on one clip -> its return value."""
    from wfl_asr_amd import _lib
    from wfl_asr_amd._lib import host_ptr as hp, ptr
    lib = _lib.load()
    z, alts, fill = clip
    lg = torch.from_numpy(z).cuda()
    p = AL.pack_clips(lg, [len(z)], [alts], [GAPS])
    n = len(alts)
    fill_t = torch.from_numpy(np.asarray(fill, np.int32)).cuda()
    tok = torch.full((len(z),), -1, dtype=torch.int32, device="cuda")
    ws_n = AL.filler_posterior_workspace_bytes(p.T, p.N) - ws_short
    ws = torch.empty(max(ws_n, 1), dtype=torch.uint8, device="cuda")
    outs = [torch.zeros(max(n, 1), dtype=torch.float32, device="cuda") for _ in range(7)]
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = lib.wfl_align_filler_posterior(ptr(lg), lg.stride(0), C, O_ID, hp(p.F0), hp(p.T), hp(p.K0), hp(p.N), ptr(p.d_tc), None, ptr(p.d_gc),
                                        1, ptr(fill_t) if d_fill == "own" else None, ctypes.c_float(phi), ptr(tok), ptr(ws), ws_n,
                                        ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]),
                                        ptr(outs[4]) if end_mean == "own" else None, ptr(outs[5]), ptr(st),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def test_host_side_refusals():
    clip = _small(40, 6, [0, 1, 0, 1, 0, 0], 91)
    assert _raw_call(clip, 0.7, d_fill=None) == -1                 # a null tok_fill
    assert _raw_call(clip, 0.7, end_mean=None) == -1               # a null end_mean
    assert _raw_call(clip, float("nan")) == -1
    assert _raw_call(clip, 0.7, ws_short=1) == -1                  # one byte too few: refused on the host, nothing is launched
    assert _raw_call(clip, 0.7) == 0                               # (a tok of -1 alone: status 8, but the call itself is fine)


def test_the_workspace_is_wfl_align_posteriors_and_a_float_per_frame():
    T, N = [200, 50, 700, 0], [100, 20, 600, 5]
    extra = sum((t + 63) // 64 * 64 * 4 for t in T)
    assert AL.filler_posterior_workspace_bytes(T, N) == AL.posterior_workspace_bytes(T, N) + extra


# ---------------------------------------------------------------------------------------------------------------- alone = in a batch
def test_a_clip_alone_equals_the_clip_in_a_ragged_batch_of_16():
    rng = np.random.default_rng(5)
    clips = []
    for b in range(16):
        N = int(rng.integers(1, 150)) if b != 11 else 300
        clips.append(_planted_clip(max(N, 12), 100 + b)[0] if N >= 12 else _small(N + 9, N, rng.random(N) < 0.4, 100 + b))
    got = _run(clips, 0.7)
    for b in (0, 5, 11, 15):
        solo = _run([clips[b]], 0.7)[0]
        assert solo["status"] == got[b]["status"] == 0
        for k in KEYS:
            assert (solo[k] == got[b][k]).all(), (b, k)


# ------------------------------------------------------------------------------------------------------------------------ C = 1024
def test_1024_classes_one_row_per_stage():
    """C = 1024: a stage of the logits ring holds one frame (F = 1), so every frame crosses a stage boundary."""
    rng = np.random.default_rng(7)
    fill = np.array([0, 1, 0, 0, 1, 0], np.int32)
    alts = _alts(6, rng, fill)
    z, _ = R.plant(45, 6, 1024, alts, GAPS, rng, fill=fill, margin=2.0, scale=1.5)
    lg = torch.from_numpy(z).cuda()
    args = (lg, [45], [alts], [GAPS], O_ID, [fill])
    _, tok, _, vst = AL.viterbi_align_filler(*args, 0.7)
    out = [x.cpu().numpy() for x in AL.filler_posteriors(*args, tok, 0.7)]
    g = dict(zip(KEYS, [out[0][:1]] + out[1:6]), status=int(out[6][0]), vstatus=int(vst.cpu()[0]), tok=tok.cpu().numpy())
    assert g["status"] == 0
    _check_case("C = 1024", [(z, alts, fill)], 0.7, [g])
