"""-m gpu: wfl_align_optional_posterior (csrc/align_optional_posterior.hip) against the float64 forward-backward over the skip lattice
of tests/optional_posterior_ref.py.  `tok` is what wfl_align_optional returned for the same clips, flags and penalty.

Tolerances are the rule of tests/test_gpu_align_posterior.py, restated here for the five outputs: for every case the float32
restatement of the reference (same renormalisation period as the kernel) is run on the same inputs; its maximum deviation from
float64 over the case, per output, is the yardstick, and the kernel is allowed 4 x that against float64; where the yardstick is below
half an fp32 ulp of the value itself, that half ulp is added (the outputs are fp32).  Every clip and token of every case is compared.
The one bit-for-bit assertion on new outputs is "a clip alone equals the clip in a batch": same kernel, same arithmetic."""
import ctypes

import numpy as np
import pytest
import torch

import optional_posterior_ref as OP
import viterbi_optional_ref as R
from wfl_asr_amd import align as AL

pytestmark = pytest.mark.gpu
C = 141
O_ID = 0
GAPS = [O_ID, 137, 138]
KEYS = ("logz", "keep_post", "tok_post", "start_mean", "start_sd")
SLOTS = ((127, 2), (511, 2), (1023, 4), (2047, 8), (4096, 9))          # csrc/lattice.h: token cap of a configuration, its R


def _slots(N):
    return next(r for cap, r in SLOTS if N <= cap)


def _alts(N, rng):
    """Random phonemes, none equal to either of the two before it."""
    ph = []
    for k in range(N):
        while True:
            p = int(rng.integers(1, 68))
            if p not in ph[-2:]:
                break
        ph.append(p)
    return [[(2 * p - 1, 2 * p)] for p in ph]


def _run(clips, lam, windows=None, tok_edit=None, post_windows="same"):
    """clips: list of (z [T, C] float32, alternatives, flags) -> per clip a dict of the search's tok / status and the entry's outputs."""
    T = [len(c[0]) for c in clips]
    lg = torch.from_numpy(np.ascontiguousarray(np.concatenate([c[0] for c in clips]))).cuda()
    args = (lg, T, [c[1] for c in clips], [GAPS] * len(clips), O_ID, [c[2] for c in clips])
    _, tok, _, vst, skipped = AL.viterbi_align_optional(*args, lam, windows=windows)
    if tok_edit is not None:
        tok = tok_edit(tok.clone())
    out = AL.optional_posteriors(*args, tok, lam, windows=windows if post_windows == "same" else post_windows)
    torch.cuda.synchronize()
    tok, vst, skipped = (x.cpu().numpy() for x in (tok, vst, skipped))
    logz, keep, tp, mu, sd, st = (x.cpu().numpy() for x in out)
    res, pos, k0 = [], 0, 0
    for b, t in enumerate(T):
        n = len(clips[b][1])
        res.append(dict(tok=tok[pos:pos + t], vstatus=int(vst[b]), skipped=skipped[k0:k0 + n], logz=np.array([logz[b]], np.float32),
                        keep_post=keep[k0:k0 + n], tok_post=tp[k0:k0 + n], start_mean=mu[k0:k0 + n], start_sd=sd[k0:k0 + n],
                        status=int(st[b])))
        pos += t
        k0 += n
    return res


def _zeros(g):
    return g["logz"][0] == 0 and not any(g[k].any() for k in KEYS[1:])


def _half_ulp(ref):
    return 0.5 * np.spacing(np.abs(np.asarray(ref, np.float64)).astype(np.float32)).astype(np.float64)


REFS = {}                                   # a reference is computed once per (case, clip) and left unchanged


def _refs(key, z, alts, opt, lam, tok, win):
    if key not in REFS:
        REFS[key] = (OP.forward_backward(z, alts, GAPS, opt, lam, tok=tok, windows=win),
                     OP.forward_backward(z, alts, GAPS, opt, lam, tok=tok, windows=win, dtype=np.float32))
    return REFS[key]


def _check_case(name, clips, lam, got, windows=None, keys=KEYS):
    """Every clip of a case against float64, by the 4 x yardstick rule; prints the figures before it asserts."""
    yard = {k: 0.0 for k in keys}
    refs = []
    for b, ((z, alts, opt), g) in enumerate(zip(clips, got)):
        win = windows[b] if windows is not None else None
        assert g["status"] == g["vstatus"], (name, b, g["status"], g["vstatus"])
        if g["status"] != 0:
            assert _zeros(g)
            if g["status"] == 1:
                assert OP.forward_backward(z, alts, GAPS, opt, lam, windows=win) is None
            refs.append(None)
            continue
        r64, r32 = _refs((name, b, lam), z, alts, opt, lam, g["tok"], win)
        assert r64 is not None, (name, b)
        assert (g["keep_post"] >= 0).all() and (g["keep_post"] <= 1).all()
        assert (g["tok_post"] >= 0).all() and (g["tok_post"] <= 1).all() and (g["start_sd"] >= 0).all()
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
    """Slots R - 1, 0 and 1 of a thread, and the first token of the second wave: where alpha reads the left thread's five values and
    beta the right thread's slots 0 and 1.  Never two in a row."""
    return [k for k in (10 * R_ - 1, 13 * R_, 17 * R_ + 1, 64 * R_) if 0 < k < N - 1]


def _planted_clip(N, seed, skip_boundary, stretch=1.3):
    """T about 1.3 N + 37 (several 128-frame blocks, no multiple of 16), a third of the tokens optional, the boundary tokens among
    them: skipped or kept by the planted path as asked, every third other optional token skipped where its neighbours are kept."""
    rng = np.random.default_rng(seed)
    R_ = _slots(N)
    T = int(stretch * N) + 37
    T += T % 16 == 0
    opt = rng.random(N) < 0.33
    bnd = _boundary_tokens(N, R_)
    opt[bnd] = True
    skipped = set(bnd) if skip_boundary else set()
    for j, k in enumerate(np.nonzero(opt)[0]):
        k = int(k)
        if k not in bnd and j % 3 == 0 and not ({k - 1, k + 1} & skipped) and not ({k - 1, k, k + 1} & set(bnd)):
            skipped.add(k)
    alts = _alts(N, rng)
    z, _ = R.plant(T, N, C, alts, GAPS, rng, skipped=sorted(skipped), margin=3.0, scale=1.5)
    return (z, alts, opt.astype(np.int32)), sorted(skipped), bnd


CONFIG_N = (100, 300, 700, 1500, 2500)


def test_one_shape_per_launch_configuration():
    made = [_planted_clip(N, N, True) for N in CONFIG_N]
    clips = [m[0] for m in made]
    got = _run(clips, 0.7)
    _check_case("configurations", clips, 0.7, got)
    for (clip, skipped, _), g in zip(made, got):
        assert g["status"] == 0
        assert g["skipped"].any() and (g["skipped"][clip[2] == 1] == 0).any()        # some optional tokens skipped, some kept
        assert (g["tok_post"][g["skipped"] == 1] == 0).all()


@pytest.mark.parametrize("N", [140, 530, 1030, 2050])
def test_skip_arcs_across_ownership_boundaries(N):
    """The tokens in slots R - 1, 0, 1 of a thread and at k = 64 R, planted once skipped and once kept (R = 2, 4, 8, 9): the smallest
    transcripts of the configurations 256 x 2, 256 x 4, 256 x 8 and 512 x 9 that hold token 64 R, over a few more frames than tokens
    (the float64 reference of two such clips is what the test's time goes to)."""
    made = [_planted_clip(N, 7 * N + s, bool(s), stretch=1.06) for s in (1, 0)]
    clips = [m[0] for m in made]
    got = _run(clips, 0.0)
    refs = _check_case(f"boundaries N={N}", clips, 0.0, got)
    bnd = made[0][2]
    assert len(bnd) == 4 and set(bnd) <= set(made[0][1]) and not set(bnd) & set(made[1][1])
    # (the plants are soft, margin 3 a frame, so that the posteriors spread over [0, 1]: what the kernel makes of them is judged
    # through the reference alone)
    assert all(r is not None for r in refs)


# ------------------------------------------------------------------------------------------------------------------ start and end
def _small(T, N, opt, seed, skipped=(), margin=2.0):
    rng = np.random.default_rng(seed)
    alts = _alts(N, rng)
    z, _ = R.plant(T, N, C, alts, GAPS, rng, skipped=skipped, margin=margin, scale=1.5)
    return z, alts, np.asarray(opt, np.int32)


def test_start_and_end():
    clips = [_small(23, 4, [1, 0, 0, 0], 1, skipped=[0]),          # opt[0] skipped: frame 0 may be B_1
             _small(23, 4, [0, 0, 0, 1], 2, skipped=[3]),          # opt[N-1] skipped at the end
             _small(9, 1, [1], 3, skipped=[0]),                    # N = 1 optional: the all-gap path is legal
             _small(9, 1, [1], 4),
             _small(11, 2, [1, 1], 5, skipped=[0]),                # N = 2, both optional
             _small(11, 2, [1, 1], 6, skipped=[1]),
             _small(1, 2, [1, 1], 7, skipped=[0])]                 # one frame: B_0, or B_1 over the skipped token 0, or the gap
    got = _run(clips, 0.7)
    _check_case("start and end", clips, 0.7, got)
    assert all(g["status"] == 0 for g in got)


def test_fewer_frames_than_tokens():
    """N = 5, all optional: T = 3 and T = 2 have paths (the reference is held to the enumeration of every path here), T = 1 has none;
    the feasible clips beside them are unaffected."""
    few = [_small(T, 5, [1] * 5, 10 + T, skipped=[0, 2, 4][:5 - T] if T > 1 else [0, 2, 4], margin=1.0) for T in (3, 2)]
    rng = np.random.default_rng(99)
    none = (rng.standard_normal((1, C)).astype(np.float32), _alts(5, rng), np.ones(5, np.int32))
    healthy = [_small(40, 6, [0, 1, 0, 1, 0, 0], 21, skipped=[1]), _small(33, 3, [0, 0, 0], 22)]
    clips = [healthy[0], few[0], none, few[1], healthy[1]]
    got = _run(clips, 0.7)
    refs = _check_case("fewer frames than tokens", clips, 0.7, got)
    assert [g["status"] for g in got] == [0, 0, 1, 0, 0] and _zeros(got[2])
    for b in (1, 3):
        z, alts, opt = clips[b]
        en = OP.enumerate_paths(z, alts, GAPS, opt, 0.7)
        assert abs(en["logz"] - refs[b]["logz"]) <= 1e-10 and np.abs(en["keep_post"] - refs[b]["sum_gamma_b"]).max() <= 1e-10
    solo = _run([healthy[0]], 0.7)[0]
    for k in KEYS:
        assert (solo[k] == got[0][k]).all(), k


@pytest.mark.parametrize("lam", [0.0, 0.7, 50.0])
def test_the_penalty(lam):
    clips = [_planted_clip(140, 31, True)[0], _small(50, 9, [0, 1, 1, 0, 1, 0, 0, 1, 0], 32, skipped=[2, 7]),
             _small(20, 12, [1, 0] * 6, 33, skipped=[0, 4, 8], margin=1.0)]
    got = _run(clips, lam)
    _check_case(f"penalty {lam}", clips, lam, got)
    assert all(g["status"] == 0 for g in got)


# ------------------------------------------------------------------------------------------------------------------- all flags 0
def test_with_every_flag_0_the_outputs_are_wfl_align_posteriors():
    made = [_planted_clip(N, 50 + N, False)[0] for N in (90, 280)]
    clips = [(z, a, np.zeros(len(a), np.int32)) for z, a, _ in made]
    wins = [[(0, 2 ** 31 - 1)] * len(a) for _, a, _ in clips]
    for k in range(0, 90, 7):
        wins[0][k] = (max(0, int(1.3 * k) - 25), int(1.3 * k) + 60)
    for name, w in (("flags 0", None), ("flags 0, windows", wins)):
        got = _run(clips, 1.3, windows=w)
        refs = _check_case(name, clips, 1.3, got, windows=w)
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
            theirs = dict(logz=plain[0][b:b + 1], tok_post=plain[1][k0:k0 + n], start_mean=plain[2][k0:k0 + n], start_sd=plain[3][k0:k0 + n],
                          keep_post=np.ones(n, np.float32))
            same &= all((theirs[k] == g[k]).all() for k in KEYS)
            k0 += n
            # wfl_align_posterior's outputs meet the same yardstick against the same float64 reference (keep_post: the constant 1)
            _check_case(f"{name}: wfl_align_posterior's own, clip {b}", [clips[b]], 1.3,
                        [dict(theirs, status=0, vstatus=0, tok=g["tok"])], windows=[w[b]] if w else None)
            assert np.abs(refs[b]["keep_post"] - 1).max() < 1e-9
        print(f"{name}: bit-identical to wfl_align_posterior{'_windowed' if w else ''}: {same}")


# ------------------------------------------------------------------------------------------------------------------------ windows
def test_an_empty_window_on_an_optional_token_and_on_a_mandatory_one():
    a = _small(40, 6, [0, 1, 0, 1, 0, 0], 61)
    b = _small(40, 6, [0, 1, 0, 1, 0, 0], 62)
    open_ = (0, 2 ** 31 - 1)
    wins = [[open_, (5, 4), open_, (3, 30), open_, open_], [open_, open_, (9, 2), open_, open_, open_]]
    got = _run([a, b], 0.7, windows=wins)
    _check_case("empty windows", [a, b], 0.7, got, windows=wins)
    assert got[0]["status"] == 0 and got[0]["keep_post"][1] == 0.0 and got[0]["skipped"][1] == 1
    assert got[1]["status"] == 1 and _zeros(got[1])


# ------------------------------------------------------------------------------------------------------------------------- status
def _erase(T0, tok_of):
    def edit(tok):
        t = tok.cpu().numpy()
        seg = t[T0:]
        for k in tok_of:
            seg[seg == k] = -1
        t[T0:] = seg
        return torch.from_numpy(t).cuda()
    return edit


@pytest.mark.parametrize("what", ["a mandatory token erased", "two adjacent optional tokens erased", "a token opened outside its window"])
def test_a_tok_that_is_no_path_is_status_8_beside_a_healthy_clip(what):
    healthy = _small(40, 6, [0, 1, 0, 1, 0, 0], 71, skipped=[1])
    victim = _small(44, 7, [0, 0, 1, 1, 0, 0, 0], 72)
    T0 = len(healthy[0])
    if what == "a token opened outside its window":
        open_ = (0, 2 ** 31 - 1)
        solo = _run([healthy], 0.7, windows=[[open_] * 6])[0]
        first = int(np.nonzero(_run([victim], 0.7)[0]["tok"] == 4)[0][0])
        narrow = [[open_] * 6, [open_] * 4 + [(first + 1, first + 9)] + [open_] * 2]
        got = _run([healthy, victim], 0.7, windows=[[open_] * 6, [open_] * 7], post_windows=narrow)
    else:
        solo = _run([healthy], 0.7)[0]
        got = _run([healthy, victim], 0.7, tok_edit=_erase(T0, [4] if what.startswith("a mandatory") else [2, 3]))
    assert got[1]["status"] == 8 and _zeros(got[1])
    assert got[0]["status"] == 0
    for k in KEYS:
        assert (solo[k] == got[0][k]).all(), k


def test_one_optional_token_erased_is_still_a_path():
    victim = _small(44, 7, [0, 0, 1, 1, 0, 0, 0], 72)
    got = _run([victim], 0.7, tok_edit=_erase(0, [2]))
    assert got[0]["status"] == 0 and got[0]["tok_post"][2] == 0 and 0 < got[0]["keep_post"][2] <= 1


def test_a_flag_of_2_is_status_4():
    a = _small(40, 6, [0, 1, 0, 1, 0, 0], 81)
    b = _small(40, 6, [0, 2, 0, 1, 0, 0], 82)
    got = _run([a, b], 0.7)
    assert got[0]["status"] == 0 and got[1]["status"] == 4 and _zeros(got[1])


def _raw_call(clip, lam, d_opt="own", ws_short=0):
    """The C entry itself on one clip -> its return value."""
    from wfl_asr_amd import _lib
    from wfl_asr_amd._lib import host_ptr as hp, ptr
    lib = _lib.load()
    z, alts, opt = clip
    lg = torch.from_numpy(z).cuda()
    p = AL.pack_clips(lg, [len(z)], [alts], [GAPS])
    n = len(alts)
    opt_t = torch.from_numpy(np.asarray(opt, np.int32)).cuda()
    tok = torch.full((len(z),), -1, dtype=torch.int32, device="cuda")
    ws_n = AL.optional_posterior_workspace_bytes(p.T, p.N) - ws_short
    ws = torch.empty(max(ws_n, 1), dtype=torch.uint8, device="cuda")
    outs = [torch.zeros(max(n, 1), dtype=torch.float32, device="cuda") for _ in range(6)]
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = lib.wfl_align_optional_posterior(ptr(lg), lg.stride(0), C, O_ID, hp(p.F0), hp(p.T), hp(p.K0), hp(p.N), ptr(p.d_tc), None, ptr(p.d_gc),
                                          1, ptr(opt_t) if d_opt == "own" else None, ctypes.c_float(lam), ptr(tok), ptr(ws), ws_n,
                                          ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), ptr(outs[4]), ptr(st),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def test_host_side_refusals():
    clip = _small(40, 6, [0, 1, 0, 1, 0, 0], 91)
    assert _raw_call(clip, 0.7, d_opt=None) == -1                  # a null tok_opt
    assert _raw_call(clip, float("nan")) == -1
    assert _raw_call(clip, -1.0) == -1
    assert _raw_call(clip, 0.7, ws_short=1) == -1                  # one byte too few: refused on the host, nothing is launched
    assert _raw_call(clip, 0.7) == 0                               # (a tok of -1 alone: status 8, but the call itself is fine)


def test_the_workspace_is_wfl_align_posteriors():
    """wfl_align_posterior's workspace rule gives a clip with 0 < T < N its floats already (only T = 0 has none), so the two functions
    agree on every batch; the clip with T < N, which may have a path here, is counted."""
    T, N = [200, 50, 700], [100, 20, 600]
    assert AL.optional_posterior_workspace_bytes(T, N) == AL.posterior_workspace_bytes(T, N)
    T2 = T + [3]
    N2 = N + [5]
    assert AL.optional_posterior_workspace_bytes(T2, N2) == AL.posterior_workspace_bytes(T2, N2)
    assert AL.optional_posterior_workspace_bytes(T2, N2) > AL.optional_posterior_workspace_bytes(T + [0], N2)


# ---------------------------------------------------------------------------------------------------------------- alone = in a batch
def test_a_clip_alone_equals_the_clip_in_a_ragged_batch_of_16():
    rng = np.random.default_rng(5)
    clips = []
    for b in range(16):
        N = int(rng.integers(1, 150)) if b != 11 else 300
        clips.append(_planted_clip(max(N, 12), 100 + b, b % 2 == 0)[0] if N >= 12 else _small(N + 9, N, rng.random(N) < 0.4, 100 + b))
    got = _run(clips, 0.7)
    for b in (0, 5, 11, 15):
        solo = _run([clips[b]], 0.7)[0]
        assert solo["status"] == got[b]["status"] == 0
        for k in KEYS:
            assert (solo[k] == got[b][k]).all(), (b, k)
