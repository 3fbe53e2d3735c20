"""-m gpu: the kernels that turn samples into the first activation, each alone against the float64 references of tests/ops_ref.py on the
fp32 values the kernel reads: the Whisper log-mel (csrc/logmel.hip through wfl_logmel) and WavLM's level 0 (csrc/wavlm.hip through
wfl_op_wav_stats, wfl_op_conv0, wfl_op_clip_frames).  The inputs come from ops_ref's seeded functions, so the CPU controls of
tests/test_ops_ref_cpu.py (a wrong reference violates each case's bound) speak about exactly these cases.

Every valid output element is compared.  Whatever must not be written is pre-filled with a sentinel (bf16 7.0; NaN in fp32 and float64
buffers, -77 in int32 ones) and compared bit for bit afterwards; whatever must not be read holds NaN.

What "the same log-mel" means: |out - logmel_ref| <= ops_ref.logmel_bound, element by element -- the worst case of a 200-term fp32 fma
chain over fp32 tables (gamma = 204 * 2^-24 of the windowed frame's L1 norm) carried through the power, the mel sum, log10, the floor
and the affine.  An element whose bound is wider than 1e-2 says nothing; on broadband input at most 1 % of them may be such.

Measured on MI355X (the parity_stats.jsonl that _note writes: notes logmel_* / conv0_* / wav_stats_*).  Log-mel, the largest over the five batch
shapes: max |err|, max err / bound, share of elements with a bound wider than 1e-2:

  n_mels x frames   noise                    DC + noise               impulses                 tone                     silence
  80 x 32           2.4e-7  0.500  0         3.8e-5  0.024  0.12 %    1.2e-7  0.037  0         2.5e-5  0.032  60.9 %    2.4e-7  0.500  0
  80 x 200          6.4e-7  0.500  0         3.8e-5  0.024  0.08 %    1.2e-7  0.037  0         4.4e-5  0.032  65.4 %    2.4e-7  0.500  0
  128 x 32          4.5e-6  0.500  0.05 %    4.8e-5  0.019  0.51 %    1.2e-7  0.037  0         4.1e-5  0.033  47.9 %    2.4e-7  0.500  0
  128 x 200         4.5e-6  0.500  0.01 %    6.9e-5  0.019  0.66 %    1.2e-7  0.037  0         7.4e-5  0.037  52.0 %    2.4e-7  0.500  0

(0.500 is one fp32 unit, 2^-22, of a value at the floor against the store's 4 * 2^-23; away from the floor no element uses more than
0.04 of its bound -- the worst case of 200 roundings all one way is far from what a chain does on real input, as for torch's own fp32
path, which sits at <= 0.12.  The tone clip is there for its dynamic range and carries no informative-share condition.)

conv0, max err / bound per case (hi alone: the bf16 store, 2^-8 |ref|, is nearly all of it by itself; hi + lo: 2^-15 |ref| + lambda * scale):

  group  C 8    T0 1 0.57 (hi)   T0 3 0.14   T0 513 0.98 (hi)   T0 1030 0.20
         C 32   T0 3 0.19   T0 511 0.97 (hi)   T0 512 0.21   T0 513 0.20   T0 1030 0.21
         C 512  T0 1 0.21   T0 512 0.99 (hi, a bias passed and not read)   T0 513 0.21   T0 1030 0.99 (hi)
  layer  C 8    T0 1 0.94 (hi)   T0 3 0.13   T0 513 0.21
         C 32   T0 3 0.19   T0 511 0.22   T0 512 0.99 (hi)   T0 1030 0.99 (hi)   T0 8200 0.22 and 0.99 (hi)
         C 512  T0 1 0.20   T0 3 0.98 (hi)   T0 513 0.99 (hi)   T0 1030 0.22

  max err / scale over the hi + lo cases: 7.2e-7 .. 4.4e-6, most of it the pair's own 2^-15 |ref|.  ops_ref.CONV0_LAMBDA = 2.09e-6 is
  4 x the CPU restatement's 5.2229e-7 (group, C 512, one frame) and is not fitted to any of these.  Beyond the store's own share
  (2^-8 or 2^-15 of |ref|) the kernel's error reaches 6.5e-8 of the scale at most (layer, C 512, one frame; note arith_over_scale_max).

wav_stats: the sums are exact on every case; the sums of squares within 1.4e-14 (L <= 1025) and 2.7e-12 (L = 70001) of the exactly
rounded ones, against bounds of 1.5e-11 and 6.8e-8.
"""
import functools

import pytest
import torch

import gpu_util as G
import ops_ref as R
from cases import tiny_whisper_config
from test_gpu_model import _build, _note

pytestmark = pytest.mark.gpu

SENT = 7.0
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _all_nan_sentinel(t):
    """Every element still holds the very NaN it was filled with."""
    return bool((_bits(t) == _bits(torch.full_like(t[:1], NAN))).all())


# ------------------------------------------------------------------------------------------------------------ Whisper log-mel
@functools.lru_cache(maxsize=None)
def _whisper(n_mels, max_positions):
    cfg = tiny_whisper_config(enable_bilstm=False)
    cfg["model"]["encoder_arch"].update(n_mels=n_mels, max_positions=max_positions)
    return _build(cfg, 5, seed=3)[0]


def _logmel(m, wav, L, lens=None, check=True):
    """wfl_logmel on a device batch wav [B, ldw] of which L samples per row count.  -> (status, out [B, n_mels, frames] fp32, guard)."""
    B, ldw = wav.shape
    n_mels, nf = m.arch.n_mels, 2 * m.arch.max_positions
    flat = torch.full((B * n_mels * nf + 64,), NAN, device="cuda")
    ws = m._workspace(B, L, wav.device)
    lens_d = G._i32(lens)
    rc = G.lib().wfl_logmel(m._handle, G.ptr(wav), ldw, G.ptr(lens_d), B, L, G.ptr(flat), G.ptr(ws), ws.numel(), G.stream())
    if check:
        G._lib.check(rc, "wfl_logmel")
    torch.cuda.synchronize()
    return rc, flat[:B * n_mels * nf].view(B, n_mels, nf), flat[B * n_mels * nf:]


@functools.lru_cache(maxsize=None)
def _logmel_ref(n_mels, max_positions, shape):
    n = 2 * max_positions * 160
    wav, L, lens, kinds = R.logmel_case(n, shape)
    r = R.logmel_ref(wav[:, :L], lens, n_mels, n)
    return wav, L, lens, kinds, r["out"], R.logmel_bound(r)


@pytest.mark.parametrize("shape", R.LOGMEL_SHAPES)
@pytest.mark.parametrize("n_mels,max_positions", R.LOGMEL_MODELS)
def test_logmel_against_float64(n_mels, max_positions, shape):
    """Five clips (noise, DC + noise, edge impulses, a tone, silence) per batch; 32 frames: one workgroup that sees both reflections, 200
    frames: a partial last workgroup.  Shapes: L == n_samples; 777 samples of 50.0 behind n_samples (cut before the reflection); L = 5000
    (zero padded); a row pitch of L + 13 with NaN in the padding; lens = [n_samples, 5000, 201, 200, 1, 0] with NaN behind each length."""
    m = _whisper(n_mels, max_positions)
    wav, L, lens, kinds, ref, bound = _logmel_ref(n_mels, max_positions, shape)
    dev = wav.cuda()
    _, got_d, guard = _logmel(m, dev, L, lens)
    _, again, _ = _logmel(m, dev, L, lens)
    assert _all_nan_sentinel(guard)
    assert torch.equal(_bits(got_d), _bits(again)), "two runs differ"
    got = got_d.double().cpu()
    assert bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    for b, kind in enumerate(kinds):
        wide = float((bound[b] > R.LOGMEL_UNINFORMATIVE).double().mean())
        _note(f"logmel_m{n_mels}_f{ref.shape[2]}_{shape}_{b}_{kind}", err_max=err[b].max(), err_over_bound_max=(err[b] / bound[b]).max(),
              uninformative=wide)
        if kind in R.LOGMEL_BROADBAND:
            assert wide <= 0.01, (kind, wide)
    over = err > bound
    assert not bool(over.any()), f"{int(over.sum())} of {over.numel()} elements beyond the bound; worst err / bound " \
                                 f"{float((err / bound).max()):.3f} (err {float(err.max()):.3e}); clips {sorted(set(over.nonzero()[:, 0].tolist()))}"
    for b, kind in enumerate(kinds):
        if kind == "silence" or (lens is not None and lens[b] == 0):
            assert float((got[b] + 1.5).abs().max()) <= 1e-6
    if lens is not None:                                                    # a ragged batch is explicit zero padding, bit for bit
        padded = wav.clone()
        for b, k in enumerate(lens):
            padded[b, k:] = 0.0
        _, want, _ = _logmel(m, padded.cuda(), L, None)
        assert torch.equal(_bits(got_d), _bits(want))


def test_logmel_rejects_null_pointers_and_an_empty_row():
    """wfl_logmel with L == 0 used to reach the kernel, whose staging loads clamp their index to L - 1 = -1.  Status and message only:
    the host check comes before anything is launched."""
    m = _whisper(80, 16)
    wav = torch.zeros(2, 64, device="cuda")
    out = torch.full((2 * 80 * 32,), NAN, device="cuda")
    ws = m._workspace(2, 64, wav.device)
    lib = G.lib()
    for w, o, L in ((wav, out, 0), (None, out, 64), (wav, None, 64), (wav, out, -1)):
        rc = lib.wfl_logmel(m._handle, G.ptr(w), 64, G.ptr(None), 2, L, G.ptr(o), G.ptr(ws), ws.numel(), G.stream())
        assert rc != 0 and b"wfl_logmel" in lib.wfl_last_error(), (L, lib.wfl_last_error())
    torch.cuda.synchronize()
    assert _all_nan_sentinel(out)


# --------------------------------------------------------------------------------------------------------------- WavLM conv0
def _conv0_launch(c, wav, lens, B, L, T0):
    """One wfl_op_conv0 launch (after wfl_op_wav_stats where the case normalises) on sentinel-filled rows.  -> (hi rows, lo rows or None)."""
    Cn, group = c["C"], c["mode"] == "group"
    wav_d, lens_d = wav.cuda().contiguous(), G._i32(lens)
    wstats = None
    if c["normalize"]:
        wstats = torch.full((2 * B,), NAN, dtype=torch.float64, device="cuda")
        G.wav_stats(wav_d, wav_d.shape[1], B, L, wstats, lens_d)
    hi = G.Rows(B, T0, Cn).set(torch.full((B, T0, Cn), SENT))
    lo = G.Rows(B, T0, Cn).set(torch.full((B, T0, Cn), SENT)) if c["pair"] else None
    scratch = torch.empty(G.conv0_scratch_bytes(B, T0, Cn), dtype=torch.uint8, device="cuda") if group else None
    G.conv0(wav_d, wav_d.shape[1], B, L, c["w"].cuda().contiguous(), c["gamma"].cuda(), c["beta"].cuda(), Cn, T0, hi.buf, hi.lead, hi.P,
            group, lens=lens_d, wstats=wstats, bias=c["bias"].cuda() if c["bias"] is not None else None, out_lo=lo.buf if lo else None,
            scratch=scratch)
    torch.cuda.synchronize()
    return hi, lo


@functools.lru_cache(maxsize=None)
def _conv0_case(case):
    c = R.conv0_inputs(case)
    ref, scale = R.conv0_case_ref(c)
    return c, ref, scale, R.conv0_valid(c)


@pytest.mark.parametrize("case", R.CONV0_CASES, ids=R.conv0_id)
def test_conv0_against_float64(case):
    """conv (k = 10, stride 5) + GroupNorm over the clip's frames or LayerNorm over the channels + GELU, B = 3 with one silent clip, one
    all-positive, one all-zero and one low-variance channel.  T0 around the 512-frame block edge, C = 512, 8200 frames for the layer
    kernel's grid-stride loop; ragged: lens = [L, 1008, 9] with NaN behind each length -- the last clip has no frame and its rows stay
    untouched.  Valid rows within conv0_bound; the rest holds the sentinel; a ragged clip equals the clip run alone and two runs equal
    each other bit for bit (no atomics anywhere)."""
    c, ref, scale, m = _conv0_case(case)
    B, L, T0, pair = 3, c["L"], c["T0"], c["pair"]
    hi, lo = _conv0_launch(c, c["wav"], c["lens"], B, L, T0)
    hi2, lo2 = _conv0_launch(c, c["wav"], c["lens"], B, L, T0)
    assert torch.equal(hi.buf, hi2.buf) and (not pair or torch.equal(lo.buf, lo2.buf)), "two runs differ"
    got = hi.get().double().cpu() + (lo.get().double().cpu() if pair else 0.0)
    bound = R.conv0_bound(ref, scale, pair)
    err = (got - ref).abs()
    store = (2.0 ** -15 if pair else 2.0 ** -8) * ref.abs()                  # (arith: what is left beyond the store's share, over the scale)
    _note("conv0_" + R.conv0_id(case), err_over_scale_max=(err / scale)[m].max(), arith_over_scale_max=((err - store) / scale)[m].max(),
          err_over_bound_max=(err / bound)[m].max(), err_max=err[m].max(), lambda_cpu_measured=R.CONV0_LAMBDA_MEASURED, lambda_used=R.CONV0_LAMBDA)
    over = (err > bound) & m[..., None]
    assert not bool(over.any()), f"{int(over.sum())} of {int(m.sum()) * c['C']} elements beyond the bound; worst err / bound " \
                                 f"{float((err / bound)[m].max()):.3f}, err / scale {float((err / scale)[m].max()):.3e}"
    for r in (hi, lo) if pair else (hi,):
        assert r.halo_is_zero() and bool((r.get().cpu()[~m] == SENT).all()), "a row beyond a clip's own frames was written"
    if c["lens"] is not None:                                               # the shorter clip alone: its own batch of one
        n = c["lens"][1]
        T1 = R.conv0_frames(n)
        a_hi, a_lo = _conv0_launch(c, c["wav"][1:2, :n], None, 1, n, T1)
        assert torch.equal(a_hi.get()[0], hi.get()[1, :T1]) and (not pair or torch.equal(a_lo.get()[0], lo.get()[1, :T1]))


def test_conv0_argument_errors_launch_nothing():
    """Null pointers, C % 8, C > 512, T0 <= 0 or beyond what L holds, group mode without enough scratch: a status, wfl_last_error naming
    the entry point, and rows that still hold the sentinel."""
    B, L, T0, Cn = 2, 5 * 19 + 10, 20, 16
    wav = torch.zeros(B, L, device="cuda")
    w, v = torch.zeros(520, 10, device="cuda"), torch.zeros(520, device="cuda")
    out = G.Rows(B, T0, 520).set(torch.full((B, T0, 520), SENT))
    scratch = torch.empty(G.conv0_scratch_bytes(B, T0, 512), dtype=torch.uint8, device="cuda")
    assert G.conv0_scratch_bytes(B, T0, Cn) == B * Cn * 16 + B * 1 * Cn * 8 and G.conv0_scratch_bytes(1, 513, 8) == 8 * 16 + 2 * 8 * 8
    ok = dict(wav=wav, ldw=L, B=B, L=L, w=w, gamma=v, beta=v, Cn=Cn, T0=T0, out=out.buf, lead=out.lead, P=out.P, group_norm=1, scratch=scratch)
    bad = [dict(wav=None), dict(w=None), dict(gamma=None), dict(beta=None), dict(out=None), dict(Cn=12), dict(Cn=520), dict(Cn=0), dict(T0=0),
           dict(T0=-1), dict(T0=T0 + 1), dict(P=T0 - 1), dict(ldw=L - 1), dict(scratch=None), dict(scratch_bytes=G.conv0_scratch_bytes(B, T0, Cn) - 1),
           dict(group_norm=0, Cn=12), dict(group_norm=0, T0=0)]
    for over in bad:
        rc = G.conv0(**{**ok, **over}, check=False)
        assert rc != 0 and b"wfl_op_conv0" in G.lib().wfl_last_error(), over
    torch.cuda.synchronize()
    assert bool((out.get() == SENT).all()) and out.halo_is_zero()


# ----------------------------------------------------------------------------------------------------------------- wav_stats
@pytest.mark.parametrize("L", R.WAV_STATS_L)
def test_wav_stats_against_exact_sums(L):
    """One workgroup of 1024 threads per clip: L below, at and above one pass, and 70001 samples; lens = [L, (L + 1) / 2, 0, 1] with NaN
    behind each length and in the row padding; float64 sums within L 2^-53 of the sums of magnitudes; an empty clip gives (0, 0)."""
    wav, lens = R.wav_stats_case(L)
    ref, bound = R.wav_stats_ref(wav, lens)
    dev = wav.cuda()
    runs = []
    for _ in range(2):
        st = torch.full((2 * 4 + 6,), NAN, dtype=torch.float64, device="cuda")
        G.wav_stats(dev, dev.shape[1], 4, L, st, G._i32(lens))
        torch.cuda.synchronize()
        runs.append(st)
    assert torch.equal(_bits(runs[0]), _bits(runs[1])) and _all_nan_sentinel(runs[0][8:])
    got = runs[0][:8].cpu().view(4, 2)
    err = (got - ref).abs()
    _note(f"wav_stats_L{L}", err_sum_max=err[:, 0].max(), err_sq_max=err[:, 1].max(), bound_sum_min=bound[:2, 0].min())
    assert bool((err <= bound).all()), (err, bound)
    assert got[2].tolist() == [0.0, 0.0]
    # without lens every row counts to L
    clean = torch.where(torch.isnan(wav), torch.zeros(()), wav)[:, :L].contiguous()
    ref2, bound2 = R.wav_stats_ref(clean)
    st = torch.full((8,), NAN, dtype=torch.float64, device="cuda")
    G.wav_stats(clean.cuda(), L, 4, L, st)
    torch.cuda.synchronize()
    assert bool(((st.cpu().view(4, 2) - ref2).abs() <= bound2).all())


# --------------------------------------------------------------------------------------------------------------- clip_frames
@pytest.mark.parametrize("rule", ["wavlm", "mel"])
def test_clip_frames_is_the_integer_formula(rule):
    """300 clips (two blocks of 256), among them lens -3, 0, 9, 10, 200, 201, 399, 400, 401, L and L + 5: the WavLM stack's seven levels,
    and the mel rule (kernel 0, stride 160, nothing below 201 samples)."""
    kernel, stride, min_len = (*R.WAVLM_STACK, 0) if rule == "wavlm" else ((0,), (160,), 201)
    lens, B, L, n = R.clip_frames_lens(), R.CLIP_FRAMES_B, R.CLIP_FRAMES_L, len(kernel)
    out = torch.full((n * B + 32,), -77, dtype=torch.int32, device="cuda")
    G.clip_frames(G._i32(lens), B, L, list(kernel), list(stride), min_len, out)
    torch.cuda.synchronize()
    assert out[:n * B].cpu().view(n, B).tolist() == R.clip_frames_ref(lens, L, kernel, stride, min_len)
    assert bool((out[n * B:] == -77).all())


def test_clip_frames_and_wav_stats_argument_errors_launch_nothing():
    lens = G._i32([100, 200])
    out = torch.full((16,), -77, dtype=torch.int32, device="cuda")
    lib = G.lib()
    for kernel, stride, n, o, ln in (([10], [5], 0, out, lens), ([10] * 9, [5] * 9, 9, out, lens), ([10], [0], 1, out, lens),
                                     ([10], [5], 1, None, lens), ([10], [5], 1, out, None)):
        rc = G.clip_frames(ln, 2, 1000, kernel, stride, 0, o, n=n, check=False)
        assert rc != 0 and b"wfl_op_clip_frames" in lib.wfl_last_error(), (kernel, stride, n)
    wav = torch.zeros(2, 64, device="cuda")
    st = torch.full((4,), NAN, dtype=torch.float64, device="cuda")
    for w, s, L, ldw in ((None, st, 64, 64), (wav, None, 64, 64), (wav, st, 0, 64), (wav, st, 64, 63)):
        rc = G.wav_stats(w, ldw, 2, L, s, check=False)
        assert rc != 0 and b"wfl_op_wav_stats" in lib.wfl_last_error(), (L, ldw)
    torch.cuda.synchronize()
    assert bool((out == -77).all()) and _all_nan_sentinel(st)
