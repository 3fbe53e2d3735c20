"""-m gpu: every mode of one GEMM launch (csrc/common.h, GemmArgs) at the operator level, through wfl_op_gemm_ex, against the plain
float64 references of tests/ops_ref.py (checked on the CPU by tests/test_ops_ref_cpu.py).

Conventions of every case
  * operands and outputs live in G.Rows frame-row buffers (lead rows, halos between clips, a tail);
  * every output, low-half, statistics and e4m3 buffer is filled with a sentinel before the launch; whatever must not be written --
    halo rows, rows t >= T or >= clip_T[b], columns >= n_valid, statistics slots >= N / 256 -- is compared with a copy taken before
    the launch (`_untouched`);
  * the kernel that ran (`kernel_id`) is asserted: a case that quietly falls to another kernel tests nothing;
  * the measured max(err / mag) goes to `_note` (parity_stats.jsonl, as in test_gpu_round4.py).

Row counts: "small" = 3 clips of 333 frames (pitch 352, 1056 rows: tiles straddle clips, the last one is partial, only the final
epilogue runs); "walk" = 25 clips of 480 (pitch 496, 12 400 rows: 65 row tiles of 192 -> 260 tiles at N = 1024, 390 at N = 1536 --
more than the 256 persistent workgroups and no multiple of them, so some workgroups run the in-loop epilogue and some do not).

Tolerances (ops_ref.tol_*): a bf16 output carries one rounding, 2^-8 |ref|; a hi + lo pair 2^-15 |ref|; an fp32 accumulation over K
at most K 2^-24 mag; GELU multiplies that by its Lipschitz constant (1.13 -> 1.2); an e4m3 output carries 2^-4 |ref|, floored at the
format's subnormal spacing.  None is fitted to a kernel.

The streaming kernel's 256-row form (kernel id 5) exists only in builds with -DWFL_STREAM_MT8 and WFL_GEMM_BM=256 in the environment
(csrc/gemm_stream.hip, launch_stream_mt): no shape reaches it in the library the tests load, so every streaming case asserts id 1."""
import math

import pytest
import torch
import torch.nn.functional as F

import gpu_util as G
import ops_ref as R
from test_gpu_model import _note
from test_gpu_round4 import _e4m3, _rows_fp8

pytestmark = pytest.mark.gpu

SENT = 77.0                       # exact in bf16 and fp32
SENT8 = 0x55
ROWS = {"small": (3, 333), "walk": (25, 480)}
RAGGED_B, RAGGED_T = 4, 300       # pitch 320; clip 3 starts at row 960 = 5 x 192, so its 200 frames end inside its second row tile
RAGGED = [300, 0, 1, 200]         # T, 0, 1 and a value inside a row tile


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _grid(r):
    """[B, T] buffer rows of the frames of a G.Rows"""
    return (r.lead + torch.arange(r.B)[:, None] * r.P + torch.arange(r.T)[None, :]).cuda()


def _sent_rows(B, T, N):
    r = G.Rows(B, T, N)
    r.buf.fill_(SENT)
    return r


def _untouched(after, before, rows, ncols):
    """everything outside rows x [0, ncols) is what it was before the launch"""
    a, b = after.reshape(after.shape[0], -1), before.reshape(before.shape[0], -1)
    keep = torch.ones(a.shape, dtype=torch.bool, device=a.device)
    keep[rows, :ncols] = False
    return bool((a[keep] == b[keep]).all())


def _launch(x, K, w, N, out, want_kid, **kw):
    """one wfl_op_gemm_ex launch with the frame-row geometry of x (operand) and out (result); asserts the kernel"""
    f = dict(A=(x.buf, x.lead * K), lda=K, W=w, M=x.B * x.P, N=N, K=K, n_valid=N, P=x.P, T=x.T, ldc=N, c_lead=out.lead, c_pitch=out.P,
             alpha=1.0)
    if "c8" not in kw:
        f["C"] = out.buf
    f.update(kw)
    _, kid = G.gemm_ex(**f)
    want = want_kid if isinstance(want_kid, tuple) else (want_kid,)
    assert kid in want, (kid, want)
    return kid


def _w_bf16(g, N, K, scale=None):
    return (torch.randn(N, K, generator=g) * (K ** -0.5 if scale is None else scale)).to(torch.bfloat16).cuda()


def _w_e4m3(g, N, K):
    """bytes over the whole e4m3 range, scales (rand + 0.5) 1e-3: as test_gemm_mx_against_a_float64_product_of_its_own_bytes"""
    w8 = _e4m3(torch.randn(N, K, generator=g).cuda() * 60).view(torch.uint8).contiguous()
    ws = ((torch.rand(N, generator=g) + 0.5) * 1e-3).cuda()
    return w8, ws


def _pair_rows(g, B, T, N, scale=4.0, sentinel=True):
    """a residual stream as a bf16 pair in two sentinel-filled buffers"""
    r0 = torch.randn(B, T, N, generator=g) * scale
    hi, lo = R.split(r0)
    a, b = (_sent_rows(B, T, N), _sent_rows(B, T, N)) if sentinel else (G.Rows(B, T, N), G.Rows(B, T, N))
    return a.set(hi.float().cuda()), b.set(lo.float().cuda())


def _clip_T(clip_T):
    return None if clip_T is None else torch.tensor(clip_T, dtype=torch.int32, device="cuda")


def _check_stats(stats, before, out, idx, N, tag):
    """stats_out against the float64 sums of the bf16 values the kernel stored in C (checked by the caller): a 256-term fp32 summation"""
    ntile = N // 256
    want, scale = R.tile_stats_ref(out.buf[idx].double())
    got = stats[idx][:, :ntile].double()
    err = (got - want).abs()
    bound = 256 * 2.0 ** -24 * scale
    _note(f"gemm_modes_stats_{tag}", err_over_bound_max=(err / bound.clamp_min(1e-300)).max(), err_max=err.max())
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    assert _untouched(stats, before, idx, 2 * ntile)


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) the residual pair + the LayerNorm-statistics producer, bf16 (gemm_stream_kernel<0, 6, true, 0, STATS>)
# ------------------------------------------------------------------------------------------------------------------------------------
def _residual_case(B, T, K, N, stats, variant, seed, w8=False):
    """-> everything one residual launch read and wrote.  variant: plain / inplace (C == res, c_lo == res_lo) / ragged."""
    g = _gen(B, T, K, N, seed)
    x = G.Rows(B, T, K).set(torch.randn(B, T, K, generator=g).cuda())
    if w8:
        w, ws = _w_e4m3(g, N, K)
        wv = R.e4m3_decode(w)
    else:
        w, ws = _w_bf16(g, N, K), None
        wv = w.double()
    bias = (torch.randn(N, generator=g) * 0.2).cuda()
    res, res_lo = _pair_rows(g, B, T, N)
    out, out_lo = (res, res_lo) if variant == "inplace" else (_sent_rows(B, T, N), _sent_rows(B, T, N))
    st = torch.full((out.R, 4, 2), SENT, dtype=torch.float32, device="cuda") if stats else None
    clip_T = RAGGED if variant == "ragged" else None
    before = dict(out=out.buf.clone(), lo=out_lo.buf.clone(), res=res.buf.clone(), res_lo=res_lo.buf.clone(),
                  st=st.clone() if stats else None)
    _launch(x, K, w, N, out, 7 if w8 else 1, bias=bias, res=res.buf, res_lo=res_lo.buf, ldres=N, c_lo=out_lo.buf, alpha=0.5,
            stats_out=st, clip_T=_clip_T(clip_T), w8_scale=ws)
    torch.cuda.synchronize()
    mask = R.ragged_mask(B, T, clip_T).cuda()
    idx = _grid(out)[mask]
    a = x.get().double().reshape(B * T, K)[mask.reshape(-1)]
    v, mag = R.gemm_ref(a, wv, bias, None, ws)
    ref, mag = R.residual_pair_ref(v, mag, before["res"][idx].double(), before["res_lo"][idx].double(), 0.5)
    return dict(x=x, w=w, ws=ws, bias=bias, out=out, out_lo=out_lo, st=st, before=before, idx=idx, ref=ref, mag=mag, clip_T=clip_T,
                res_hi=before["res"], res_lo=before["res_lo"], res_geo=res)


def _check_residual(c, K, N, tag):
    got = c["out"].buf[c["idx"]].double() + c["out_lo"].buf[c["idx"]].double()
    err = (got - c["ref"]).abs()
    _note(f"gemm_modes_{tag}", err_over_mag_max=(err / c["mag"]).max(), err_max=err.max())
    tol = R.tol_pair(c["ref"], c["mag"], K)
    assert bool((err <= tol).all()), float((err / c["mag"]).max())
    assert _untouched(c["out"].buf, c["before"]["out"], c["idx"], N) and _untouched(c["out_lo"].buf, c["before"]["lo"], c["idx"], N)
    if c["st"] is not None:
        _check_stats(c["st"], c["before"]["st"], c["out"], c["idx"], N, tag)


def _check_clip0_alone(c, B, T, K, N, kid, tag):
    """Clip 0 launched alone equals its rows of the batch launch bit for bit: C, c_lo and the statistics (csrc/gemm_stream.hip, the
    comment in wfl_gemm_stream_takes: no lower bound on M, so that a clip labelled alone equals the same clip inside a batch)."""
    x, out = c["x"], c["out"]
    x1 = G.Rows(1, T, K)
    x1.buf[x1.lead:x1.lead + T] = x.buf[x.lead:x.lead + T]
    res1, lo1 = G.Rows(1, T, N), G.Rows(1, T, N)
    res1.buf[res1.lead:res1.lead + T] = c["res_hi"][out.lead:out.lead + T]
    lo1.buf[lo1.lead:lo1.lead + T] = c["res_lo"][out.lead:out.lead + T]
    out1, out1_lo = _sent_rows(1, T, N), _sent_rows(1, T, N)
    st1 = torch.full((out1.R, 4, 2), SENT, dtype=torch.float32, device="cuda") if c["st"] is not None else None
    _launch(x1, K, c["w"], N, out1, kid, bias=c["bias"], res=res1.buf, res_lo=lo1.buf, ldres=N, c_lo=out1_lo.buf, alpha=0.5,
            stats_out=st1, clip_T=_clip_T(c["clip_T"][:1] if c["clip_T"] else None), w8_scale=c["ws"])
    torch.cuda.synchronize()
    n0 = T if not c["clip_T"] else c["clip_T"][0]
    a, b = slice(out1.lead, out1.lead + n0), slice(out.lead, out.lead + n0)
    assert torch.equal(out1.buf[a], out.buf[b]) and torch.equal(out1_lo.buf[a], c["out_lo"].buf[b]), tag
    if st1 is not None:
        assert torch.equal(st1[a][:, :N // 256], c["st"][b][:, :N // 256]), tag


@pytest.mark.parametrize("rows,K,N,variant", [
    ("small", 512, 512, "plain"), ("small", 512, 512, "inplace"), ("small", 256, 768, "plain"), ("small", 256, 768, "ragged"),
    ("walk", 256, 1024, "plain")])
@pytest.mark.parametrize("stats", [False, True])
def test_residual_pair_and_statistics_producer(rows, K, N, variant, stats):
    """C + c_lo = res_hi + res_lo + alpha (A W^T + b) to sixteen bits; stats_out[(row 4 + tile) 2 + {0, 1}] = the sum and the sum of squares
    of the bf16 values stored in C for that row's 256 columns -- C was checked just above, so this checks the summation alone."""
    B, T = (RAGGED_B, RAGGED_T) if variant == "ragged" else ROWS[rows]
    tag = f"a_{rows}_K{K}_N{N}_{variant}_stats{int(stats)}"
    c = _residual_case(B, T, K, N, stats, variant, seed=1)
    _check_residual(c, K, N, tag)
    if variant != "inplace":
        _check_clip0_alone(c, B, T, K, N, 1, tag)


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) the consumer: LayerNorm folded into the GEMM, statistics from a producer (ln_s + stats_in / stats_nsl / stats_lead)
# ------------------------------------------------------------------------------------------------------------------------------------
def _ln_inputs(g, B, T, K, kind, chain):
    """-> (x rows, stats buffer [R, 4, 2] fp32 indexed by x's buffer row).  chain: the rows and their statistics are what a real
    residual + statistics launch wrote; else the test's own float64 sums, rounded once, unused slots and rows NaN."""
    if chain:
        c = _residual_case(B, T, 256, K, True, "plain", seed=3)
        return c["out"], c["st"]
    x0 = torch.randn(B, T, K, generator=g)
    if kind == "offset":
        x0 = x0 + 30
    if kind == "outlier":
        x0[..., 7] *= 100
    x = G.Rows(B, T, K).set(x0.cuda())
    st = torch.full((x.R, 4, 2), math.nan, dtype=torch.float32, device="cuda")
    st[_grid(x).reshape(-1)] = R.row_stats_slots(x.get().double().reshape(B * T, K), K // 256)
    return x, st


def _ln_fold_case(rows, K, N, act, chain, kind, w8, tag):
    B, T = ROWS[rows]
    g = _gen(B, T, K, N, act, 5)
    x, st = _ln_inputs(g, B, T, K, kind, chain)
    gamma = torch.randn(K, generator=g) * 0.2 + 1
    if w8:
        w, ws = _w_e4m3(g, N, K)
        wv = R.e4m3_decode(w) * ws.double()[:, None]
    else:
        w, ws = (torch.randn(N, K, generator=g) * K ** -0.5 * gamma[None, :]).to(torch.bfloat16).cuda(), None
        wv = w.double()
    bias = (torch.randn(N, generator=g) * 0.2).cuda()
    ln_s = wv.sum(1).float()
    out = _sent_rows(B, T, N)
    before = out.buf.clone()
    _launch(x, K, w, N, out, 7 if w8 else 1, bias=bias, act=act, ln_s=ln_s, ln_eps=1e-5, stats_in=st, stats_nsl=K // 256,
            stats_lead=x.lead, w8_scale=ws)
    torch.cuda.synchronize()
    idx = _grid(out).reshape(-1)
    a = x.buf[_grid(x).reshape(-1)].double()                       # the operand is `hi` alone
    v, mag, cancel = R.ln_fold_ref(a, wv, bias, R.tile_stats_ref(a)[0], K // 256, 1e-5)
    ref, lip = (F.gelu(v), R.GELU_LIPSCHITZ) if act else (v, 1.0)
    err = (out.buf[idx].double() - ref).abs()
    tol = R.tol_ln_fold(ref, mag, cancel, K, lip)
    _note(f"gemm_modes_{tag}", err_over_mag_max=(err / mag).max(), err_over_tol_max=(err / tol).max(), err_max=err.max())
    assert bool((err <= tol).all()), (float((err / tol).max()), float((err / mag).max()))
    assert _untouched(out.buf, before, idx, N)


@pytest.mark.parametrize("rows,K,N,act,chain,kind", [(r, K, 512, act, chain, "normal")
                                                   for r in ("small",) for K in (256, 512, 768, 1024) for act in (0, 1)
                                                   for chain in (False, True)] + [
    ("walk", 512, 1536, 1, False, "normal"), ("walk", 512, 1536, 0, True, "normal"),
    ("small", 512, 512, 0, False, "offset"), ("small", 512, 512, 1, False, "outlier")])
def test_layernorm_fold_from_statistics(rows, K, N, act, chain, kind):
    """Reference: float64 LayerNorm of the bf16 rows, then @ W'^T + b.  Bound: 2^-8 |ref| + rstd K 2^-24 (sum |a||w'| + |mean| sum |w'|)
    + 2^-22 (E[x^2] / var) |ref - bias| -- the last term is the cancellation of the one-pass variance E[x^2] - mean^2."""
    _ln_fold_case(rows, K, N, act, chain, kind, False, f"b_{rows}_K{K}_N{N}_act{act}_chain{int(chain)}_{kind}")


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) e4m3 weights x bf16 activations (w8_scale): the conversion to bf16 is exact, so the bounds are those of the bf16 forms
# ------------------------------------------------------------------------------------------------------------------------------------
def _w8_cases():
    out = []
    for K in (512, 1280):
        for N in (256, 768, 1280):
            forms = ["plain", "gelu", "res"] + (["res_stats"] if N <= 1024 else []) + (["lnfold"] if K == 512 else [])
            out += [("small", K, N, f) for f in forms]
    return out + [("walk", 512, 1024, f) for f in ("plain", "gelu", "res", "res_stats", "lnfold")]


@pytest.mark.parametrize("rows,K,N,form", _w8_cases())
def test_e4m3_weights_times_bf16_activations(rows, K, N, form):
    B, T = ROWS[rows]
    tag = f"c_{rows}_K{K}_N{N}_{form}"
    if form in ("res", "res_stats"):
        c = _residual_case(B, T, K, N, form == "res_stats", "plain", seed=7, w8=True)
        _check_residual(c, K, N, tag)
        _check_clip0_alone(c, B, T, K, N, 7, tag)
        return
    if form == "lnfold":
        _ln_fold_case(rows, K, N, 1, False, "normal", True, tag)
        return
    g = _gen(B, T, K, N, 9)
    x = G.Rows(B, T, K).set(torch.randn(B, T, K, generator=g).cuda())
    w, ws = _w_e4m3(g, N, K)
    bias = (torch.randn(N, generator=g) * 0.2).cuda()
    out = _sent_rows(B, T, N)
    before = out.buf.clone()
    act = int(form == "gelu")
    _launch(x, K, w, N, out, 7, bias=bias, act=act, w8_scale=ws)
    torch.cuda.synchronize()
    idx = _grid(out).reshape(-1)
    v, mag = R.gemm_ref(x.get().double().reshape(B * T, K), R.e4m3_decode(w), bias, None, ws)
    ref, lip = (F.gelu(v), R.GELU_LIPSCHITZ) if act else (v, 1.0)
    err = (out.buf[idx].double() - ref).abs()
    _note(f"gemm_modes_{tag}", err_over_mag_max=(err / mag).max(), err_max=err.max())
    assert bool((err <= R.tol_bf16(ref, mag, K, lip)).all()), float((err / mag).max())
    assert _untouched(out.buf, before, idx, N)


# ------------------------------------------------------------------------------------------------------------------------------------
# (d) fp8 x fp8 on the non-scaled MFMA (a8 == 1), operands from wfl_op_rows_fp8
# ------------------------------------------------------------------------------------------------------------------------------------
A8_STATIC = 0.0078125


def _a8_operands(B, T, K, N, seed):
    g = _gen(B, T, K, N, seed)
    x = G.Rows(B, T, K).set((torch.randn(B, T, K, generator=g) * 0.7).cuda())
    hi, _, sc = _rows_fp8(x)
    w, ws = _w_e4m3(g, N, K)
    bias = (torch.randn(N, generator=g) * 0.2).cuda()
    return g, x, hi, sc, w, ws, bias


def _a8_ref(x, hi, sc, w, ws, bias, static):
    rows = _grid(x).reshape(-1)
    rs = torch.full((rows.numel(),), A8_STATIC, dtype=torch.float64, device="cuda") if static else sc[rows]
    return R.gemm_ref(R.e4m3_decode(hi[rows]), R.e4m3_decode(w), bias, rs, ws)


def _a8_launch(x, hi, sc, w, ws, K, N, out, static, **kw):
    return _launch(x, K, w, N, out, 7, A=(hi, x.lead * K), a8=1, w8_scale=ws, a8_scale=None if static else sc, a8_lead=x.lead,
                   a8_static=A8_STATIC if static else 0.0, **kw)


@pytest.mark.parametrize("rows,K,N,form,static", [(r, K, 768, f, s) for r, K in (("small", 512), ("small", 1280)) for f in ("plain", "res", "gelu_c8")
                                                  for s in (False, True)] + [("walk", 512, 1024, "res", False), ("walk", 512, 1024, "gelu_c8", False)])
def test_fp8_activations_on_the_nonscaled_mfma(rows, K, N, form, static):
    """The float64 product of the very bytes given, times the row's scale (a8_scale[a8_lead + m], or a8_static) and the channel's.
    Accumulation term: K 2^-24 mag, like an fp32 chain.  Status: 0 where the reference fits e4m3 by a factor two, 2 where it misses by two."""
    B, T = ROWS[rows]
    tag = f"d_{rows}_K{K}_N{N}_{form}_static{int(static)}"
    g, x, hi, sc, w, ws, bias = _a8_operands(B, T, K, N, 11)
    v, mag = _a8_ref(x, hi, sc, w, ws, bias, static)
    if form == "gelu_c8":
        ref = F.gelu(v)
        top = float(ref.abs().max())
        geo = G.Rows(B, T, N)                                          # (the row geometry of the e4m3 output; its bf16 buffer is not used)
        orow = _grid(geo).reshape(-1)
        for inv, want in ((224.0 / top, 0), (896.0 / top, 2)):
            c8 = torch.full((geo.R, N), SENT8, dtype=torch.uint8, device="cuda")
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            _a8_launch(x, hi, sc, w, ws, K, N, geo, static, bias=bias, act=1, c8=c8, ldc8=N, c8_inv_scale=inv, status=status)
            torch.cuda.synchronize()
            assert int(status.item()) == want, (inv, int(status.item()))
            keep = torch.ones(geo.R, dtype=torch.bool, device="cuda")
            keep[orow] = False
            assert bool((c8[keep] == SENT8).all())
            if want == 0:
                got = R.e4m3_decode(c8[orow]) / inv
                err = (got - ref).abs()
                tol = 2.0 ** -4 * ref.abs().clamp_min(2.0 ** -6 / inv) + R.GELU_LIPSCHITZ * K * 2.0 ** -24 * mag
                _note(f"gemm_modes_{tag}", err_over_tol_max=(err / tol).max(), err_max=err.max())
                assert bool((err <= tol).all()), float((err / tol).max())
        return
    out = _sent_rows(B, T, N)
    before = out.buf.clone()
    idx = _grid(out).reshape(-1)
    if form == "res":
        res, res_lo = _pair_rows(g, B, T, N, sentinel=False)
        out_lo = _sent_rows(B, T, N)
        _a8_launch(x, hi, sc, w, ws, K, N, out, static, bias=bias, res=res.buf, res_lo=res_lo.buf, ldres=N, c_lo=out_lo.buf, alpha=0.5)
        torch.cuda.synchronize()
        ref, mag = R.residual_pair_ref(v, mag, res.buf[idx].double(), res_lo.buf[idx].double(), 0.5)
        got, tol = out.buf[idx].double() + out_lo.buf[idx].double(), R.tol_pair(ref, mag, K)
        assert _untouched(out_lo.buf, before, idx, N)
    else:
        _a8_launch(x, hi, sc, w, ws, K, N, out, static, bias=bias)
        torch.cuda.synchronize()
        ref = v
        got, tol = out.buf[idx].double(), R.tol_bf16(ref, mag, K)
    err = (got - ref).abs()
    _note(f"gemm_modes_{tag}", err_over_mag_max=(err / mag).max(), err_max=err.max())
    assert bool((err <= tol).all()), float((err / mag).max())
    assert _untouched(out.buf, before, idx, N)


# ------------------------------------------------------------------------------------------------------------------------------------
# (e) NaN and Inf in an e4m3 output: status 2 ("saturates or NaN", csrc/common.h GemmArgs::err), judged on stored elements only
# ------------------------------------------------------------------------------------------------------------------------------------
E_B, E_T, E_K, E_N = 2, 100, 512, 256


@pytest.mark.parametrize("where,value,want", [("valid_row", math.nan, 2), ("valid_row", math.inf, 2), ("halo_row", math.nan, 0), ("clean", 0.0, 0)])
@pytest.mark.parametrize("entry", ["mx_single", "mx_pair", "stream_c8"])
def test_e4m3_output_reports_nan_and_inf(entry, where, value, want):
    B, T, K, N = E_B, E_T, E_K, E_N
    g = _gen(B, T, K, N, 13)
    x = G.Rows(B, T, K).set((torch.randn(B, T, K, generator=g) * 0.7).cuda())
    pair = entry == "mx_pair"
    hi, lo, sc = _rows_fp8(x, pair=pair)
    w, ws = _w_e4m3(g, N, K)
    if where == "valid_row":
        sc[x.lead + x.P + 37] = value                                 # clip 1, frame 37
    if where == "halo_row":
        sc[x.lead + T + 2] = value                                    # a row t >= T: computed, never stored
    geo = G.Rows(B, T, N)
    c8 = torch.full((geo.R, N), SENT8, dtype=torch.uint8, device="cuda")
    c8lo = torch.full((geo.R, N), SENT8, dtype=torch.uint8, device="cuda") if pair else None
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    if entry == "stream_c8":
        _launch(x, K, w, N, geo, 7, A=(hi, x.lead * K), a8=1, w8_scale=ws, a8_scale=sc, a8_lead=x.lead, act=1, c8=c8, ldc8=N,
                c8_inv_scale=4.0, status=status)
    else:
        rc = G.lib().wfl_op_gemm_mx(G.ptr(hi, x.lead * K), G.ptr(lo, x.lead * K) if pair else None, K, G.ptr(w), G.ptr(ws), G.ptr(sc, x.lead), 1.0,
                                    B * x.P, N, K, x.P, T, G.ptr(geo.buf), N, geo.lead, geo.P, None, None, None, None, 1.0, 1, G.ptr(c8),
                                    G.ptr(c8lo), N, 4.0, G.ptr(status), G.stream())
        G._lib.check(rc, "wfl_op_gemm_mx")
    torch.cuda.synchronize()
    assert int(status.item()) == want, (entry, where, value, int(status.item()))
    keep = torch.ones(geo.R, dtype=torch.bool, device="cuda")
    keep[_grid(geo).reshape(-1)] = False
    assert bool((c8[keep] == SENT8).all()) and (c8lo is None or bool((c8lo[keep] == SENT8).all()))


def test_e4m3_output_ignores_nan_in_columns_that_are_not_stored():
    """columns >= n_valid are computed and not stored: a NaN there (their channel scale) sets no status bit and writes nothing"""
    B, T, K, N, nv = E_B, E_T, E_K, E_N, 200
    g = _gen(B, T, K, N, 17)
    x = G.Rows(B, T, K).set((torch.randn(B, T, K, generator=g) * 0.7).cuda())
    hi, _, sc = _rows_fp8(x)
    w, ws = _w_e4m3(g, N, K)
    ws[nv:] = math.nan
    geo = G.Rows(B, T, N)
    c8 = torch.full((geo.R, N), SENT8, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    _launch(x, K, w, N, geo, 7, A=(hi, x.lead * K), a8=1, w8_scale=ws, a8_scale=sc, a8_lead=x.lead, act=1, c8=c8, ldc8=N, c8_inv_scale=4.0,
            status=status, n_valid=nv)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert _untouched(c8, torch.full_like(c8, SENT8), _grid(geo).reshape(-1), nv)
    assert bool((c8[_grid(geo).reshape(-1), :nv] != SENT8).any())


# ------------------------------------------------------------------------------------------------------------------------------------
# (g) the positional table, the per-clip bias, ragged batches and the fp32 accumulate on the 128-tile kernel (id 4) and gemm256 (2 / 3)
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,kid", [(2, 128, 4), (13, 256, (2, 3))])
def test_positional_table_behind_the_stride2_conv(B, N, kid):
    """The Whisper stem's second conv (k 3, stride 2, padding 1 as a GEMM with lda = 2 C over rows of twice the pitch) + GELU + the real
    `pos` field: the table row is t.  The table has more rows than T, all distinct, so a wrong row index shows."""
    T, C = 150, 64
    g = _gen(B, N, 19)
    geo = G.Rows(B, T, N, halo=18, lead=16)                            # P = 168; 13 clips: 2184 rows >= 2048, gemm256's lower bound
    out = G.Rows(B, T, N, halo=18, lead=16)
    out.buf.fill_(SENT)
    before = out.buf.clone()
    a = G.Rows(B, 2 * T, C, lead=8, pitch=2 * geo.P, tail=512).set(torch.randn(B, 2 * T, C, generator=g).cuda())
    w = _w_bf16(g, N, 3 * C)
    bias = (torch.randn(N, generator=g) * 0.1).cuda()
    pos = torch.randn(T + 40, N, generator=g).to(torch.bfloat16).cuda()
    M = B * geo.P
    _, got_kid = G.gemm_ex(A=(a.buf, (a.lead - 1) * C), lda=2 * C, W=w, M=M, N=N, K=3 * C, n_valid=N, P=geo.P, T=T, C=out.buf, ldc=N,
                           c_lead=out.lead, c_pitch=out.P, bias=bias, act=1, alpha=1.0, pos=pos, ldpos=N)
    assert got_kid in (kid if isinstance(kid, tuple) else (kid,)), got_kid
    torch.cuda.synchronize()
    rows = torch.as_strided(a.buf, (M, 3 * C), (2 * C, 1), (a.lead - 1) * C).double().view(B, geo.P, 3 * C)[:, :T].reshape(B * T, 3 * C)
    v, mag = R.gemm_ref(rows, w.double(), bias)
    ref, mag = R.gemm_table_terms(v, mag, B, T, act="gelu", pos=pos)
    idx = _grid(out).reshape(-1)
    err = (out.buf[idx].double() - ref).abs()
    _note(f"gemm_modes_g_pos_B{B}_N{N}", err_over_mag_max=(err / mag).max(), err_max=err.max(), kernel=got_kid)
    assert bool((err <= R.tol_bf16(ref, mag, 3 * C, R.GELU_LIPSCHITZ)).all()), float((err / mag).max())
    assert _untouched(out.buf, before, idx, N)


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("plain_bias", [False, True])
@pytest.mark.parametrize("ragged", [False, True])
def test_clip_bias_table_and_ragged_batches(big, plain_bias, ragged):
    """clip_bias: a 4-row table with clip_ld > N, clip_idx a non-identity map with a repeated row, added before the activation; clip_T
    with the length pattern of (a); c_lo without a residual (what keeps these launches away from the streaming kernel's epilogue is
    clip_bias itself)."""
    K, N, ld = 256, 256, 264
    B, T = (8, 300) if big else (RAGGED_B, RAGGED_T)                  # 8 x 320 = 2560 rows: gemm256; 1280: the 128-tile kernel
    clip_T = (RAGGED * (B // 4)) if ragged else None
    g = _gen(B, big, plain_bias, ragged, 23)
    x = G.Rows(B, T, K).set(torch.randn(B, T, K, generator=g).cuda())
    w = _w_bf16(g, N, K)
    bias = (torch.randn(N, generator=g) * 0.2).cuda() if plain_bias else None
    table = torch.randn(4, ld, generator=g).cuda()
    cidx = [(3, 1, 3, 0, 2, 2, 1, 0)[b] for b in range(B)]
    out, out_lo = _sent_rows(B, T, N), _sent_rows(B, T, N)
    before = out.buf.clone()
    kid = _launch(x, K, w, N, out, (2, 3) if big else 4, bias=bias, act=2, clip_bias=table, clip_idx=torch.tensor(cidx, dtype=torch.int32, device="cuda"),
                  clip_ld=ld, clip_T=_clip_T(clip_T), c_lo=out_lo.buf)
    torch.cuda.synchronize()
    mask = R.ragged_mask(B, T, clip_T).cuda().reshape(-1)
    v, mag = R.gemm_ref(x.get().double().reshape(B * T, K), w.double(), bias)
    ref, mag = R.gemm_table_terms(v, mag, B, T, table, cidx, "relu")
    ref, mag = ref[mask], mag[mask]
    idx = _grid(out).reshape(-1)[mask]
    err = (out.buf[idx].double() + out_lo.buf[idx].double() - ref).abs()
    _note(f"gemm_modes_g_clipbias_big{int(big)}_bias{int(plain_bias)}_ragged{int(ragged)}", err_over_mag_max=(err / mag).max(), err_max=err.max(), kernel=kid)
    assert bool((err <= R.tol_pair(ref, mag, K)).all()), float((err / mag).max())
    assert _untouched(out.buf, before, idx, N) and _untouched(out_lo.buf, before, idx, N)


def test_ragged_batch_on_the_plain_streaming_kernel():
    K, N = 256, 512
    B, T, clip_T = RAGGED_B, RAGGED_T, RAGGED
    g = _gen(B, T, K, N, 29)
    x = G.Rows(B, T, K).set(torch.randn(B, T, K, generator=g).cuda())
    w = _w_bf16(g, N, K)
    bias = (torch.randn(N, generator=g) * 0.2).cuda()
    out = _sent_rows(B, T, N)
    before = out.buf.clone()
    _launch(x, K, w, N, out, 1, bias=bias, act=1, clip_T=_clip_T(clip_T))
    torch.cuda.synchronize()
    mask = R.ragged_mask(B, T, clip_T).cuda().reshape(-1)
    v, mag = R.gemm_ref(x.get().double().reshape(B * T, K)[mask], w.double(), bias)
    ref = F.gelu(v)
    idx = _grid(out).reshape(-1)[mask]
    err = (out.buf[idx].double() - ref).abs()
    _note("gemm_modes_g_ragged_stream", err_over_mag_max=(err / mag).max(), err_max=err.max())
    assert bool((err <= R.tol_bf16(ref, mag, K, R.GELU_LIPSCHITZ)).all()), float((err / mag).max())
    assert _untouched(out.buf, before, idx, N)


@pytest.mark.parametrize("big", [False, True])
def test_fp32_output_accumulates_into_c(big):
    """out_f32 + acc_f32 (the split-precision classifier adds its passes up in fp32): C = C_before + result within the project's f32-out
    bound (1e-3 relative + absolute); n_valid = 141, the columns beyond and every row that is no frame keep what they held."""
    K, N, nv, ldc = 256, 256, 141, 160
    B, T = (8, 300) if big else (3, 333)
    g = _gen(B, T, big, 31)
    x = G.Rows(B, T, K).set(torch.randn(B, T, K, generator=g).cuda())
    w = _w_bf16(g, N, K)
    w[nv:] = 0
    bias = torch.zeros(N, device="cuda")
    bias[:nv] = (torch.randn(nv, generator=g) * 0.2).cuda()
    geo = G.Rows(B, T, 8)
    c = (torch.randn(geo.R, ldc, generator=g) * 3).cuda()
    before = c.clone()
    kid = _launch(x, K, w, N, geo, (2, 3) if big else 4, C=c, ldc=ldc, n_valid=nv, bias=bias, out_f32=1, acc_f32=1)
    torch.cuda.synchronize()
    idx = _grid(geo).reshape(-1)
    v, mag = R.gemm_ref(x.get().double().reshape(B * T, K), w.double()[:nv], bias[:nv])
    ref = before[idx, :nv].double() + v
    err = (c[idx, :nv].double() - ref).abs()
    _note(f"gemm_modes_g_acc_f32_big{int(big)}", err_over_mag_max=(err / (mag + before[idx, :nv].abs())).max(), err_max=err.max(), kernel=kid)
    assert bool((err <= 1e-3 * ref.abs() + 1e-3).all()), float(err.max())
    assert _untouched(c, before, idx, nv)
