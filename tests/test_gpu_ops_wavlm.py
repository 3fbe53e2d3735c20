"""-m gpu: attention's bias / ragged / split / fp8 modes and the WavLM-path kernels (relative-position table and gate, regroup,
positional conv, the LayerNorm launchers with GELU / pairs / n_div / clip_T), each through its single-op export against the float64
references of tests/ops_ref.py on the values the kernel reads.  The inputs come from ops_ref's seeded functions, so the CPU controls of
tests/test_ops_ref_cpu.py (a wrong reference violates each case's bound) speak about exactly these cases.

No element is excluded: every valid output element is compared, and whatever must not be written -- rows at t >= clip_T[b], whole
clips of length 0 -- is pre-filled with a sentinel (bf16 7.0) and compared bit for bit afterwards; halos must stay zero."""
import functools

import pytest
import torch

import gpu_util as G
import ops_ref as R
from test_gpu_model import _note

pytestmark = pytest.mark.gpu

SENT = 7.0


def _rows(B, T, Cn, x=None, **kw):
    """Frame rows holding x [B, T, Cn], or the sentinel in every valid frame."""
    r = G.Rows(B, T, Cn, **kw)
    return r.set(x.cuda() if x is not None else torch.full((B, T, Cn), SENT))


def _valid(B, T, clip_T):
    n = torch.tensor([T] * B if clip_T is None else list(clip_T))
    return torch.arange(T)[None, :] < n[:, None]


def _within(got, ref, bound, what):
    err = (got - ref).abs()
    assert bool((err <= bound).all()), f"{what}: max err {float(err.max()):.4g}, worst excess {float((err - bound).max()):.4g}, " \
                                       f"{int((err > bound).sum())} of {err.numel()} elements"


# ------------------------------------------------------------------------------------------------------------------ attention
def _attention(c, o_lo=False):
    """Run a case of ops_ref.attn_inputs.  -> (O rows, O_lo rows or None)."""
    B, T, d, heads = c["B"], c["T"], c["d"], c["heads"]
    qk = _rows(B, T, 2 * d, torch.cat([c["q_hi"], c["k_hi"]], -1))
    v = _rows(B, T, d, c["v_hi"])
    qkl = _rows(B, T, 2 * d, torch.cat([c["q_lo"], c["k_lo"]], -1)) if c["pair"] else None
    vl = _rows(B, T, d, c["v_lo"]) if c["pair"] else None
    o = _rows(B, T, d)
    ol = _rows(B, T, d) if (o_lo or c["pair"]) else None
    bias = c["table"].cuda().contiguous() if c["table"] is not None else None
    gate = c["gate"].cuda().contiguous() if c["gate"] is not None else None
    G.attention_ex(qk.buf, 2 * d, qk.lead, v.buf, 0, d, o.buf, d, B, T, qk.P, heads, d, QK_lo=qkl.buf if qkl else None,
                   V_lo=vl.buf if vl else None, O_lo=ol.buf if ol else None, bias=bias, gate=gate, clip_T=G._i32(c["clip_T"]))
    torch.cuda.synchronize()
    assert o.halo_is_zero() and (ol is None or ol.halo_is_zero())
    return o, ol


def _check_attention(c, name):
    """The whole comparison of one case: valid rows against the reference under the case's bound, the rest against the sentinel."""
    ref, A = R.attn_case_ref(c)
    o, ol = _attention(c)
    got = o.get().double().cpu() + (ol.get().double().cpu() if c["pair"] else 0.0)
    m = _valid(c["B"], c["T"], c["clip_T"])
    err = (got - ref).abs()[m]
    _note(name, err_max=err.max() if err.numel() else 0.0, err_over_A_max=(err / A[m]).max() if err.numel() else 0.0)
    bound = R.attn_bound_split(ref, A) if c["pair"] else R.attn_bound_bf16(ref)
    _within(got[m], ref[m], bound[m], name)
    for r in (o, ol) if c["pair"] else (o,):
        assert bool((r.get().cpu()[~m] == SENT).all()), "a row beyond the clip's own length was written"
    return got, ref


@pytest.mark.parametrize("hd,heads,T", R.ATTN_BIAS_CASES)
def test_attention_gated_relative_position_bias(hd, heads, T):
    """bf16 bias kernel.  T = 64: one exact tile (no last-tile mask); T = 257: 3 query blocks, 5 key tiles, a last tile of one key and
    the table slice clamped at both ends.  Tolerance: test_qkv_projection_and_attention's."""
    _check_attention(R.bias_case(hd, heads, T), f"attn_bias_hd{hd}_T{T}")


@pytest.mark.parametrize("variant,hd", R.ATTN_CLIP_CASES)
def test_attention_clip_lengths_against_the_reference(variant, hd):
    """clip_T = [257, 70, 1, 0] in a batch of T = 257; K and V rows beyond each clip hold 50.0."""
    c = R.clip_case(variant, hd)
    got, _ = _check_attention(c, f"attn_clip_{variant}_hd{hd}")
    v = c["v_hi"].double() + c["v_lo"].double()
    one = (got[2, 0] - v[2, 0]).abs()                                  # clip 2's one frame attends itself alone: its v row
    assert bool((one <= (2.0 ** -15 * v[2, 0].abs() if c["pair"] else 0.0)).all()), float(one.max())
    # (clip 3, no frames: every row still holds the sentinel -- checked in _check_attention)


# kappa: measured max(err / A) on MI355X (parity_stats.jsonl notes, attn_split_* and attn_clip_split_hd64):
#   hd 32  3.12e-6     hd 64  2.71e-6     hd 128  2.59e-6     hd 256  3.49e-6     hd 64, clip_T  3.94e-6
#   hd 32 + bias  9.86e-6     hd 64 + bias  1.211e-5
# ops_ref.ATTN_KAPPA = 4 x the largest = 4.84e-5: room for another summation order, not for a lost pass -- a kernel that drops the low
# halves is off by ~1e-3 A (tests/test_ops_ref_cpu.py, test_control_split_cases).


@pytest.mark.parametrize("hd,bias", R.ATTN_SPLIT_CASES)
def test_attention_split_precision(hd, bias):
    """QK_lo / V_lo / O_lo: O + O_lo against the reference over the hi + lo operands, 2^-15 |ref| + kappa A."""
    _check_attention(R.split_case(hd, bias), f"attn_split_hd{hd}_bias{int(bias)}")


@pytest.mark.parametrize("hd", [64, 256])
def test_attention_low_half_of_the_plain_kernel(hd):
    c = R.attn_inputs(hd, 2, 2, 257, seed=40 + hd)
    ref, _ = R.attn_case_ref(c)
    o1, _ = _attention(c)
    o2, ol = _attention(c, o_lo=True)
    assert torch.equal(o1.buf, o2.buf)                                 # O does not depend on O_lo being asked for
    hi, lo = o2.get().double().cpu(), ol.get().double().cpu()
    # O_lo = bf16(o - O) is at most half a unit in the last place of O.  bf16 has 8 significant bits: for |O| in [2^e, 2^(e+1)) the
    # spacing is 2^(e-7), half of it 2^(e-8) -- that is 2^-9 of the binade's upper end, and up to 2^-8 |O| at its lower end.
    _, ex = torch.frexp(hi)                                            # |hi| = m 2^ex, m in [0.5, 1): 2^e = 2^(ex - 1)
    assert bool((lo.abs() <= torch.ldexp(torch.tensor(1.0, dtype=torch.float64), ex - 9)).all())
    e_hi, e_pair = float((hi - ref).abs().max()), float((hi + lo - ref).abs().max())
    _note(f"attn_o_lo_hd{hd}", err_hi=e_hi, err_pair=e_pair)
    assert e_pair <= e_hi
    _within(hi, ref, R.attn_bound_bf16(ref), "plain attention")


def _o8_run(c, pair, o8_scale=64.0):
    B, T, d, heads = c["B"], c["T"], c["d"], c["heads"]
    qk = _rows(B, T, 2 * d, torch.cat([c["q_hi"], c["k_hi"]], -1))
    v = _rows(B, T, d, c["v_hi"])
    hi = torch.full((qk.R, d), 0x55, dtype=torch.uint8, device="cuda")
    lo = torch.full((qk.R, d), 0x55, dtype=torch.uint8, device="cuda") if pair else None
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    G.attention_ex(qk.buf, 2 * d, qk.lead, v.buf, 0, d, None, d, B, T, qk.P, heads, d, O8=hi, O8_lo=lo, ldo8=d, o8_scale=o8_scale,
                   status=status)
    torch.cuda.synchronize()
    rows = (qk.lead + torch.arange(B)[:, None] * qk.P + torch.arange(T)[None, :]).reshape(-1).cuda()
    other = torch.ones(qk.R, dtype=torch.bool, device="cuda")
    other[rows] = False
    for p in (hi, lo) if pair else (hi,):
        assert bool((p[other] == 0x55).all()), "a byte outside the valid frames was written"
    dec = lambda p: p[rows].view(torch.float8_e4m3fn).float().double().cpu().view(B, T, d)      # noqa: E731
    return dec(hi), dec(lo) if pair else None, int(status.item())


def test_attention_fp8_context():
    """O8 (+ O8_lo) at head_dim 64: hi / scale within one e4m3 rounding (2^-4 relative) of the reference, (hi + lo / 16) / scale within
    2^-8 -- the claim of test_rows_fp8_pair_carries_eight_significant_bits -- plus e4m3's subnormal step over the scale; no saturation."""
    scale = 64.0
    c = R.attn_inputs(64, 2, 2, 129, seed=50, v_range=(0.25, 1.0))               # |v| <= 1: |v| * scale <= 64, far from 448
    ref, _ = R.attn_case_ref(c)
    floor = 2.0 ** -9 / scale
    h1, _, st1 = _o8_run(c, False, scale)
    h2, l2, st2 = _o8_run(c, True, scale)
    assert torch.equal(h1, h2) and st1 == 0 and st2 == 0
    e1, e2 = (h1 / scale - ref).abs(), ((h2 + l2 / 16) / scale - ref).abs()
    _note("attn_fp8_context", rel_single_max=(e1 / ref.abs()).max(), rel_pair_max=(e2 / ref.abs()).max())
    _within(h1 / scale, ref, 2.0 ** -4 * ref.abs() + floor, "e4m3 context")
    _within((h2 + l2 / 16) / scale, ref, 2.0 ** -8 * ref.abs() + floor, "e4m3 pair context")


def test_attention_fp8_context_saturation_is_flagged():
    """One query attends one key (as in test_attention_peaked_softmax) whose v row is +-100: 6400 at scale 64 does not fit e4m3, the
    element is stored as +-448 and bit 1 of the status word is set."""
    c = R.attn_inputs(64, 1, 1, 200, seed=51, v_range=(-1.0, 1.0))
    q, k, v = c["q_hi"].float() * 0.1, c["k_hi"].float() * 0.1, c["v_hi"].float()
    k[0, 170] = 3.0
    q[0, 5] = 3.0
    sign = torch.where(torch.arange(64) % 2 == 0, 1.0, -1.0)
    v[0, 170] = 100.0 * sign
    c["q_hi"], c["k_hi"], c["v_hi"] = (t.to(torch.bfloat16) for t in (q, k, v))
    hi, _, status = _o8_run(c, False)
    assert status & 2
    assert torch.equal(hi[0, 5], 448.0 * sign.double())


def test_attention_unsupported_combinations_are_errors():
    """O8 at head_dim 128 and O8 with a bias have no kernel: an error status with a message, nothing launched."""
    for hd, bias in ((128, False), (64, True)):
        c = R.attn_inputs(hd, 1, 1, 64, bias=bias, seed=52)
        d = hd
        qk = _rows(1, 64, 2 * d, torch.cat([c["q_hi"], c["k_hi"]], -1))
        v = _rows(1, 64, d, c["v_hi"])
        o8 = torch.full((qk.R, d), 0x55, dtype=torch.uint8, device="cuda")
        rc = G.attention_ex(qk.buf, 2 * d, qk.lead, v.buf, 0, d, None, d, 1, 64, qk.P, 1, d, bias=c["table"].cuda() if bias else None,
                            gate=c["gate"].cuda() if bias else None, O8=o8, ldo8=d, o8_scale=64.0, check=False)
        torch.cuda.synchronize()
        assert rc != 0 and b"wfl_op_attention_ex" in G.lib().wfl_last_error()
        assert bool((o8 == 0x55).all())
    # fields the dispatch would otherwise pass over in silence: low halves beside the fp8 context, split precision at a head size
    # that has no split kernel (head_dim 384 runs, without them)
    for hd, fp8 in ((64, True), (384, False)):
        c = R.attn_inputs(hd, 1, 1, 64, pair=True, seed=53)
        d = hd
        qk, qkl = (_rows(1, 64, 2 * d, torch.cat([c["q" + s], c["k" + s]], -1)) for s in ("_hi", "_lo"))
        v, vl = _rows(1, 64, d, c["v_hi"]), _rows(1, 64, d, c["v_lo"])
        o, ol = _rows(1, 64, d), _rows(1, 64, d)
        o8 = torch.full((qk.R, d), 0x55, dtype=torch.uint8, device="cuda")
        rc = G.attention_ex(qk.buf, 2 * d, qk.lead, v.buf, 0, d, None if fp8 else o.buf, d, 1, 64, qk.P, 1, d, QK_lo=qkl.buf, V_lo=vl.buf,
                            O_lo=None if fp8 else ol.buf, O8=o8 if fp8 else None, ldo8=d, o8_scale=64.0, check=False)
        torch.cuda.synchronize()
        assert rc != 0 and b"wfl_op_attention_ex" in G.lib().wfl_last_error()
        assert bool((o8 == 0x55).all()) and bool((o.get() == SENT).all()) and bool((ol.get() == SENT).all())


# ------------------------------------------------------------------------------------------------------ table, gate, regroup
@pytest.mark.parametrize("T", [1, 64, 257])
def test_relpos_table_is_the_gather(T):
    heads, max_t, nb = 3, 300, 32
    g = torch.Generator().manual_seed(60 + T)
    rel_emb = torch.randn(nb, heads, generator=g)
    bod = torch.randint(0, nb, (2 * max_t - 1,), generator=g, dtype=torch.int32)
    n = heads * (2 * T - 1)
    table = torch.full((n + 64,), SENT, device="cuda")
    G.relpos_table(rel_emb.cuda(), bod.cuda(), max_t, heads, T, table)
    torch.cuda.synchronize()
    assert torch.equal(table[:n].cpu().view(heads, 2 * T - 1), R.relpos_table_ref(rel_emb, bod, max_t, T))
    assert bool((table[n:] == SENT).all())


def test_relpos_table_longer_than_the_bucket_table_is_an_error():
    z = torch.zeros(2048, device="cuda")
    rc = G.relpos_table(z, torch.zeros(599, dtype=torch.int32, device="cuda"), 300, 3, 301, z, check=False)
    assert rc != 0 and b"wfl_op_relpos_table" in G.lib().wfl_last_error()


# Measured max |gate - float64 gate| on MI355X (parity_stats.jsonl notes, relpos_gate_*): 4.2e-7 .. 1.1e-6 at hd 32, 5.9e-7 .. 1.3e-6
# at hd 64, 1.3e-6 .. 2.71e-6 at hd 128 (the largest: ldx = d + 64, with x_lo).  The assertion is 4 x the largest, 1.08e-5, far below the 1e-4 at which the gate -- it multiplies bias values of a few units into log2 scores -- would matter beside
# the bf16 rounding of P.
GATE_MEASURED = 2.7065e-6
GATE_TOL = 4 * GATE_MEASURED
assert GATE_TOL < 1e-4


@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("pair", [False, True])
def test_relpos_gate(hd, wide, pair):
    heads, B, T = 3, 2, 257
    d = heads * hd
    ldx = d + 64 if wide else d
    g = torch.Generator().manual_seed(70 + hd)
    x = torch.randn(B, T, ldx, generator=g)                              # (wide: 64 junk columns behind the heads)
    x_hi, x_lo = R.split(x)
    w8, b8 = torch.randn(8, hd, generator=g) * 0.3, torch.randn(8, generator=g) * 0.3
    cst = torch.tensor([0.5, 1.0, 1.7])                                  # distinct per head
    xr = _rows(B, T, ldx, x_hi)
    xl = _rows(B, T, ldx, x_lo) if pair else None
    n = B * heads * T
    gate = torch.full((n + 64,), SENT, device="cuda")
    G.relpos_gate(xr.buf, xl.buf if pair else None, ldx, xr.lead, B, xr.P, T, heads, hd, w8.cuda(), b8.cuda(), cst.cuda(), gate)
    torch.cuda.synchronize()
    val = x_hi.double() + (x_lo.double() if pair else 0.0)
    ref = R.relpos_gate_ref(val[..., :d], heads, w8, b8, cst)
    err = (gate[:n].cpu().double().view(B, heads, T) - ref).abs()
    _note(f"relpos_gate_hd{hd}_wide{int(wide)}_pair{int(pair)}", err_max=err.max())
    assert float(err.max()) <= GATE_TOL, float(err.max())
    assert bool((gate[n:] == SENT).all())


@pytest.mark.parametrize("groups,cpg", [(4, 16), (16, 48), (16, 64)])
@pytest.mark.parametrize("ragged", [False, True])
def test_regroup_is_exact(groups, cpg, ragged):
    B, T, d = 3, 100, groups * cpg
    clip_T = [T, 70, 0] if ragged else None
    g = torch.Generator().manual_seed(80 + cpg)
    x = G.Rows(B, T, d)
    x.buf.copy_(torch.randn(x.R, d, generator=g).to(torch.bfloat16))     # junk in the halo rows too
    xg = torch.full((groups, x.R, 64), SENT, dtype=torch.bfloat16, device="cuda")
    G.regroup(x.buf, d, groups, cpg, x.R, x.lead, B, x.P, T, xg, G._i32(clip_T))
    torch.cuda.synchronize()
    # (the reference is zero in every padding channel, every halo row and every frame >= clip_T[b])
    assert torch.equal(xg.cpu(), R.regroup_ref(x.buf.cpu(), groups, cpg, x.lead, B, x.P, T, clip_T))


# ------------------------------------------------------------------------------------------------------------- positional conv
# c: measured max(err / mag) of the pair output on MI355X (parity_stats.jsonl notes, posconv_*_pair1), the same with and without clip_T:
#   (4, 16, 16)  2.33e-6     (16, 48, 128)  7.2e-7     (2, 64, 128)  4.9e-7
# None exceeds test_gemm_split's 4e-6 although K reaches 8192 here against 2048 there, so ops_ref.POSCONV_C stays 4e-6.


@functools.lru_cache(maxsize=None)
def _posconv_ref(groups, cpg, taps, ragged, pair):
    c = R.posconv_case(groups, cpg, taps, pair)
    return R.posconv_ref(c["x_hi"].double(), c["x_hi"].double() + c["x_lo"].double(), c["W"], c["bias"], cpg, taps,
                         R.POSCONV_CLIP_T if ragged else None, with_mag=True)


@pytest.mark.parametrize("groups,cpg,taps", R.POSCONV_CASES)
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("pair", [False, True])
def test_posconv(groups, cpg, taps, ragged, pair):
    """x + gelu(grouped conv) on rows regrouped by the regroup export; B * P = 736 > 256: a workgroup's 256 frames straddle the clips.
    Row geometry as make_plan gives a WavLM model: lead and the halo between clips both >= taps / 2."""
    c = R.posconv_case(groups, cpg, taps, pair)
    B, T, d = c["B"], c["T"], c["d"]
    clip_T = R.POSCONV_CLIP_T if ragged else None
    x = _rows(B, T, d, c["x_hi"], halo=64, lead=64)
    xl = _rows(B, T, d, c["x_lo"], halo=64, lead=64) if pair else None
    xg = torch.full((groups, x.R, 64), SENT, dtype=torch.bfloat16, device="cuda")
    G.regroup(x.buf, d, groups, cpg, x.R, x.lead, B, x.P, T, xg, G._i32(clip_T))
    out = _rows(B, T, d, halo=64, lead=64)
    outl = _rows(B, T, d, halo=64, lead=64) if pair else None
    W, bias = c["W"].cuda().contiguous(), c["bias"].cuda().contiguous()
    G.posconv(xg, x.R, x.lead, B, x.P, T, groups, cpg, taps, W, taps * 64, bias, x.buf, xl.buf if pair else None, out.buf,
              outl.buf if pair else None, d, G._i32(clip_T))
    torch.cuda.synchronize()
    ref, mag = _posconv_ref(groups, cpg, taps, ragged, pair)
    got = out.get().double().cpu() + (outl.get().double().cpu() if pair else 0.0)
    m = _valid(B, T, clip_T)
    err = (got - ref).abs()[m]
    _note(f"posconv_g{groups}_c{cpg}_k{taps}_ragged{int(ragged)}_pair{int(pair)}", err_over_mag_max=(err / mag[m]).max(), err_max=err.max())
    _within(got[m], ref[m], R.posconv_bound(ref, mag, pair)[m], "posconv")
    for r in (out, outl) if pair else (out,):
        assert r.halo_is_zero() and bool((r.get().cpu()[~m] == SENT).all())


def test_posconv_launcher_rules_are_errors():
    """lead < taps / 2, odd taps, cpg % 8: the launcher does not take the shape, and the export says so instead of running nothing."""
    z = torch.zeros(1 << 16, dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(1024, device="cuda")
    for lead, taps, cpg in ((8, 128, 16), (64, 15, 16), (64, 16, 12)):
        rc = G.posconv(z, 16, lead, 1, 8, 4, 2, cpg, taps, z, 128 * 64, f, z, None, z, None, 2 * cpg, check=False)
        assert rc != 0 and b"wfl_op_posconv" in G.lib().wfl_last_error()


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
# lambda: measured max(err / scale) of the pair output on MI355X (parity_stats.jsonl notes, layernorm_act_*), scale as derived at
# ops_ref.LN_LAMBDA:
#   C 64  4.77e-6 / 4.89e-6 (GELU)     C 768  5.43e-6 / 5.12e-6     C 1280  5.41e-6 / 5.14e-6     C 2048  5.716e-6 / 5.37e-6
#   C 128 (n_div 80)  5.01e-6 / 4.54e-6     N(30, 1) rows, C 768  7.5e-7
# ops_ref.LN_LAMBDA = 4 x the largest = 2.29e-5.  (Against the scale without the row term, |gamma| |x - mean| rstd + |beta|, the same runs
# gave up to 4.9e-5, and 1.9e-3 on the N(30, 1) rows: elements next to the row mean.)


def _ln_run(c, gelu, pair, inplace, clip_T):
    """One wfl_op_layernorm_act launch on a case of ops_ref.layernorm_inputs.  -> (y rows, y_lo rows or None)."""
    B, T, Cn = c["B"], c["T"], c["C"]
    x = _rows(B, T, Cn, c["x_hi"])
    xl = _rows(B, T, Cn, c["x_lo"]) if pair else None
    y = x if inplace else _rows(B, T, Cn)
    yl = (xl if inplace else _rows(B, T, Cn)) if pair else None
    G.layernorm_act(x.buf, xl.buf if pair else None, y.buf, yl.buf if pair else None, c["gamma"].cuda(), c["beta"].cuda(), 1e-5, x.lead, B,
                    x.P, T, Cn, c["n_div"], int(gelu), G._i32(clip_T))
    torch.cuda.synchronize()
    return y, yl


def _ln_check(c, gelu, pair, inplace, clip_T, name):
    B, T = c["B"], c["T"]
    y, yl = _ln_run(c, gelu, pair, inplace, clip_T)
    val = c["x_hi"].double() + (c["x_lo"].double() if pair else 0.0)
    ref, scale = R.layernorm_ref(val, c["gamma"], c["beta"], 1e-5, c["n_div"], gelu, with_scale=True)
    got = y.get().double().cpu() + (yl.get().double().cpu() if pair else 0.0)
    m = _valid(B, T, clip_T)
    err = (got - ref).abs()[m]
    if pair:
        ok = scale[m] > 0
        _note(name, err_over_scale_max=(err[ok] / scale[m][ok]).max(), err_max=err.max())
    _within(got[m], ref[m], R.layernorm_bound(ref, scale, pair)[m], name)
    if c["n_div"]:
        assert bool((got[m][..., c["n_div"]:] == 0).all())                    # zero gamma / beta: the padding columns come out zero
    # rows the launch must leave alone: the sentinel, or -- in place -- the input itself
    keep_hi = c["x_hi"].float() if inplace else torch.full_like(c["x_hi"].float(), SENT)
    assert y.halo_is_zero() and torch.equal(y.get().cpu()[~m], keep_hi[~m])
    if pair:
        keep_lo = c["x_lo"].float() if inplace else torch.full_like(c["x_lo"].float(), SENT)
        assert yl.halo_is_zero() and torch.equal(yl.get().cpu()[~m], keep_lo[~m])


@pytest.mark.parametrize("C,n_div", [(64, 0), (768, 0), (1280, 0), (2048, 0), (128, 80)])
@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("pair", [False, True])
def test_layernorm_act(C, n_div, gelu, pair):
    """Out of place over whole clips, and in place (y == x, as the WavLM feature encoder calls it) with clip_T = [211, 70, 0]."""
    c = R.layernorm_inputs(C, n_div, 3, R.LN_T, pair)
    name = f"layernorm_act_C{C}_gelu{int(gelu)}_pair{int(pair)}"
    _ln_check(c, gelu, pair, False, None, name)
    _ln_check(c, gelu, pair, True, R.LN_CLIP_T, name + "_inplace_ragged")


@pytest.mark.parametrize("pair", [False, True])
def test_layernorm_act_common_offset(pair):
    """mean 30, std 1: a variance taken as E[x^2] - mean^2 in fp32 would lose it; the kernel's is centred."""
    c = R.layernorm_inputs(768, 0, 3, R.LN_T, pair, offset=True)
    _ln_check(c, False, pair, False, None, f"layernorm_act_offset_pair{int(pair)}")


@pytest.mark.parametrize("C,n_div", [(128, 80), (512, 0), (1280, 0)])
@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("alias", [False, True])
def test_layernorm_pair_is_two_layernorm_launches(C, n_div, pair, ragged, alias):
    """norm.hip's stated contract: y1, y2 and their low halves are bit for bit what two layernorm_kernel launches write.  No tolerance."""
    c = R.layernorm_inputs(C, n_div, 3, R.LN_T, pair)
    B, T = c["B"], c["T"]
    clip_T = G._i32(R.LN_CLIP_T) if ragged else None
    g1, b1, g2, b2 = (c[k].float().cuda() for k in ("gamma", "beta", "gamma2", "beta2"))
    mk = lambda x=None: _rows(B, T, C, x)                                       # noqa: E731
    # two launches
    x, xl = mk(c["x_hi"]), (mk(c["x_lo"]) if pair else None)
    a1, a1l, a2, a2l = mk(), (mk() if pair else None), mk(), (mk() if pair else None)
    lo = lambda r: r.buf if r is not None else None                             # noqa: E731
    G.layernorm_act(x.buf, lo(xl), a1.buf, lo(a1l), g1, b1, 1e-5, x.lead, B, x.P, T, C, n_div, 0, clip_T)
    G.layernorm_act(a1.buf, lo(a1l), a2.buf, lo(a2l), g2, b2, 1e-5, x.lead, B, x.P, T, C, n_div, 0, clip_T)
    # one launch; alias: y2 is x (and y2_lo is x_lo)
    y1, y1l = mk(), (mk() if pair else None)
    y2, y2l = (x, xl) if alias else (mk(), (mk() if pair else None))
    x_before = x.buf.clone()
    G.layernorm_pair(x.buf, lo(xl), y1.buf, lo(y1l), y2.buf, lo(y2l), g1, b1, g2, b2, 1e-5, x.lead, B, x.P, T, C, n_div, clip_T)
    torch.cuda.synchronize()
    assert torch.equal(y1.buf, a1.buf) and (not pair or torch.equal(y1l.buf, a1l.buf))
    if alias:
        # rows the launch leaves alone hold x there, the sentinel in the two-launch output
        m = _valid(B, T, R.LN_CLIP_T if ragged else None)
        assert torch.equal(y2.get().cpu()[m], a2.get().cpu()[m]) and (not pair or torch.equal(y2l.get().cpu()[m], a2l.get().cpu()[m]))
        rows = G.Rows(B, T, C)
        rows.buf = x_before
        assert torch.equal(y2.get().cpu()[~m], rows.get().cpu()[~m])
    else:
        assert torch.equal(y2.buf, a2.buf) and (not pair or torch.equal(y2l.buf, a2l.buf))
    for r in (y1, y1l, y2, y2l):
        assert r is None or r.halo_is_zero()
