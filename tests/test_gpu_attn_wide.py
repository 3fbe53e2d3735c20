"""-m gpu: head_dim 256 attention with K / V tiles shared by 8 or 12 waves of one workgroup (attention.hip, `NW`).  A wave does
exactly what it does in the 4-wave form, which WFL_ATTN_WAVES=4 still selects at every launch, so every byte of the output buffer
must be the same in both forms; the wide form is also held to a float64 softmax(q k^T) v of the bf16-rounded inputs within the
bound of test_gpu_ops.test_qkv_projection_and_attention (rtol 2e-2, atol 1e-2).
Shapes: d = 512, 2 heads, B = 3, pitch > T, halos.  T covers one query, a wave with no valid query, one to three key tiles with
tails, a fifth key tile, and exactly / one under / one over a block of 128 and of 192 queries.
The split-precision kernel (QK_lo / V_lo / O_lo, "model.precision: high") has an eight-wave form too: the same identity on O and O_lo,
and O + O_lo within ops_ref.attn_bound_split of the float64 reference over the hi + lo operands (the bound of
test_gpu_ops_wavlm.test_attention_split_precision)."""
import functools
import math

import pytest
import torch

import gpu_util as G
import ops_ref as R

pytestmark = pytest.mark.gpu

D, HEADS, B = 512, 2, 3
HD = D // HEADS
POISON = 777.0                                   # (exact in bf16)
T_CASES = [1, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257]
WIDE_FORMS = [None, "8", "12"]                   # WFL_ATTN_WAVES: unset = the shipped default


@functools.lru_cache(maxsize=None)
def _inputs(T):
    """q|k|v rows for B clips of T frames (CPU, float, already bf16-rounded) -- made once per T and left unchanged."""
    g = torch.Generator(device="cpu").manual_seed(1000 + T)
    x = torch.randn(B, T, 3 * D, generator=g)
    x[..., :D] *= 0.25                           # scores ~ N(0, 4^2) in log2 units: a few rows cross the rescale threshold
    return x.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def _reference(T, clip_T=None):
    """float64 softmax(q k^T) v per (clip, head); exp2 scores as the kernel has them (q is pre-scaled at weight-pack time).
    -> [B, T, D] float32 on the CPU, rows >= the clip's length zero."""
    x = _inputs(T).double()
    ref = torch.zeros(B, T, D, dtype=torch.float64)
    for b in range(B):
        n = clip_T[b] if clip_T else T
        for h in range(HEADS):
            q = x[b, :n, h * HD:(h + 1) * HD]
            k = x[b, :n, D + h * HD:D + (h + 1) * HD]
            v = x[b, :n, 2 * D + h * HD:2 * D + (h + 1) * HD]
            ref[b, :n, h * HD:(h + 1) * HD] = torch.softmax(q @ k.T * math.log(2.0), -1) @ v
    return ref.float()


def _select(monkeypatch, waves):
    if waves is None:
        monkeypatch.delenv("WFL_ATTN_WAVES", raising=False)
    else:
        monkeypatch.setenv("WFL_ATTN_WAVES", waves)


def _run(monkeypatch, waves, T, clip_T=None):
    """one launch into a poisoned output buffer -> the output rows."""
    _select(monkeypatch, waves)
    qkv = G.Rows(B, T, 3 * D).set(_inputs(T).cuda())
    o = G.Rows(B, T, D)
    o.buf.fill_(POISON)
    ct = G._i32(clip_T)
    if clip_T is None:
        G.attention(qkv.buf, 3 * D, qkv.lead, qkv.buf, 2 * D, 3 * D, o.buf, D, B, T, qkv.P, HEADS, D)
    else:
        G.attention_ex(qkv.buf, 3 * D, qkv.lead, qkv.buf, 2 * D, 3 * D, o.buf, D, B, T, qkv.P, HEADS, D, clip_T=ct)
    torch.cuda.synchronize()
    return o


def _check_poison(o, T, clip_T=None):
    v = o.buf[o.lead:o.lead + B * o.P].view(B, o.P, D)
    for b in range(B):
        n = clip_T[b] if clip_T else T
        assert bool((v[b, n:] == POISON).all()), f"clip {b}: a row >= {n} was written"
    assert bool((o.buf[:o.lead] == POISON).all()) and bool((o.buf[o.lead + B * o.P:] == POISON).all()), "lead / tail rows written"


def _close(got, want, rtol, atol, what):
    err = (got - want).abs()
    lim = atol + rtol * want.abs()
    print(f"{what}: max err {err.max().item():.4g}, worst excess {(err - lim).max().item():.4g}")
    assert bool((err <= lim).all()), f"{what}: max err {err.max().item():.4g}, worst excess {(err - lim).max().item():.4g}"


def _both_forms(monkeypatch, waves, T, clip_T=None):
    wide = _run(monkeypatch, waves, T, clip_T)
    four = _run(monkeypatch, "4", T, clip_T)
    assert wide.P > T
    _check_poison(four, T, clip_T)
    _check_poison(wide, T, clip_T)
    assert torch.equal(wide.buf, four.buf), f"WFL_ATTN_WAVES={waves or 'default'} differs from the 4-wave form"
    got = wide.get().cpu()
    if clip_T:
        for b in range(B):
            got[b, clip_T[b]:] = 0
    _close(got, _reference(T, clip_T), 2e-2, 1e-2, f"T {T} waves {waves or 'default'}")


@pytest.mark.parametrize("waves", WIDE_FORMS)
@pytest.mark.parametrize("T", T_CASES)
def test_wide_equals_four_wave_form_and_float64(monkeypatch, T, waves):
    _both_forms(monkeypatch, waves, T)


@pytest.mark.parametrize("waves", WIDE_FORMS)
def test_wide_ragged_batch(monkeypatch, waves):
    """clips of 193, 1 and 64 frames inside a batch-wide T = 193: blocks that return early, blocks whose last waves are empty."""
    _both_forms(monkeypatch, waves, 193, clip_T=(193, 1, 64))


# ---- split precision: four waves against eight (the default), single-buffered both

@functools.lru_cache(maxsize=None)
def _split_case(T):
    c = R.attn_inputs(HD, HEADS, B, T, pair=True, seed=300 + T)
    return c, R.attn_case_ref(c)


def _run_split(monkeypatch, waves, T):
    _select(monkeypatch, waves)
    c, _ = _split_case(T)
    qk = G.Rows(B, T, 2 * D).set(torch.cat([c["q_hi"], c["k_hi"]], -1).cuda())
    qkl = G.Rows(B, T, 2 * D).set(torch.cat([c["q_lo"], c["k_lo"]], -1).cuda())
    v, vl = G.Rows(B, T, D).set(c["v_hi"].cuda()), G.Rows(B, T, D).set(c["v_lo"].cuda())
    o, ol = G.Rows(B, T, D), G.Rows(B, T, D)
    o.buf.fill_(POISON)
    ol.buf.fill_(POISON)
    G.attention_ex(qk.buf, 2 * D, qk.lead, v.buf, 0, D, o.buf, D, B, T, qk.P, HEADS, D, QK_lo=qkl.buf, V_lo=vl.buf, O_lo=ol.buf)
    torch.cuda.synchronize()
    return o, ol


@pytest.mark.parametrize("waves", [None, "8"])
@pytest.mark.parametrize("T", [65, 129, 193])
def test_wide_split_precision(monkeypatch, T, waves):
    o, ol = _run_split(monkeypatch, waves, T)
    o4, ol4 = _run_split(monkeypatch, "4", T)
    for r in (o, ol, o4, ol4):
        _check_poison(r, T)
    assert torch.equal(o.buf, o4.buf) and torch.equal(ol.buf, ol4.buf), f"WFL_ATTN_WAVES={waves or 'default'} differs from the 4-wave form"
    ref, A = _split_case(T)[1]
    got = o.get().double().cpu() + ol.get().double().cpu()
    err = (got - ref).abs()
    bound = R.attn_bound_split(ref, A)
    print(f"split T {T} waves {waves or 'default'}: max err {float(err.max()):.4g}, worst excess {float((err - bound).max()):.4g}")
    assert bool((err <= bound).all()), f"max err {float(err.max()):.4g}, worst excess {float((err - bound).max()):.4g}"
