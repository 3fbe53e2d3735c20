"""-m gpu: the streaming GEMM's epilogue, the attention's score accumulators and the Conformer block's LayerNorm pair after the
vector-ALU work their results do not need was taken out.

1. Bit identity of the whole model against tests/golden/epilogue_parent.npz, recorded from the build before that change by
   tests/golden/make_epilogue_parent.py (cases: tests/epilogue_cases.py): ids, argmax, and the bit patterns of maxprob and offsets.
2. The operators alone, through the C ABI, at shapes that reach both copies of the epilogue -- M = 12 500 rows, K = 256, with N = 1024
   (66 row tiles x 4 column tiles = 264 tiles for 256 persistent workgroups: eight of them run the in-loop epilogue; the last row tile is
   partial) and with N = 512 (132 tiles: the final epilogue only) -- against the float64 product, with the bounds tests/test_gpu_ops.py
   uses for the same operators (2e-2 relative + 2e-2 absolute for a GEMM, 2e-2 + 1e-2 for the attention)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gpu_util as G
import epilogue_cases as E

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. the model, bit for bit

@pytest.fixture(scope="module")
def model_runs():
    m = E.build_model()
    wav6 = E.clips(6)
    return {name: E.run_case(m, wav6, name) for name in E.CASES}


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_model_outputs_equal_the_parent_build_bit_for_bit(name, model_runs, golden_dir):
    want = np.load(os.path.join(golden_dir, "epilogue_parent.npz"))
    got = model_runs[name]
    for k in ("ids", "argmax", "maxprob", "offsets"):
        w = want[f"{name}.{k}"]
        assert got[k].shape == w.shape and got[k].dtype == w.dtype, (name, k)
        nd = int((got[k] != w).sum())
        assert nd == 0, f"{name}.{k}: {nd} of {w.size} elements differ from the parent build's"


def test_a_clip_alone_equals_the_clip_inside_a_batch(model_runs):
    """b1 runs only the final epilogue of every launch, b6 the in-loop copy as well: the two copies must agree."""
    for k in ("ids", "argmax", "maxprob", "offsets"):
        assert np.array_equal(model_runs["b1"][k][0], model_runs["b6"][k][0]), k


# ------------------------------------------------------------------------------------------------ 2. the operators

def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _bf64(x):
    return x.to(torch.bfloat16).double()


def _close(got, want, rtol=2e-2, atol=2e-2, what=""):
    err = (got.double() - want).abs()
    lim = atol + rtol * want.abs()
    print(f"{what}: max err {err.max().item():.4g}, worst excess over the bound {(err - lim).max().item():.4g}")
    assert bool((err <= lim).all()), f"{what}: max err {err.max().item():.4g}, worst excess {(err - lim).max().item():.4g}"


M_ROWS, K_IN, B_, T_, P_ = 12500, 256, 5, 2490, 2504       # five clips of 2 490 frames, 2 504 rows apart: M stops inside the last clip


def _gelu64(y):
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


@pytest.fixture(scope="module")
def gemm_operands():
    x0 = _rand(B_, T_, K_IN, seed=101) * 2.0 + 0.5
    x0[..., 3] += 9.0                                          # an outlier channel, as real encoder states have
    a = G.Rows(B_, T_, K_IN, pitch=P_).set(x0)
    w = _rand(1024, K_IN, scale=K_IN ** -0.5, seed=102)
    bias = _rand(1024, scale=0.1, seed=103)
    r0 = _rand(B_, T_, 1024, seed=104)
    gamma, beta = 1.0 + 0.2 * _rand(K_IN, seed=105), 0.1 * _rand(K_IN, seed=106)
    valid = torch.zeros(B_, T_, dtype=torch.bool, device="cuda")            # frames with a flat row index below M
    for b in range(B_):
        valid[b, :max(0, min(T_, M_ROWS - b * P_))] = True
    assert int(valid.sum()) == 4 * T_ + (M_ROWS - 4 * P_)
    assert ((M_ROWS + 191) // 192) * 4 == 264 and M_ROWS % 192 != 0
    x64 = a.get().double()
    return dict(a=a, w=w, bias=bias, r0=r0, gamma=gamma, beta=beta, valid=valid, x64=x64,
                y64=x64 @ _bf64(w).T + bias.double())                       # the float64 product, shared by the cases below


def _check_rows(out, ref, valid, N, what):
    got = out.get()
    _close(got[valid][:, :N], ref[valid][:, :N], what=what)
    assert bool((got[~valid] == 0).all()) and out.halo_is_zero(), what + ": rows outside the launch were written"


@pytest.mark.parametrize("N", [1024, 512])
@pytest.mark.parametrize("form", ["gelu", "residual", "ln_gelu"])
def test_stream_gemm_epilogue_forms(form, N, gemm_operands):
    o = gemm_operands
    a, valid = o["a"], o["valid"]
    if form == "ln_gelu":
        wf = (o["w"][:N] * o["gamma"]).to(torch.bfloat16)
        ln_s = wf.float().sum(1).contiguous()
        bfold = o["bias"][:N] + o["w"][:N] @ o["beta"]
        wp, bp = G.pad_weight(wf.float(), bfold)
        out = G.Rows(B_, T_, N, pitch=P_)
        G.gemm_ln(a.buf, a.lead * K_IN, K_IN, wp, M_ROWS, N, P_, T_, out.buf, N, out.lead, P_, bp, ln_s, 1e-5, 1)
        torch.cuda.synchronize()
        ln = F.layer_norm(o["x64"], (K_IN,), o["gamma"].double(), o["beta"].double(), 1e-5)
        ref = _gelu64(ln @ o["w"][:N].double().T + o["bias"][:N].double())
        _check_rows(out, ref, valid, N, f"LN-folded GELU GEMM N={N}")
        return
    wp, bp = G.pad_weight(o["w"][:N], o["bias"][:N])
    y64 = o["y64"][..., :N]
    if form == "gelu":
        out = G.Rows(B_, T_, N, pitch=P_)
        G.gemm(a.buf, a.lead * K_IN, K_IN, wp, M_ROWS, N, P_, T_, out.buf, N, out.lead, P_, bias=bp, act=1)
        torch.cuda.synchronize()
        _check_rows(out, _gelu64(y64), valid, N, f"GELU GEMM N={N}")
    else:
        r0 = o["r0"][..., :N].contiguous()
        x = G.Rows(B_, T_, N, pitch=P_).set(r0)
        G.gemm(a.buf, a.lead * K_IN, K_IN, wp, M_ROWS, N, P_, T_, x.buf, N, x.lead, P_, bias=bp, res=x.buf, ldres=N, alpha=0.5)
        torch.cuda.synchronize()
        got = x.get()
        _close(got[valid], (_bf64(r0) + 0.5 * y64)[valid], what=f"residual GEMM N={N}")
        assert torch.equal(got[~valid], _bf64(r0).float()[~valid]) and x.halo_is_zero()


def test_conv_mode_without_a_low_half_equals_the_high_half_of_the_launch_that_keeps_one():
    """3 taps, cin 256.  The plain launch has no low-half buffer.  The C ABI hands the conv mode one only in its three-segment form
    (wfl_op_gemm_split: [A_hi W_hi | A_lo W_hi | A_hi W_lo]); with A_lo = 0 and W_lo = 0 the second and third segments add exact zeros
    to the accumulators after the first has walked K in the plain launch's order, so its high half must equal the plain output bit for
    bit.  (A sum that is exactly zero could differ in sign; with a bias none is.)  The plain output is also held to the float64 conv."""
    B, T, C, k, N = 3, 700, 256, 3, 512
    x0 = _rand(B, T, C, seed=111)
    a = G.Rows(B, T, C, halo=32, lead=32).set(x0)
    w, bias = _rand(N, C, k, scale=(k * C) ** -0.5, seed=112), _rand(N, scale=0.1, seed=113) + 0.5
    wp, bp = G.pad_weight(w.permute(0, 2, 1).reshape(N, k * C), bias)
    assert wp.shape == (N, k * C)
    plain = G.Rows(B, T, N, halo=32, lead=32)
    G.gemm(a.buf, (a.lead - 1) * C, C, wp, B * a.P, N, a.P, T, plain.buf, N, plain.lead, plain.P, bias=bp, act=1, cin=C, tap_stride=C)
    torch.cuda.synchronize()
    ref = _gelu64(F.conv1d(_bf64(x0).transpose(1, 2), _bf64(w), bias.double(), padding=1).transpose(1, 2))
    _close(plain.get(), ref, what="conv mode, no low half")
    assert plain.halo_is_zero()
    both = torch.zeros(2 * a.R, C, dtype=torch.bfloat16, device="cuda")         # hi rows, then an all-zero low half
    both[:a.R] = a.buf
    w3 = torch.cat([wp, wp, torch.zeros_like(wp)], 1).contiguous()
    hi, lo = G.Rows(B, T, N, halo=32, lead=32), G.Rows(B, T, N, halo=32, lead=32)
    rc = G.lib().wfl_op_gemm_split(G.ptr(both, (a.lead - 1) * C), G.ptr(both, (a.R + a.lead - 1) * C), C, C, C, G.ptr(w3), B * a.P, N, k * C, N,
                                   a.P, T, G.ptr(hi.buf), G.ptr(lo.buf), N, hi.lead, hi.P, G.ptr(bp), None, None, 0, 1.0, 1, 0, G.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(hi.buf.view(torch.int16), plain.buf.view(torch.int16))
    assert float((lo.get().abs()).max()) > 0.0 and lo.halo_is_zero()            # (the launch did keep a low half)
    _close(hi.get().double() + lo.get().double(), ref, rtol=2e-4, atol=2e-4, what="hi + lo")   # 16 significant bits against 8


@pytest.mark.parametrize("d,heads,T", [(128, 2, 200), (512, 2, 300)])
def test_attention_against_the_float64_softmax(d, heads, T):
    """head_dim 64 with a masked last key tile (T = 200 = 3 x 64 + 8) and head_dim 256 (T = 300: masked too)."""
    B, hd = 2, d // heads
    q = _rand(B, T, d, seed=121) * (hd ** -0.25) * 1.5
    k = _rand(B, T, d, seed=122) * (hd ** -0.25) * 1.5
    v = _rand(B, T, d, seed=123)
    qkv = G.Rows(B, T, 3 * d).set(torch.cat([q, k, v], -1))
    o = G.Rows(B, T, d)
    G.attention(qkv.buf, 3 * d, qkv.lead, qkv.buf, 2 * d, 3 * d, o.buf, d, B, T, qkv.P, heads, d)
    torch.cuda.synchronize()
    x = qkv.get().double()
    qh = x[..., :d].view(B, T, heads, hd).transpose(1, 2) * math.log(2.0)        # scores are in log2 units
    kh = x[..., d:2 * d].view(B, T, heads, hd).transpose(1, 2)
    vh = x[..., 2 * d:].view(B, T, heads, hd).transpose(1, 2)
    ref = (torch.softmax(qh @ kh.transpose(2, 3), -1) @ vh).transpose(1, 2).reshape(B, T, d)
    _close(o.get(), ref, rtol=2e-2, atol=1e-2, what=f"attention head_dim {hd}")
    assert o.halo_is_zero()
