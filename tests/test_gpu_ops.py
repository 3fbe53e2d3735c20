"""-m gpu: each HIP kernel, called through the C ABI, against a plain PyTorch fp32 computation of the same op on
the same bf16-rounded operands.  Tolerances are stated per test (bf16 output rounding = 2^-9 relative)."""
import math

import pytest
import torch
import torch.nn.functional as F

import gpu_util as G

pytestmark = pytest.mark.gpu


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _bf(x):
    return x.to(torch.bfloat16).float()


def _close(got, want, rtol=2e-2, atol=2e-2, what=""):
    err = (got - want).abs()
    lim = atol + rtol * want.abs()
    assert bool((err <= lim).all()), f"{what}: max err {err.max().item():.4g}, worst excess {(err - lim).max().item():.4g}"


@pytest.mark.parametrize("B,T,K,N", [(2, 200, 64, 128), (3, 301, 512, 512), (1, 1500, 256, 141), (16, 100, 2048, 512)])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_gemm_linear(B, T, K, N, act):
    a = G.Rows(B, T, K).set(_rand(B, T, K, seed=1))
    w, bias = _rand(N, K, scale=K ** -0.5, seed=2), _rand(N, scale=0.1, seed=3)
    wp, bp = G.pad_weight(w, bias)
    out = G.Rows(B, T, (N + 7) // 8 * 8)
    G.gemm(a.buf, a.lead * K, K, wp, B * a.P, N, a.P, T, out.buf, out.C, out.lead, out.P, bias=bp, act=act)
    torch.cuda.synchronize()
    ref = a.get() @ _bf(w).T + bias
    ref = [ref, F.gelu(ref), F.relu(ref), torch.sigmoid(ref)][act]
    _close(out.get()[..., :N], ref, what="gemm")
    assert out.halo_is_zero()
    if out.C > N:
        assert bool((out.get()[..., N:] == 0).all())


def test_gemm_residual_alpha_inplace_and_f32():
    B, T, K, N = 2, 333, 512, 512
    a = G.Rows(B, T, K).set(_rand(B, T, K, seed=4))
    x0 = _rand(B, T, N, seed=5)
    x = G.Rows(B, T, N).set(x0)
    w, bias = _rand(N, K, scale=K ** -0.5, seed=6), _rand(N, scale=0.1, seed=7)
    wp, bp = G.pad_weight(w, bias)
    G.gemm(a.buf, a.lead * K, K, wp, B * a.P, N, a.P, T, x.buf, N, x.lead, x.P, bias=bp, res=x.buf, ldres=N, alpha=0.5)
    torch.cuda.synchronize()
    ref = _bf(x0) + 0.5 * (a.get() @ _bf(w).T + bias)
    _close(x.get(), ref, what="residual")
    # fp32 compact output, ragged N (the classifier's shape)
    Nc = 141
    wc, bc = _rand(Nc, K, scale=0.3, seed=8), _rand(Nc, seed=9)
    wcp, bcp = G.pad_weight(wc, bc)
    lg = torch.full((B * T, Nc), float("nan"), device="cuda")
    G.gemm(a.buf, a.lead * K, K, wcp, B * a.P, Nc, a.P, T, lg, Nc, 0, T, bias=bcp, out_f32=1)
    torch.cuda.synchronize()
    ref = (a.get() @ _bf(wc).T + bc).reshape(B * T, Nc)
    _close(lg, ref, rtol=1e-3, atol=1e-3, what="f32 out")


@pytest.mark.parametrize("C,k,dil", [(64, 3, 1), (512, 31, 1), (128, 3, 2), (64, 5, 4)])
def test_gemm_conv_taps(C, k, dil):
    B, T, N = 2, 257, 128
    pad = dil * (k - 1) // 2
    halo = max(16, (pad + 8) // 8 * 8)
    x0 = _rand(B, T, C, seed=10)
    a = G.Rows(B, T, C, halo=halo, lead=halo).set(x0)
    w, bias = _rand(N, C, k, scale=(C * k) ** -0.5, seed=11), _rand(N, scale=0.1, seed=12)
    rows = w.permute(0, 2, 1).reshape(N, k * C)                 # tap-major
    wp, bp = G.pad_weight(rows, bias)
    out = G.Rows(B, T, N, halo=halo, lead=halo)
    if dil == 1:
        G.gemm(a.buf, (a.lead - pad) * C, C, wp, B * a.P, N, a.P, T, out.buf, N, out.lead, out.P, bias=bp)
    else:
        G.gemm(a.buf, (a.lead - pad) * C, C, wp, B * a.P, N, a.P, T, out.buf, N, out.lead, out.P, bias=bp, cin=C, tap_stride=dil * C)
    torch.cuda.synchronize()
    ref = F.conv1d(_bf(x0).transpose(1, 2), _bf(w), bias, padding=pad, dilation=dil).transpose(1, 2)
    _close(out.get(), ref, what="conv")


def test_gemm_conv_stride2_and_pos():
    # the Whisper stem's second conv: k3 s2 p1 on rows whose pitch is twice the output pitch, + positional table
    B, T, C, N = 2, 150, 64, 128
    out = G.Rows(B, T, N, halo=18, lead=16)            # P = 168
    Tin, Pin = 2 * T, 2 * out.P
    x0 = _rand(B, Tin, C, seed=13)
    a = G.Rows(B, Tin, C, lead=8, pitch=Pin, tail=512).set(x0)
    w, bias = _rand(N, C, 3, scale=(3 * C) ** -0.5, seed=14), _rand(N, scale=0.1, seed=15)
    wp, bp = G.pad_weight(w.permute(0, 2, 1).reshape(N, 3 * C), bias)
    pos = _rand(T, N, seed=16).to(torch.bfloat16)
    lib = G.lib()
    # wfl_op_gemm has no `pos` argument: here the table goes in as the residual input (the same add, alpha = 1).  GemmArgs::pos itself is
    # tested behind this conv in test_gpu_ops_gemm_modes.py::test_positional_table_behind_the_stride2_conv (wfl_op_gemm_ex)
    posrows = G.Rows(B, T, N, halo=18, lead=16).set(pos.float().expand(B, T, N))
    G.gemm(a.buf, (a.lead - 1) * C, 2 * C, wp, B * out.P, N, out.P, T, out.buf, N, out.lead, out.P, bias=bp, act=1,
           res=posrows.buf, ldres=N, alpha=1.0)
    torch.cuda.synchronize()
    ref = F.gelu(F.conv1d(_bf(x0).transpose(1, 2), _bf(w), bias, stride=2, padding=1)).transpose(1, 2) + pos.float()
    _close(out.get(), ref, what="conv s2")


def test_gemm_glu():
    B, T, d = 2, 130, 128
    x0 = _rand(B, T, d, seed=17)
    a = G.Rows(B, T, d).set(x0)
    w, bias = _rand(2 * d, d, scale=d ** -0.5, seed=18), _rand(2 * d, scale=0.2, seed=19)
    rows = torch.empty_like(w)
    brow = torch.empty_like(bias)
    for g in range(d // 16):
        rows[32 * g:32 * g + 16] = w[16 * g:16 * g + 16]
        rows[32 * g + 16:32 * g + 32] = w[d + 16 * g:d + 16 * g + 16]
        brow[32 * g:32 * g + 16] = bias[16 * g:16 * g + 16]
        brow[32 * g + 16:32 * g + 32] = bias[d + 16 * g:d + 16 * g + 16]
    wp, bp = G.pad_weight(rows, brow)
    out = G.Rows(B, T, d)
    G.gemm(a.buf, a.lead * d, d, wp, B * a.P, 2 * d, a.P, T, out.buf, d, out.lead, out.P, bias=bp, glu=1)
    torch.cuda.synchronize()
    ref = F.glu(a.get() @ _bf(w).T + bias, dim=-1)
    _close(out.get(), ref, what="glu")


@pytest.mark.parametrize("d,heads,T", [(64, 2, 100), (128, 2, 257), (512, 8, 1500), (512, 2, 300), (768, 2, 300), (1024, 2, 200),
                                       (1280, 2, 150)])
def test_qkv_projection_and_attention(d, heads, T):
    """packed q|k|v GEMM + flash attention (V read row-major through the transposing LDS read) vs softmax(q k^T / sqrt(hd)) v."""
    B = 2
    hd = d // heads
    x0 = _rand(B, T, d, seed=20)
    a = G.Rows(B, T, d).set(x0)
    w, bias = _rand(3 * d, d, scale=d ** -0.5 * 2.0, seed=21), _rand(3 * d, scale=0.1, seed=22)
    qs = hd ** -0.5 * math.log2(math.e)
    wq = w.clone(); bq = bias.clone()
    wq[:d] *= qs; bq[:d] *= qs
    wp, bp = G.pad_weight(wq, bq)
    qkv = G.Rows(B, T, 3 * d)
    G.gemm(a.buf, a.lead * d, d, wp, B * a.P, 3 * d, a.P, T, qkv.buf, 3 * d, qkv.lead, qkv.P, bias=bp)
    torch.cuda.synchronize()
    proj = a.get() @ _bf(wq).T + bq
    _close(qkv.get(), proj, what="q|k|v")
    assert qkv.halo_is_zero()
    o = G.Rows(B, T, d)
    G.attention(qkv.buf, 3 * d, qkv.lead, qkv.buf, 2 * d, 3 * d, o.buf, d, B, T, a.P, heads, d)
    torch.cuda.synchronize()
    q = qkv.get()[..., :d].view(B, T, heads, hd).transpose(1, 2) / math.log2(math.e)
    k = qkv.get()[..., d:2 * d].view(B, T, heads, hd).transpose(1, 2)
    v = qkv.get()[..., 2 * d:].view(B, T, heads, hd).transpose(1, 2)
    ref = (torch.softmax(q @ k.transpose(2, 3), -1) @ v).transpose(1, 2).reshape(B, T, d)
    _close(o.get(), ref, rtol=2e-2, atol=1e-2, what="attention")
    assert o.halo_is_zero()


def test_attention_peaked_softmax():
    """a query row that matches one late key with a huge score (forces the online-softmax rescale path); V in its own
    buffer (ldv != ldqk)."""
    B, T, d, heads = 1, 200, 64, 1
    q = _rand(B, T, d, seed=23) * 0.1
    k = _rand(B, T, d, seed=24) * 0.1
    v = _rand(B, T, d, seed=25)
    k[0, 170] = 3.0
    q[0, 5] = 3.0                       # score(5, 170) ~ 576 in log2 units; everything else ~0
    qk = G.Rows(B, T, 2 * d).set(torch.cat([q, k], -1))
    vr = G.Rows(B, T, d).set(v)
    o = G.Rows(B, T, d)
    G.attention(qk.buf, 2 * d, qk.lead, vr.buf, 0, d, o.buf, d, B, T, qk.P, heads, d)
    torch.cuda.synchronize()
    s = (_bf(q) @ _bf(k).transpose(1, 2)) * math.log(2.0)
    ref = torch.softmax(s, -1) @ _bf(v)
    _close(o.get(), ref, rtol=2e-2, atol=1e-2, what="peaked attention")
    _close(o.get()[0, 5], _bf(v)[0, 170], rtol=1e-2, atol=1e-2, what="one-hot row")


@pytest.mark.parametrize("C", [64, 512, 768, 1280])
def test_layernorm(C):
    B, T = 3, 211
    x0 = _rand(B, T, C, seed=26) * 3.0 + 0.7
    x = G.Rows(B, T, C).set(x0)
    y = G.Rows(B, T, C)
    g, b = 1.0 + 0.1 * _rand(C, seed=27), 0.1 * _rand(C, seed=28)
    G.layernorm(x.buf, y.buf, g, b, 1e-5, x.lead, B, x.P, T, C)
    torch.cuda.synchronize()
    ref = F.layer_norm(x.get(), (C,), g, b, 1e-5)
    _close(y.get(), ref, rtol=1e-2, atol=1e-2, what="layernorm")
    assert y.halo_is_zero()


def test_tag_decide_exact():
    rows, C_ = 3000, 141
    logits = _rand(rows, C_, seed=29) * 4.0
    logits[7, 3] = logits[7, 90] = 50.0            # tie -> first index
    ids, arg, mp = G.tag_decide(logits, 0.5, 77)
    torch.cuda.synchronize()
    p = torch.softmax(logits, -1)
    mref, aref = p.max(-1)
    assert torch.equal(arg.long(), aref) and int(arg[7]) == 3
    torch.testing.assert_close(mp, mref, rtol=2e-6, atol=2e-7)
    sure = (mref - 0.5).abs() > 1e-5
    want = torch.where(mref < 0.5, torch.full_like(aref, 77), aref)
    assert torch.equal(ids.long()[sure], want[sure])


# ---- the 256x256 tile kernel takes over when N % 256 == 0 and M >= 2048 (gemm256.hip)

@pytest.mark.parametrize("K,N", [(64, 256), (512, 512), (1536, 256), (2048, 512)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_gemm256_linear_residual(K, N, act):
    B, T = 3, 1500
    a = G.Rows(B, T, K).set(_rand(B, T, K, seed=41))
    x0 = _rand(B, T, N, seed=42)
    x = G.Rows(B, T, N).set(x0)
    w, bias = _rand(N, K, scale=K ** -0.5, seed=43), _rand(N, scale=0.1, seed=44)
    wp, bp = G.pad_weight(w, bias)
    assert B * a.P >= 2048
    G.gemm(a.buf, a.lead * K, K, wp, B * a.P, N, a.P, T, x.buf, N, x.lead, x.P, bias=bp, res=x.buf, ldres=N, alpha=0.5, act=act)
    torch.cuda.synchronize()
    y = a.get() @ _bf(w).T + bias
    y = [y, F.gelu(y), F.relu(y)][act]
    _close(x.get(), _bf(x0) + 0.5 * y, what="gemm256")
    assert x.halo_is_zero()


def test_gemm256_conv_k31_glu_f32():
    B, T, C = 2, 1500, 256
    x0 = _rand(B, T, C, seed=45)
    a = G.Rows(B, T, C).set(x0)
    # dense k=31 conv as one contiguous-tap GEMM (the Conformer conv)
    w, bias = _rand(C, C, 31, scale=(31 * C) ** -0.5, seed=46), _rand(C, scale=0.1, seed=47)
    wp, bp = G.pad_weight(w.permute(0, 2, 1).reshape(C, 31 * C), bias)
    out = G.Rows(B, T, C)
    G.gemm(a.buf, (a.lead - 15) * C, C, wp, B * a.P, C, a.P, T, out.buf, C, out.lead, out.P, bias=bp, act=1)
    torch.cuda.synchronize()
    ref = F.gelu(F.conv1d(_bf(x0).transpose(1, 2), _bf(w), bias, padding=15)).transpose(1, 2)
    _close(out.get(), ref, what="k31 conv 256")
    # GLU (pointwise conv d -> 2d, rows interleaved 16 a | 16 gate)
    d = C
    w2, b2 = _rand(2 * d, d, scale=d ** -0.5, seed=48), _rand(2 * d, scale=0.2, seed=49)
    rows, brow = torch.empty_like(w2), torch.empty_like(b2)
    for g in range(d // 16):
        rows[32 * g:32 * g + 16] = w2[16 * g:16 * g + 16]
        rows[32 * g + 16:32 * g + 32] = w2[d + 16 * g:d + 16 * g + 16]
        brow[32 * g:32 * g + 16] = b2[16 * g:16 * g + 16]
        brow[32 * g + 16:32 * g + 32] = b2[d + 16 * g:d + 16 * g + 16]
    wp2, bp2 = G.pad_weight(rows, brow)
    o2 = G.Rows(B, T, d)
    G.gemm(a.buf, a.lead * d, d, wp2, B * a.P, 2 * d, a.P, T, o2.buf, d, o2.lead, o2.P, bias=bp2, glu=1)
    torch.cuda.synchronize()
    _close(o2.get(), F.glu(a.get() @ _bf(w2).T + b2, dim=-1), what="glu 256")
    # fp32 frame-row output (the BiLSTM input projection's shape)
    w3, b3 = _rand(512, C, scale=C ** -0.5, seed=50), _rand(512, seed=51)
    wp3, bp3 = G.pad_weight(w3, b3)
    gx = torch.zeros(a.R, 512, device="cuda")
    G.gemm(a.buf, a.lead * C, C, wp3, B * a.P, 512, a.P, T, gx, 512, a.lead, a.P, bias=bp3, out_f32=1)
    torch.cuda.synchronize()
    got = gx[a.lead:a.lead + B * a.P].view(B, a.P, 512)[:, :T]
    _close(got, a.get() @ _bf(w3).T + b3, rtol=1e-3, atol=1e-3, what="f32 256")
    # dilated taps + stride 2 through the big kernel
    C2 = 64
    x1 = _rand(B, 2 * T, C2, seed=52)
    o3 = G.Rows(B, T, 256, halo=20, lead=16)
    a3 = G.Rows(B, 2 * T, C2, lead=8, pitch=2 * o3.P, tail=512).set(x1)
    w4, b4 = _rand(256, C2, 3, scale=(3 * C2) ** -0.5, seed=53), _rand(256, scale=0.1, seed=54)
    wp4, bp4 = G.pad_weight(w4.permute(0, 2, 1).reshape(256, 3 * C2), b4)
    G.gemm(a3.buf, (a3.lead - 1) * C2, 2 * C2, wp4, B * o3.P, 256, o3.P, T, o3.buf, 256, o3.lead, o3.P, bias=bp4, act=1)
    torch.cuda.synchronize()
    ref = F.gelu(F.conv1d(_bf(x1).transpose(1, 2), _bf(w4), b4, stride=2, padding=1)).transpose(1, 2)
    _close(o3.get(), ref, what="stride-2 conv 256")
    x2 = _rand(B, T, 128, seed=55)
    a4 = G.Rows(B, T, 128).set(x2)
    w5, b5 = _rand(256, 128, 3, scale=(3 * 128) ** -0.5, seed=56), _rand(256, scale=0.1, seed=57)
    wp5, bp5 = G.pad_weight(w5.permute(0, 2, 1).reshape(256, 3 * 128), b5)
    o5 = G.Rows(B, T, 256)
    G.gemm(a4.buf, (a4.lead - 4) * 128, 128, wp5, B * a4.P, 256, a4.P, T, o5.buf, 256, o5.lead, o5.P, bias=bp5, act=2, cin=128, tap_stride=4 * 128)
    torch.cuda.synchronize()
    ref = F.relu(F.conv1d(_bf(x2).transpose(1, 2), _bf(w5), b5, padding=4, dilation=4)).transpose(1, 2)
    _close(o5.get(), ref, what="dilated conv 256")


def test_gemm256_both_block_heights():
    """The launcher picks a 192- or 256-row block by a cost model; run the big-tile tests with each forced."""
    import os
    import subprocess
    import sys
    if os.environ.get("WFL_GEMM_BM"):
        pytest.skip("inner run")
    for bm in ("192", "256"):
        env = dict(os.environ, WFL_GEMM_BM=bm)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-k", "gemm256_linear or gemm256_conv",
                            "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=600,
                           cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        assert r.returncode == 0, (bm, r.stdout[-3000:])


# ---- the persistent streaming kernel (gemm_stream.hip): several tiles per workgroup, register epilogue, folded LayerNorm

@pytest.mark.parametrize("B,T,K,N,act,res", [(16, 1500, 512, 1536, 0, False), (16, 1500, 512, 2048, 1, False),
                                             (16, 1500, 1024, 1024, 0, True), (6, 1500, 2048, 512, 0, True),
                                             (64, 49, 256, 512, 2, False), (40, 499, 512, 768, 1, False)])
def test_gemm_stream_shapes(B, T, K, N, act, res):
    """more tiles than CUs (each workgroup walks several tiles on one operand stream), both block heights, clips shorter
    than a tile (T = 49) and a residual epilogue; every frame and the halos are checked."""
    a = G.Rows(B, T, K).set(_rand(B, T, K, seed=61))
    x0 = _rand(B, T, N, seed=62)
    x = G.Rows(B, T, N).set(x0)
    w, bias = _rand(N, K, scale=K ** -0.5, seed=63), _rand(N, scale=0.1, seed=64)
    wp, bp = G.pad_weight(w, bias)
    assert B * a.P >= 2048 and wp.shape[0] == N
    G.gemm(a.buf, a.lead * K, K, wp, B * a.P, N, a.P, T, x.buf, N, x.lead, x.P, bias=bp, res=x.buf if res else None,
           ldres=N, alpha=0.5, act=act)
    torch.cuda.synchronize()
    y = a.get() @ _bf(w).T + bias
    y = [y, F.gelu(y), F.relu(y)][act]
    _close(x.get(), _bf(x0) + 0.5 * y if res else y, what="gemm_stream")
    assert x.halo_is_zero()


def test_gemm_stream_ragged_columns_and_conv_taps():
    """n_valid < N (columns beyond it must stay untouched) and a 3-tap dilated conv through the streaming kernel."""
    B, T, C, N, nv = 4, 1500, 256, 512, 328
    x0 = _rand(B, T, C, seed=65)
    a = G.Rows(B, T, C).set(x0)
    w, bias = _rand(nv, C, 3, scale=(3 * C) ** -0.5, seed=66), _rand(nv, scale=0.1, seed=67)
    wp, bp = G.pad_weight(w.permute(0, 2, 1).reshape(nv, 3 * C), bias)
    wp = torch.cat([wp, torch.zeros(N - wp.shape[0], wp.shape[1], dtype=wp.dtype, device="cuda")])
    bp = torch.cat([bp, torch.zeros(N - bp.shape[0], device="cuda")])
    out = G.Rows(B, T, N)
    out.buf.fill_(7.0)
    dil = 2
    G.gemm(a.buf, (a.lead - dil) * C, C, wp, B * a.P, nv, a.P, T, out.buf, N, out.lead, out.P, bias=bp, act=2, cin=C, tap_stride=dil * C)
    torch.cuda.synchronize()
    ref = F.relu(F.conv1d(_bf(x0).transpose(1, 2), _bf(w), bias, padding=dil, dilation=dil)).transpose(1, 2)
    got = out.buf[out.lead:out.lead + B * out.P].view(B, out.P, N)
    _close(got[:, :T, :nv].float(), ref, what="stream dilated conv")
    assert bool((got[:, :T, nv:] == 7.0).all()) and bool((got[:, T:] == 7.0).all())


@pytest.mark.parametrize("B,T,K,N,act", [(16, 1500, 512, 1536, 0), (16, 1500, 512, 2048, 1), (3, 1500, 768, 768, 0)])
def test_gemm_stream_layernorm_fold(B, T, K, N, act):
    """LN(x) W^T + b computed as rstd (x W'^T - mean s) + b' with the statistics taken inside the GEMM."""
    x0 = _rand(B, T, K, seed=71) * 2.0 + 0.5
    x0[..., 3] += 9.0                                  # an outlier channel, as real encoder states have
    a = G.Rows(B, T, K).set(x0)
    gamma, beta = 1.0 + 0.2 * _rand(K, seed=72), 0.1 * _rand(K, seed=73)
    w, bias = _rand(N, K, scale=K ** -0.5, seed=74), _rand(N, scale=0.1, seed=75)
    wf = (w * gamma).to(torch.bfloat16)
    ln_s = wf.float().sum(1)
    bf = bias + w @ beta
    wp, bp = G.pad_weight(wf.float(), bf)
    out = G.Rows(B, T, N)
    G.gemm_ln(a.buf, a.lead * K, K, wp, B * a.P, N, a.P, T, out.buf, N, out.lead, out.P, bp, ln_s.contiguous(), 1e-5, act)
    torch.cuda.synchronize()
    y = F.layer_norm(a.get(), (K,), gamma, beta, 1e-5) @ w.T + bias
    y = [y, F.gelu(y)][act]
    _close(out.get(), y, rtol=2e-2, atol=2e-2, what="LN-folded gemm")
    assert out.halo_is_zero()


@pytest.mark.parametrize("C,k,N,act", [(256, 31, 256, 1), (512, 31, 512, 1), (128, 3, 256, 0), (64, 5, 256, 2), (192, 4, 256, 1)])
def test_gemm_stream_dense_conv_tap_stationary(C, k, N, act):
    """dense k-tap Conv1d given as (cin = C, tap stride = one row): the streaming kernel's tap-stationary mode (the frame tile of
    a channel chunk is staged once and re-read at a row offset per tap); odd chunk counts, both few and many taps."""
    B, T = 3, 700
    x0 = _rand(B, T, C, seed=81)
    a = G.Rows(B, T, C, halo=32, lead=32).set(x0)
    w, bias = _rand(N, C, k, scale=(k * C) ** -0.5, seed=82), _rand(N, scale=0.1, seed=83)
    wp, bp = G.pad_weight(w.permute(0, 2, 1).reshape(N, k * C), bias)
    assert wp.shape[1] == k * C
    out = G.Rows(B, T, N, halo=32, lead=32)
    left = (k - 1) // 2                                           # (even k: one more tap to the right)
    G.gemm(a.buf, (a.lead - left) * C, C, wp, B * a.P, N, a.P, T, out.buf, N, out.lead, out.P, bias=bp, act=act, cin=C, tap_stride=C)
    torch.cuda.synchronize()
    ref = F.conv1d(F.pad(_bf(x0).transpose(1, 2), (left, k - 1 - left)), _bf(w), bias).transpose(1, 2)
    ref = [ref, F.gelu(ref), F.relu(ref)][act]
    _close(out.get(), ref, what="tap-stationary conv")
    assert out.halo_is_zero()


@pytest.mark.parametrize("B,T,C,k,N", [(16, 1500, 128, 3, 2048), (32, 1500, 64, 31, 512)])
def test_gemm_stream_dense_conv_several_tiles_per_workgroup(B, T, C, k, N):
    """the tap-stationary mode with more tiles than CUs: the channel-chunk buffers, tap counters and the operand stream carry
    over from one tile to the next inside a persistent workgroup (a batch of 32 clips puts the k = 31 Conformer conv here)."""
    x0 = _rand(B, T, C, seed=91)
    a = G.Rows(B, T, C, halo=32, lead=32).set(x0)
    w, bias = _rand(N, C, k, scale=(k * C) ** -0.5, seed=92), _rand(N, scale=0.1, seed=93)
    wp, bp = G.pad_weight(w.permute(0, 2, 1).reshape(N, k * C), bias)
    out = G.Rows(B, T, N, halo=32, lead=32)
    assert ((B * a.P + 191) // 192) * (N // 256) > 256
    left = (k - 1) // 2
    G.gemm(a.buf, (a.lead - left) * C, C, wp, B * a.P, N, a.P, T, out.buf, N, out.lead, out.P, bias=bp, act=1, cin=C, tap_stride=C)
    torch.cuda.synchronize()
    ref = F.gelu(F.conv1d(F.pad(_bf(x0).transpose(1, 2), (left, k - 1 - left)), _bf(w), bias)).transpose(1, 2)
    _close(out.get(), ref, what="tap-stationary conv, several tiles per workgroup")
    assert out.halo_is_zero()


@pytest.mark.parametrize("kind", ["outlier_channels", "common_offset"])
def test_gemm_stream_layernorm_fold_outliers(kind):
    """The folded LayerNorm takes var = E[x^2] - mean^2 in fp32 (one pass).  Real encoder states carry a few channels in the
    hundreds ("massive activations") or a common offset; both stress that formula.  outlier_channels: two channels x 100 (the
    row's variance is then dominated by them: mean^2 << E[x^2], the benign direction); common_offset: every channel + 30 at unit
    spread (mean^2 / var = 900: ten of the 24 mantissa bits go to the cancellation, still 2^-14 relative on the variance)."""
    B, T, K, N = 4, 1500, 512, 1536
    x0 = _rand(B, T, K, seed=171)
    if kind == "outlier_channels":
        x0[..., 7] *= 100.0
        x0[..., 300] = x0[..., 300] * 100.0 + 150.0
    else:
        x0 += 30.0
    a = G.Rows(B, T, K).set(x0)
    gamma, beta = 1.0 + 0.2 * _rand(K, seed=172), 0.1 * _rand(K, seed=173)
    w, bias = _rand(N, K, scale=K ** -0.5, seed=174), _rand(N, scale=0.1, seed=175)
    wf = (w * gamma).to(torch.bfloat16)
    ln_s = wf.float().sum(1)
    bf = bias + w @ beta
    wp, bp = G.pad_weight(wf.float(), bf)
    out = G.Rows(B, T, N)
    G.gemm_ln(a.buf, a.lead * K, K, wp, B * a.P, N, a.P, T, out.buf, N, out.lead, out.P, bp, ln_s.contiguous(), 1e-5, 0)
    torch.cuda.synchronize()
    y = F.layer_norm(a.get(), (K,), gamma, beta, 1e-5) @ w.T + bias          # on the same bf16-rounded rows
    err = (out.get() - y).abs()
    # LayerNorm output is O(1) per channel whatever the input scale; the bf16-rounded weights W' = gamma o W leave ~2^-9 relative
    assert float(err.max()) <= 6e-2 and float(err.mean()) <= 8e-3, (kind, float(err.max()), float(err.mean()))
    assert out.halo_is_zero()
