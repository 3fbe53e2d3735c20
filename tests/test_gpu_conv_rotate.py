"""-m gpu: the tap-stationary conv mode of csrc/gemm_stream.hip with its frame fragments rotated across taps (the default) against
F.conv1d, and bit for bit against the blocked-fragment form it replaced, which WFL_CONV_ROTATE=0 still selects at every launch.
The two forms issue the same MFMAs on the same operands in the same K order; only the frame a lane column owns differs (and with it
the LDS image of the extended frame tile and the epilogue's row index), so every stored element -- halos, row and column tails
included -- must be equal, not merely close.  Tolerances against the reference are those of test_gpu_ops.py's conv test (its _close
defaults) and, for the three-segment form, test_gpu_round4.py's float64 bound."""
import os

import pytest
import torch
import torch.nn.functional as F

import gpu_util as G
from wfl_asr_amd import _lib
from test_gpu_round4 import _PairRows, _split

pytestmark = pytest.mark.gpu


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _bf(x):
    return x.to(torch.bfloat16).float()


def _close(got, want, rtol=2e-2, atol=2e-2, what=""):      # test_gpu_ops.py's, defaults and all
    err = (got - want).abs()
    lim = atol + rtol * want.abs()
    assert bool((err <= lim).all()), f"{what}: max err {err.max().item():.4g}, worst excess {(err - lim).max().item():.4g}"


def _cmin(k):
    """fewest channels at which k taps reach the conv mode: wfl_launch_gemm takes cin in whole 64s only (two 32-channel chunks), and the
    streaming kernel K = k C of at least 8 steps of 32 (wfl_gemm_stream_takes).  64 from k = 4 on, 128 for k = 3."""
    return 64 if k >= 4 else 128


def _both_forms(monkeypatch, launch):
    """launch() -> the output buffers of one launch; run once per form."""
    assert "WFL_GEMM_NO_CONV" not in os.environ
    monkeypatch.delenv("WFL_CONV_ROTATE", raising=False)
    new = launch()
    monkeypatch.setenv("WFL_CONV_ROTATE", "0")
    old = launch()
    monkeypatch.delenv("WFL_CONV_ROTATE")
    torch.cuda.synchronize()
    return new, old


def _conv(monkeypatch, B, T, C, k, N, act, pitch=None):
    """N: output channels (n_valid); the weight is padded to whole 256-column tiles as the model's are."""
    x0 = _rand(B, T, C, seed=81)
    a = G.Rows(B, T, C, halo=32, lead=32, pitch=pitch).set(x0)
    w, bias = _rand(N, C, k, scale=(k * C) ** -0.5, seed=82), _rand(N, scale=0.1, seed=83)
    Np = (N + 255) // 256 * 256
    wp = torch.zeros(Np, k * C, dtype=torch.bfloat16, device="cuda")
    wp[:N] = w.permute(0, 2, 1).reshape(N, k * C).to(torch.bfloat16)
    bp = torch.zeros(Np, dtype=torch.float32, device="cuda")
    bp[:N] = bias
    assert N % 8 == 0
    left = (k - 1) // 2                                            # (even k: one more tap to the right)

    def launch():
        out = G.Rows(B, T, N, halo=32, lead=32, pitch=pitch)
        G.gemm(a.buf, (a.lead - left) * C, C, wp, B * a.P, N, a.P, T, out.buf, N, out.lead, out.P, bias=bp, act=act, cin=C, tap_stride=C)
        return out

    new, old = _both_forms(monkeypatch, launch)
    ref = F.conv1d(F.pad(_bf(x0).transpose(1, 2), (left, k - 1 - left)), _bf(w), bias).transpose(1, 2)
    ref = [ref, F.gelu(ref), F.relu(ref)][act]
    _close(new.get(), ref, what=f"rotated conv C={C} k={k} N={N}")
    assert new.halo_is_zero() and old.halo_is_zero()
    assert torch.equal(new.buf, old.buf)
    return a


@pytest.mark.parametrize("k", [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 31, 32])
def test_every_tap_count_residue(monkeypatch, k):
    """k = 3 is the fewest taps the mode takes (the steady loop's carried fragments meet a chunk boundary at once), 32 the most; every
    k mod 6; even k has one more tap on the right.  The fewest channels the launch takes (_cmin)."""
    _conv(monkeypatch, 3, 700, _cmin(k), k, 256, 0)


@pytest.mark.parametrize("C", [64, 128, 192, 320])           # 2, 4, 6, 10 chunks (cin comes in whole 64s)
@pytest.mark.parametrize("k", [7, 31])
def test_chunk_boundaries_and_buffer_parity(monkeypatch, C, k):
    _conv(monkeypatch, 3, 700, C, k, 256, 1)


@pytest.mark.parametrize("T", [50, 7, 1])
@pytest.mark.parametrize("k", [5, 31])
def test_clips_and_halos_inside_one_fragment(monkeypatch, T, k):
    """short clips: the 16 lane columns of one fragment, six rows apart, fall in different clips and in halo rows."""
    _conv(monkeypatch, 40, T, _cmin(k), k, 256, 0)


@pytest.mark.parametrize("T,pitch,rows", [(700, 744, "no multiple of 96"), (700, 736, "a multiple of 96, not of 192"), (600, 640, "a multiple of 192")])
def test_row_tail(monkeypatch, T, pitch, rows):
    a = _conv(monkeypatch, 3, T, 64, 9, 256, 2, pitch=pitch)
    m = 3 * a.P
    assert {"no multiple of 96": m % 96 != 0, "a multiple of 96, not of 192": m % 96 == 0 and m % 192 != 0, "a multiple of 192": m % 192 == 0}[rows]


@pytest.mark.parametrize("k", [9, 31])
def test_column_tail(monkeypatch, k):
    """144 valid columns of a 256-column tile (the kernel takes n_valid in whole runs of 8: the classifier's 141 go to another kernel)."""
    _conv(monkeypatch, 3, 700, 64, k, 144, 1)


def test_several_tiles_per_workgroup(monkeypatch):
    B, T, C, k, N = 32, 750, _cmin(7), 7, 512
    a = _conv(monkeypatch, B, T, C, k, N, 1)
    assert ((B * a.P + 191) // 192) * (N // 256) > 256


def test_the_models_own_instantiation(monkeypatch):
    _conv(monkeypatch, 3, 700, 512, 31, 512, 1)


@pytest.mark.parametrize("C,k,N,act", [(64, 31, 256, 1), (64, 3, 256, 0)])
def test_three_segment_form(monkeypatch, C, k, N, act):
    """model.precision: high: operands and result as bf16 pairs, K = [A_hi W_hi | A_lo W_hi | A_hi W_lo] (wfl_op_gemm_split), the conv
    mode's instantiation that writes a low half.  Inputs and the float64 bound as test_gpu_round4.py's gemm_split test."""
    B, T, K = 3, 700, k * C
    g = torch.Generator().manual_seed(3 + K + N)
    x = _PairRows(B, T, C).set((torch.randn(B, T, C, generator=g) * torch.logspace(-1, 1, C)).cuda())
    w = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
    w_hi, w_lo = _split(w)
    w3 = torch.cat([w_hi, w_hi, w_lo], 1).contiguous()
    bias = torch.randn(N, generator=g).cuda()
    P = x.hi.P
    left = (k - 1) // 2
    lead = x.hi.lead - left
    assert lead >= 0 and P - T >= k - 1 - left

    def launch():
        out = _PairRows(B, T, N)
        rc = G.lib().wfl_op_gemm_split(G.ptr(x.hi.buf, lead * C), G.ptr(x.lo.buf, lead * C), C, C, C, G.ptr(w3), B * P, N, K, N, P, T,
                                       G.ptr(out.hi.buf), G.ptr(out.lo.buf), N, out.hi.lead, out.hi.P, G.ptr(bias), None, None, N, 1.0, act, 0,
                                       G.stream())
        _lib.check(rc, "wfl_op_gemm_split")
        return out

    new, old = _both_forms(monkeypatch, launch)

    def unfold(v):
        v = F.pad(v, (0, 0, left, k - 1 - left))
        return torch.cat([v[:, j:j + T] for j in range(k)], 2)

    xh, xl = unfold(x.hi.get().double()), unfold(x.lo.get().double())
    wh, wl = w_hi.double(), w_lo.double()
    ref = xh @ wh.T + xl @ wh.T + xh @ wl.T + bias.double()
    mag = (xh.abs() + xl.abs()) @ (wh.abs() + wl.abs()).T + bias.abs().double()
    if act == 1:
        ref = F.gelu(ref)
    err = (new.value() - ref).abs()
    assert bool((err <= 2 ** -15 * ref.abs() + 4e-6 * mag + 1e-30).all()), float((err / mag).max())
    assert new.hi.halo_is_zero() and new.lo.halo_is_zero() and old.hi.halo_is_zero() and old.lo.halo_is_zero()
    assert torch.equal(new.both, old.both)
