"""Plain float64 references of the WavLM-path kernels and of attention's bias / ragged / split modes, and the seeded inputs of the
operator tests (tests/test_gpu_ops_wavlm.py runs the kernels on them, tests/test_ops_ref_cpu.py checks the references themselves and
that each test's bound separates a right reference from a wrong one), and -- in the second half -- the same for the front-end kernels
(Whisper log-mel, WavLM waveform statistics, conv level 0 and frame counts: tests/test_gpu_ops_frontend.py).  Everything here runs on
the CPU.

The references take the operand VALUES as the kernels read them -- bf16 values, or hi + lo sums of bf16 pairs -- so operand rounding
is no part of any error; what is left is the kernel's own arithmetic and the rounding of what it stores."""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64


def split(x):
    """float -> bf16 pair (hi, lo): hi = bf16(x), lo = bf16(x - hi)."""
    hi = x.to(torch.bfloat16)
    lo = (x.double() - hi.double()).to(torch.bfloat16)
    return hi, lo


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------ attention
def attention_ref(q, k, v, heads, table=None, gate=None, clip_T=None):
    """q, k, v [B, T, d] float64 (q already scaled by hd^-1/2 log2 e).  table [heads, 2T-1] and gate [B, heads, T] (both laid out for
    the batch-wide T) or None.  clip_T: list of B frame counts or None.
    s[b,h,q,k] = q.k + gate[b,h,q] * table[h][k - q + T - 1] in log2 units; p = 2^(s - max); out = p @ v / sum p over keys < clip_T[b].
    -> (out [B, T, d], A [B, T, d] = softmax-weighted mean of |v|); rows >= clip_T[b] are zero in both."""
    B, T, d = q.shape
    hd = d // heads
    qh = q.double().view(B, T, heads, hd).transpose(1, 2)
    kh = k.double().view(B, T, heads, hd).transpose(1, 2)
    vh = v.double().view(B, T, heads, hd).transpose(1, 2)
    s = qh @ kh.transpose(2, 3)                                             # [B, heads, T(q), T(k)]
    if table is not None:
        idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + T - 1   # [q, k]
        s = s + gate.double()[..., None] * table.double()[:, idx][None]
    n = torch.tensor([T] * B if clip_T is None else list(clip_T))
    alive = torch.arange(T)[None, :] < n[:, None]                           # [B, T]
    s = s.masked_fill(~alive[:, None, None, :], -math.inf)
    s = s.masked_fill(~alive[:, None, :, None], 0.0)                        # (dead queries: any finite row; zeroed below)
    empty = n == 0
    s[empty] = 0.0
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    p = p / p.sum(-1, keepdim=True)
    out = (p @ vh).transpose(1, 2).reshape(B, T, d)
    A = (p @ vh.abs()).transpose(1, 2).reshape(B, T, d)
    out = out * alive[..., None]
    A = A * alive[..., None]
    return out, A


def attn_inputs(hd, heads, B, T, bias=False, pair=False, clip_T=None, seed=0, v_range=None):
    """Seeded inputs of one attention case.  q, k ~ N(0,1) hd^-1/4 (scores ~ N(0,1) in log2 units); v ~ N(0,1), or uniform in v_range.
    Table: independent N(0, 2^2) per (head, delta) -- no two deltas equal; gate uniform in [0.5, 2.5].  K and V rows at t >= clip_T[b]
    hold 50.0: finite junk that would dominate the softmax if a key there were not masked.
    -> dict of bf16 tensors q_hi, q_lo, k_hi, ... [B, T, d] (lo all zero unless pair), fp32 table / gate or None, clip_T."""
    g = _gen(1000 + seed)
    d = hd * heads
    c = {"hd": hd, "heads": heads, "B": B, "T": T, "d": d, "clip_T": clip_T, "pair": pair}
    for name in ("q", "k", "v"):
        x = torch.randn(B, T, d, generator=g)
        if name != "v":
            x = x * hd ** -0.25
        elif v_range is not None:
            x = torch.rand(B, T, d, generator=g) * (v_range[1] - v_range[0]) + v_range[0]
        if clip_T is not None and name != "q":
            for b in range(B):
                x[b, clip_T[b]:] = 50.0
        hi, lo = split(x)
        c[name + "_hi"], c[name + "_lo"] = hi, (lo if pair else torch.zeros_like(lo))
    c["table"] = (torch.randn(heads, 2 * T - 1, generator=g) * 2.0) if bias else None
    c["gate"] = (torch.rand(B, heads, T, generator=g) * 2.0 + 0.5) if bias else None
    return c


def attn_values(c, drop_lo=False):
    """The float64 operand values of a case: hi + lo (drop_lo: the wrong reading that forgets the low halves)."""
    return tuple(c[n + "_hi"].double() + (0.0 if drop_lo else c[n + "_lo"].double()) for n in ("q", "k", "v"))


def attn_case_ref(c):
    q, k, v = attn_values(c)
    return attention_ref(q, k, v, c["heads"], c["table"], c["gate"], c["clip_T"])


def gate_own_length(gate, clip_T):
    """The wrong gate a kernel reads when it indexes the [B][heads][T] buffer with each clip's own length instead of T."""
    B, H, T = gate.shape
    flat = gate.reshape(-1)
    out = gate.clone()
    for b in range(B):
        n = clip_T[b]
        for h in range(H):
            out[b, h, :n] = flat[(b * H + h) * n:(b * H + h) * n + n]
    return out


# bounds.  bf16 attention: the tolerance of test_qkv_projection_and_attention (same kernel family, same bf16 P and output rounding)
ATTN_RTOL, ATTN_ATOL = 2e-2, 1e-2
# split precision: 2^-15 |ref| (sixteen significant bits of the stored pair) + ATTN_KAPPA * A, A the softmax-weighted mean of |v|.
# Measured max(err / A) over the split cases of tests/test_gpu_ops_wavlm.py (table at test_attention_split_precision there): 2.6e-6 ..
# 3.9e-6 without a bias, 9.9e-6 and 1.21e-5 with one; ATTN_KAPPA = 4 x the largest.  Dropping the low halves costs ~1e-3 A: the CPU
# control still trips at this kappa.
ATTN_KAPPA = 4 * 1.2106e-5


def attn_bound_bf16(ref):
    return ATTN_ATOL + ATTN_RTOL * ref.abs()


def attn_bound_split(ref, A):
    return 2.0 ** -15 * ref.abs() + ATTN_KAPPA * A


# ---------------------------------------------------------------------------------------------------------- gate, table, regroup
def relpos_table_ref(rel_emb, bucket_of_delta, max_t, T):
    """table[h][delta + T - 1] = rel_emb[bucket_of_delta[delta + max_t - 1]][h], delta in [-(T-1), T-1]."""
    delta = torch.arange(-(T - 1), T)
    return rel_emb[bucket_of_delta[delta + max_t - 1].long()].T.contiguous()


def relpos_gate_ref(x, heads, w8, b8, cst):
    """x [B, T, heads * hd] float64 values.  (ga, gb) = sigmoid((w8 x_head + b8).view(2, 4).sum(-1)); gate = ga (gb cst_h - 1) + 2.
    -> [B, heads, T] float64."""
    B, T, d = x.shape
    hd = d // heads
    xh = x.double().view(B, T, heads, hd).transpose(1, 2)                    # [B, heads, T, hd]
    proj = (xh @ w8.double().T + b8.double()).view(B, heads, T, 2, 4).sum(-1)
    ga, gb = torch.sigmoid(proj).unbind(-1)
    return ga * (gb * cst.double()[None, :, None] - 1.0) + 2.0


def regroup_ref(buf, groups, cpg, lead, B, P, T, clip_T=None):
    """buf [R, d] frame rows as they lie in memory (junk in the halos included) -> xg [groups, R, 64]: channels g*cpg .. +cpg of every
    valid frame, zero elsewhere."""
    R, d = buf.shape
    xg = torch.zeros(groups, R, 64, dtype=buf.dtype)
    for b in range(B):
        n = T if clip_T is None else clip_T[b]
        r0 = lead + b * P
        xg[:, r0:r0 + n, :cpg] = buf[r0:r0 + n].view(n, groups, cpg).transpose(0, 1)
    return xg


# ------------------------------------------------------------------------------------------------------------- positional conv
def pack_posconv(w, b, groups):
    """Conv1d weight [d, cpg, taps] + bias [d] -> the kernel's operands, as model.hip packs them: W [groups][64][taps * 64] with
    W[g][o][tap * 64 + c] = w[g cpg + o][c][tap] and zero rows / columns beyond cpg, bias [groups][64]."""
    d, cpg, taps = w.shape
    W = torch.zeros(groups, 64, taps, 64, dtype=w.dtype)
    W[:, :cpg, :, :cpg] = w.view(groups, cpg, cpg, taps).permute(0, 1, 3, 2)
    bb = torch.zeros(groups, 64, dtype=b.dtype)
    bb[:, :cpg] = b.view(groups, cpg)
    return W.reshape(groups, 64, taps * 64).contiguous(), bb


def posconv_ref(x_conv, res, W, bias, cpg, taps, clip_T=None, with_mag=False):
    """x_conv, res [B, T, d] float64: the conv's operand (the hi halves) and the residual (hi + lo).  W, bias as pack_posconv lays them out.
    out = res + gelu_erf(conv1d(x, w, b, padding = taps/2, groups)[..., :-1]) per clip over its own clip_T frames, zeros beyond them;
    computed from the PACKED weights as a product over unfolded windows (frame t reads frames t - taps/2 .. t + taps/2 - 1).
    -> out (rows >= clip_T[b] zero), and with_mag: sum |x||w| + |bias| + |res|."""
    B, T, d = x_conv.shape
    groups = W.shape[0]
    n = torch.tensor([T] * B if clip_T is None else list(clip_T))
    alive = (torch.arange(T)[None, :] < n[:, None])[..., None]
    x = x_conv.double() * alive
    xp = F.pad(x, (0, 0, taps // 2, taps // 2))                              # [B, T + taps, d]
    Wg = W.double().view(groups, 64, taps, 64)[:, :cpg, :, :cpg]             # [g, o, j, c]
    bg = bias.double()[:, :cpg]
    y = torch.empty(B, T, groups, cpg, dtype=F64)
    mag = torch.empty(B, T, groups, cpg, dtype=F64) if with_mag else None
    for gi in range(groups):                                                 # (one group at a time: the unfolded windows are large)
        win = xp[:, :, gi * cpg:(gi + 1) * cpg].unfold(1, taps, 1)[:, :T]    # [B, T, cpg, taps]: win[b, t, c, j] = x[b, t - taps/2 + j, c]
        y[:, :, gi] = torch.einsum("btcj,ojc->bto", win, Wg[gi]) + bg[gi]
        if with_mag:
            mag[:, :, gi] = torch.einsum("btcj,ojc->bto", win.abs(), Wg[gi].abs()) + bg[gi].abs()
    out = (res.double() + F.gelu(y).reshape(B, T, d)) * alive
    if not with_mag:
        return out
    return out, (mag.reshape(B, T, d) + res.double().abs()) * alive


def posconv_inputs(groups, cpg, taps, B, T, pair, seed=0):
    g = _gen(2000 + seed)
    d = groups * cpg
    x = torch.randn(B, T, d, generator=g)
    w = torch.randn(d, cpg, taps, generator=g) * (2.0 / math.sqrt(cpg * taps))      # conv outputs ~ N(0, 2^2): both GELU branches
    b = torch.randn(d, generator=g) * 0.5
    x_hi, x_lo = split(x)
    W, bias = pack_posconv(w.to(torch.bfloat16), b, groups)
    return {"groups": groups, "cpg": cpg, "taps": taps, "B": B, "T": T, "d": d, "x_hi": x_hi, "x_lo": x_lo if pair else torch.zeros_like(x_lo),
            "W": W, "bias": bias, "w": w.to(torch.bfloat16), "b": b}


# pair output: sixteen significant bits + the fp32 accumulation, c * mag with c = 4e-6 as in
# test_gemm_split_against_a_float64_product_of_its_own_pairs (same MFMA, fp32 accumulation).  hi alone: 2^-8 |ref| instead of 2^-15.
POSCONV_C = 4e-6


def posconv_bound(ref, mag, pair):
    return (2.0 ** -15 if pair else 2.0 ** -8) * ref.abs() + POSCONV_C * mag


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_ref(x, gamma, beta, eps, n_div=0, gelu=False, with_scale=False):
    """x [..., C] float64 values.  Statistics over the first n_div channels (0: all): biased variance, eps inside the root; optional
    exact-erf GELU.  with_scale: also what an error of the fp32 arithmetic scales with (see layernorm_bound)."""
    C = x.shape[-1]
    n = n_div or C
    x = x.double()
    mean = x[..., :n].sum(-1, keepdim=True) / n
    var = ((x[..., :n] - mean) ** 2).sum(-1, keepdim=True) / n
    rstd = (var + eps) ** -0.5
    y = (x - mean) * rstd * gamma.double() + beta.double()
    out = F.gelu(y) if gelu else y
    if with_scale:
        g = gamma.double().abs()
        return out, g * rstd * ((x - mean).abs() + mean.abs() + 1.0 / rstd) + beta.double().abs()
    return out


def layernorm_inputs(C, n_div, B, T, pair, offset=False, seed=0):
    """x ~ N(0.7, 3^2), or N(30, 1) (offset: the common offset a one-pass variance would lose); gamma = beta = 0 and x = 0 beyond n_div."""
    g = _gen(3000 + seed + C)
    x = torch.randn(B, T, C, generator=g) * (1.0 if offset else 3.0) + (30.0 if offset else 0.7)
    gamma = 1.0 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    n = n_div or C
    x[..., n:] = 0
    gamma[n:] = 0
    beta[n:] = 0
    x_hi, x_lo = split(x)
    return {"C": C, "n_div": n_div, "B": B, "T": T, "x_hi": x_hi, "x_lo": x_lo if pair else torch.zeros_like(x_lo), "gamma": gamma,
            "beta": beta, "gamma2": (1.0 + 0.1 * torch.randn(C, generator=g)) * (torch.arange(C) < n),
            "beta2": 0.1 * torch.randn(C, generator=g) * (torch.arange(C) < n)}


LN_RTOL, LN_ATOL = 1e-2, 1e-2          # bf16 output: test_layernorm's tolerance
# pair output: 2^-15 |ref| (sixteen significant bits of the stored pair) + LN_LAMBDA * scale for the fp32 statistics and affine, with
#   scale = |gamma| rstd (|x - mean| + |mean| + 1 / rstd) + |beta|.
# Derivation: y = gamma (x - mean) rstd + beta.  An error d_mean of the fp32 mean -- a few fp32 roundings of |mean| + the row's spread
# 1 / rstd -- moves EVERY element of the row by |gamma| rstd d_mean, whatever its own |x - mean|; a relative error of rstd and the
# roundings of the affine move it by a few 2^-24 of |gamma| |x - mean| rstd + |beta|.  (Relative to |gamma| |x - mean| rstd + |beta| alone
# the first part is unbounded at elements near the row mean with a small beta: measured max 4.9e-5 on N(0.7, 3^2) rows, 1.9e-3 on
# N(30, 1) rows, against 2e-6 .. 1e-5 typical -- a bound fitted to that would pass a kernel that lost the low halves, 2^-9.)
# LN_LAMBDA = 4 x the largest measured err / scale over the pair cases of test_layernorm_act and test_layernorm_act_common_offset
# (table there).
LN_LAMBDA = 4 * 5.7155e-6


def layernorm_bound(ref, scale, pair):
    if pair:
        return 2.0 ** -15 * ref.abs() + LN_LAMBDA * scale
    return LN_ATOL + LN_RTOL * ref.abs()


def frac_outside(wrong, right, bound, factor=2.0):
    """Share of the compared elements at which a wrong reference is further than factor x bound from the right one: no output within
    `bound` of the right reference can then be within `bound` of the wrong one there."""
    return float(((wrong - right).abs() > factor * bound).double().mean())


# ---------------------------------------------------------------------------------------------- the operator tests' cases
# (one place, so that the CPU controls see exactly the inputs the GPU tests run on)
CLIP_T = [257, 70, 1, 0]
ATTN_BIAS_CASES = [(hd, heads, T) for hd, heads in ((32, 2), (64, 3)) for T in (64, 129, 257)]
ATTN_CLIP_CASES = [("plain", 64), ("plain", 256), ("bias", 32), ("bias", 64), ("split", 64)]
ATTN_SPLIT_CASES = [(32, False), (64, False), (128, False), (256, False), (32, True), (64, True)]
POSCONV_CASES = [(4, 16, 16), (16, 48, 128), (2, 64, 128)]
POSCONV_B, POSCONV_T, POSCONV_CLIP_T = 2, 300, [300, 70]
LN_T, LN_CLIP_T = 211, [211, 70, 0]


def bias_case(hd, heads, T):
    return attn_inputs(hd, heads, 2, T, bias=True, seed=hd + T)


def clip_case(variant, hd):
    return attn_inputs(hd, 2, 4, 257, bias=variant == "bias", pair=variant == "split", clip_T=CLIP_T, seed=7 + hd)


def split_case(hd, bias):
    return attn_inputs(hd, 2, 2, 257, bias=bias, pair=True, seed=11 + hd + int(bias))


def posconv_case(groups, cpg, taps, pair):
    return posconv_inputs(groups, cpg, taps, POSCONV_B, POSCONV_T, pair, seed=groups + taps)


# =================================================================================================== the front-end kernels
# (tests/test_gpu_ops_frontend.py; the references take the fp32 input VALUES in float64, so operand rounding is no part of any error)
U24 = 2.0 ** -24                         # fp32 unit roundoff


# ------------------------------------------------------------------------------------------------------------ Whisper log-mel
def mel_bank(n_mels, htk=False):
    """[201, n_mels] float64 VALUES of the fp32 bank the model uploads (the oracle's float64 Slaney bank rounded to fp32)."""
    from oracle import wfl_oracle as O
    fb = O.mel_filter_bank_htk(n_mels) if htk else O.mel_filter_bank(n_mels)
    return torch.from_numpy(fb).to(torch.float32).double()


def mel_maxw(fb):
    """The widest triangle of the bank in bins: the longest fp32 sum of the sparse mel projection."""
    nz = fb != 0
    k = torch.arange(fb.shape[0])[:, None]
    first = torch.where(nz, k, fb.shape[0]).amin(0)
    last = torch.where(nz, k, -1).amax(0)
    return int((last - first + 1).clamp(min=1).max())


def hann400(periodic=True):
    return 0.5 - 0.5 * torch.cos(2.0 * math.pi * torch.arange(400, dtype=F64) / (400.0 if periodic else 399.0))


def _dft_tables():
    nk = (torch.arange(400)[:, None] * torch.arange(201)[None, :]) % 400                 # exact angle reduction
    ang = 2.0 * math.pi * nk.double() / 400.0
    return torch.cos(ang), -torch.sin(ang)


def logmel_ref(wav, lens, n_mels, n_samples, pad="reflect", window=None, fold200=1.0, frame_shift=0, bank=None, batch_max=False,
               reflect_about_L=False):
    """wav [B, L] fp32 values, lens list of B lengths or None.  Truncate / zero-pad to n_samples, reflect-pad 200, periodic Hann of 400,
    hop 160, drop the last frame, power, fp32-rounded Slaney bank, log10 with a clamp at 1e-10, per-clip floor max - 8, (x + 4) / 4.
    -> dict: out [B, n_mels, frames]; absX [B, frames, 201]; P [B, frames, n_mels] mel power; E [B, frames] = sum |x_n w_n| of the
    windowed frame; fb.  The keyword arguments are the WRONG readings of the CPU controls (tests/test_ops_ref_cpu.py): symmetric
    padding, another window, sample 200 of every frame weighted fold200 (the fold's forgotten 1/2: 2.0), frames shifted, another bank,
    one maximum for the whole batch, and the end reflected about L - 1 with the samples beyond n_samples read, not cut."""
    x = wav.double()
    B, L = x.shape
    if lens is not None:
        keep = torch.arange(L)[None, :] < torch.tensor(list(lens))[:, None]
        x = torch.where(keep, x, torch.zeros((), dtype=F64))                    # (where, not a product: NaN may stand beyond a length)
    nf = n_samples // 160
    if reflect_about_L and L > n_samples:
        pass                                                                   # wrong: the tail stays, the reflection is about L - 1
    elif L >= n_samples:
        x = x[:, :n_samples]
    else:
        x = F.pad(x, (0, n_samples - L))
    n = x.shape[1]
    if pad == "reflect":
        left, right = x[:, 1:201].flip(1), x[:, n - 201:n - 1].flip(1)
    else:                                                                      # symmetric: the edge sample is repeated
        left, right = x[:, 0:200].flip(1), x[:, n - 200:n].flip(1)
    xp = torch.cat([left, x, right], 1)
    frames = xp.unfold(1, 400, 160)[:, frame_shift:frame_shift + nf]          # [B, nf, 400]
    w = hann400() if window is None else window
    fw = frames * w
    if fold200 != 1.0:
        fw = fw.clone()
        fw[..., 200] *= fold200
    cos, msin = _dft_tables()
    re, im = fw @ cos, fw @ msin
    power = re * re + im * im
    fb = mel_bank(n_mels) if bank is None else bank
    P = power @ fb
    lg = torch.log10(P.clamp(min=1e-10))
    mx = lg.amax(dim=(1, 2), keepdim=True)
    if batch_max:
        mx = mx.amax(dim=0, keepdim=True).expand(B, 1, 1)
    out = (torch.maximum(lg, mx - 8.0) + 4.0) / 4.0
    return {"out": out.transpose(1, 2).contiguous(), "absX": power.sqrt(), "P": P, "E": fw.abs().sum(-1), "fb": fb, "lg": lg, "mx": mx}


# The kernel's DFT (csrc/logmel.hip): Re X_k = sum_{j=1..200} (x_j + x_{400-j}) Wc[j][k], Im likewise with x_j - x_{400-j} and Ws, the
# window folded into fp32-rounded tables, accumulated as a 200-term fp32 fma chain.  Each term carries the fold's rounding and the
# table entry's (2 u, u = 2^-24), the chain at most 200 u of the sum of the terms' magnitudes: (1 + u)^202 - 1 <= 204 u.  With
# m_j = (|x_j| + |x_{400-j}|) w_j >= both folds' magnitudes times the window, the error vector (d Re, d Im) is at most
# gamma sum_j m_j |(cos, sin)| = gamma E in length, E = sum_n |x_n w_n|: |dX_k| <= gamma E, worst case, for this arithmetic.
LOGMEL_GAMMA = 204 * U24
LOGMEL_STORE = 4 * 2.0 ** -23            # the fp32 floor, affine and store of values of order 1
LOGMEL_UNINFORMATIVE = 1e-2              # an element whose bound is wider than this (output units) says nothing


def logmel_bound(r):
    """r: logmel_ref's dict -> the bound [B, n_mels, frames] of |kernel - r["out"]|.
    Power domain: d|X_k|^2 <= 2 |X_k| gamma E + (gamma E)^2, so dP_m = sum_k fb[k][m] (2 |X_k| gamma E + (gamma E)^2) + c_mel u P_m with
    c_mel = mel_maxw + 8 for the fp32 power, the mel sum of at most mel_maxw terms and log10f.  dP goes through log10 exactly (both sides,
    with the 1e-10 clamp); the floor max - 8 moves by the log's error at the reference's arg-max element; max(log, floor) is then bounded
    from both sides; / 4 and the store."""
    fb, P = r["fb"], r["P"]
    gE = (LOGMEL_GAMMA * r["E"])[..., None]                                     # [B, nf, 1]
    dP = (2.0 * r["absX"] * gE + gE * gE) @ fb + (mel_maxw(fb) + 8) * U24 * P
    lg, mx = r["lg"], r["mx"]
    lg_hi = torch.log10((P + dP).clamp(min=1e-10))
    lg_lo = torch.log10((P - dP).clamp(min=1e-10))
    B = P.shape[0]
    flat = lg.reshape(B, -1)
    at = flat.argmax(1)
    ar = torch.arange(B)
    d_floor = torch.maximum(lg_hi.reshape(B, -1)[ar, at] - flat[ar, at], flat[ar, at] - lg_lo.reshape(B, -1)[ar, at])[:, None, None]
    floor = mx - 8.0
    ref = torch.maximum(lg, floor)
    up = torch.maximum(lg_hi, floor + d_floor) - ref
    down = ref - torch.maximum(lg_lo, floor - d_floor)
    return (torch.maximum(up, down) / 4.0 + LOGMEL_STORE).transpose(1, 2).contiguous()


LOGMEL_MODELS = [(80, 16), (80, 100), (128, 16), (128, 100)]                    # (n_mels, max_positions): 32 or 200 frames
LOGMEL_KINDS = ["noise", "dc_noise", "impulses", "tone", "silence"]
LOGMEL_BROADBAND = ["noise", "dc_noise", "impulses"]                            # the kinds the informative-share condition holds on
LOGMEL_SHAPES = ["exact", "longer", "short", "pitch", "ragged"]
LOGMEL_TAIL = 777


def logmel_ragged_lens(n_samples):
    return [n_samples, 5000, 201, 200, 1, 0]


def logmel_signal(kind, n, seed):
    """One clip of n samples (fp32): white noise at 0.1; DC 0.3 + noise at 0.01; unit impulses at 0, 1, 199, 200, 201, n - 201, n - 2,
    n - 1; a tone at 1013.7 Hz over noise 60 dB down; silence."""
    g = _gen(5000 + seed)
    noise = torch.randn(n, generator=g)
    if kind == "noise":
        return 0.1 * noise
    if kind == "dc_noise":
        return 0.3 + 0.01 * noise
    if kind == "impulses":
        x = torch.zeros(n)
        for i in (0, 1, 199, 200, 201, n - 201, n - 2, n - 1):
            if 0 <= i < n:
                x[i] = 1.0
        return x
    if kind == "tone":
        return 0.5 * torch.sin(2.0 * math.pi * 1013.7 / 16000.0 * torch.arange(n, dtype=F64)).float() + 0.5e-3 * noise
    return torch.zeros(n)


def logmel_case(n_samples, shape, fill=float("nan")):
    """The batch of one GPU case -> (wav [B, ldw] fp32, L, lens or None, kinds).  `fill` stands wherever the kernel must not read: the
    row padding behind L ("pitch") and the samples behind each clip's length ("ragged"); the CPU control of an ignored `lens` passes
    None and gets the clips' own continuation there instead.  "longer": 777 samples of 50.0 behind n_samples."""
    if shape == "ragged":
        lens = logmel_ragged_lens(n_samples)
        kinds = ["noise", "dc_noise", "impulses", "tone", "noise", "noise"]
        wav = torch.stack([logmel_signal(k, n_samples, 10 + i) for i, k in enumerate(kinds)])
        if fill is not None:
            for b, n in enumerate(lens):
                wav[b, n:] = fill
        return wav, n_samples, lens, kinds
    kinds = list(LOGMEL_KINDS)
    n = 5000 if shape == "short" else n_samples
    wav = torch.stack([logmel_signal(k, n, i) for i, k in enumerate(kinds)])
    if shape == "longer":
        wav = torch.cat([wav, torch.full((len(kinds), LOGMEL_TAIL), 50.0)], 1)
    if shape == "pitch":
        wav = torch.cat([wav, torch.full((len(kinds), 13), float("nan") if fill is None else fill)], 1)
    return wav, (wav.shape[1] - 13 if shape == "pitch" else wav.shape[1]), None, kinds


# ----------------------------------------------------------------------------------------------------------------- wav_stats
def wav_stats_ref(wav, lens=None):
    """-> (stats [B, 2] float64: sum v, sum v^2 over the first lens[b] samples, exactly rounded; bound [B, 2]).
    Any order of float64 additions of n terms is within (n - 1) 2^-53 sum |terms| of the exact sum (the squares of fp32 values are
    exact in float64): L 2^-53 sum |v| and L 2^-53 sum v^2."""
    B, L = wav.shape
    st, bd = torch.zeros(B, 2, dtype=F64), torch.zeros(B, 2, dtype=F64)
    for b in range(B):
        n = L if lens is None else int(lens[b])
        v = wav[b, :n].double()
        st[b, 0], st[b, 1] = math.fsum(v.tolist()), math.fsum((v * v).tolist())
        bd[b, 0], bd[b, 1] = L * 2.0 ** -53 * math.fsum(v.abs().tolist()), L * 2.0 ** -53 * float(st[b, 1])
    return st, bd


WAV_STATS_L = [1, 1023, 1024, 1025, 70001]


def wav_stats_case(L):
    """-> (wav [4, L + 5] fp32 with NaN behind each length and in the row padding, lens).  Noise at 0.1 on a DC of 0.25."""
    g = _gen(6000 + L)
    wav = 0.25 + 0.1 * torch.randn(4, L + 5, generator=g)
    lens = [L, (L + 1) // 2, 0, min(L, 1)]
    for b, n in enumerate(lens):
        wav[b, n:] = float("nan")
    return wav, lens


# --------------------------------------------------------------------------------------------------------------- clip_frames
def clip_frames_ref(lens, L, kernel, stride, min_len):
    """-> [levels][B] ints: t = clamp(lens[b], 0, L), nothing below min_len, then t <- (t - k) // s + 1 if t >= k else 0 per level."""
    out = [[0] * len(lens) for _ in kernel]
    for b, n in enumerate(lens):
        t = min(max(int(n), 0), L)
        alive = t >= min_len
        for i, (k, s) in enumerate(zip(kernel, stride)):
            t = ((t - k) // s + 1) if (alive and t >= k) else 0
            out[i][b] = t
    return out


WAVLM_STACK = ((10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2))
CLIP_FRAMES_L, CLIP_FRAMES_B = 32000, 300


def clip_frames_lens():
    L = CLIP_FRAMES_L
    edge = [-3, 0, 9, 10, 200, 201, 399, 400, 401, L, L + 5]
    g = _gen(7000)
    rest = torch.randint(0, L + 1, (CLIP_FRAMES_B - len(edge),), generator=g).tolist()
    return rest[:250] + edge + rest[250:]                                        # the edges in the second block of 256 clips


# --------------------------------------------------------------------------------------------------------------- WavLM conv0
def conv0_frames(n):
    return (n - 10) // 5 + 1 if n >= 10 else 0


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def conv0_ref(wav, lens, normalize, w, bias, gamma, beta, mode, with_scale=False, reverse_taps=False, unbiased=False, gn_eps=1e-5,
              stats_T=None, mean_over_L=False, ln_div=None, tanh=False):
    """Level 0 of WavLM's feature encoder in float64.  wav [B, L] fp32 values; lens list or None; normalize: (x - mean) / sqrt(var + 1e-7)
    with the biased variance over the clip's own lens[b] samples; conv1d k = 10, stride 5, no padding, tap 0 at the earliest sample;
    mode "group": per-(clip, channel) statistics over the clip's own frames, eps 1e-5 (a bias, when given, is added -- and cancels);
    mode "layer": + bias, LayerNorm over the C channels, eps 1e-5; exact-erf GELU.
    -> out [B, T0, C] (T0 from L; rows beyond a clip's own frames zero), and with_scale: what an fp32 error scales with,
       |gamma| r (|y - mu| + |mu| + 1 / r + A) + |beta|,  A = sum_j |w_j x_j|  (conv0_bound).
    The other keyword arguments are the controls' WRONG readings: taps reversed, unbiased GroupNorm variance, another GroupNorm eps,
    GroupNorm sums divided by stats_T frames instead of the clip's, waveform sums divided by L instead of lens[b], the LayerNorm
    divisor ln_div instead of C, tanh-GELU."""
    B, L = wav.shape
    C = w.shape[0]
    T0 = conv0_frames(L)
    wd = w.double().flip(-1) if reverse_taps else w.double()
    g, bt = gamma.double(), beta.double()
    out = torch.zeros(B, T0, C, dtype=F64)
    scale = torch.zeros(B, T0, C, dtype=F64)
    for b in range(B):
        n = L if lens is None else int(lens[b])
        Tb = conv0_frames(n)
        if Tb == 0:
            continue
        x = wav[b, :n].double()
        if normalize:
            div = L if mean_over_L else n
            m = x.sum() / div
            var = (x * x).sum() / div - m * m if mean_over_L else ((x - m) ** 2).sum() / n
            x = (x - m) / torch.sqrt(var.clamp(min=0.0) + 1e-7)
        win = x.unfold(0, 10, 5)[:Tb]                                            # [Tb, 10]
        y = win @ wd.T                                                           # [Tb, C]
        A = win.abs() @ wd.abs().T
        if bias is not None:
            y = y + bias.double()
        if mode == "group":
            div = Tb if stats_T is None else stats_T
            mu = y.sum(0, keepdim=True) / div
            if stats_T is None:
                var = ((y - mu) ** 2).sum(0, keepdim=True) / ((Tb - 1) if unbiased else Tb)
            else:
                var = ((y * y).sum(0, keepdim=True) / div - mu * mu).clamp(min=0.0)
            r = (var + gn_eps) ** -0.5
        else:
            div = C if ln_div is None else ln_div
            mu = y.sum(1, keepdim=True) / div
            var = ((y - mu) ** 2).sum(1, keepdim=True) / C if ln_div is None else ((y * y).sum(1, keepdim=True) / div - mu * mu).clamp(min=0.0)
            r = (var + 1e-5) ** -0.5
        v = g * (y - mu) * r + bt
        out[b, :Tb] = gelu_tanh(v) if tanh else F.gelu(v)
        scale[b, :Tb] = g.abs() * r * ((y - mu).abs() + mu.abs() + 1.0 / r + A) + bt.abs()
    return (out, scale) if with_scale else out


def _fma32(a, b, c):
    """fmaf on fp32 tensors: the product of two fp32 values is exact in float64; one float64 addition, then the rounding to fp32."""
    return (a.double() * b.double() + c.double()).float()


def gelu_f32(x):
    """csrc/common.h's gelu_erf in fp32: max(x, 0) - |x| 2^q(|x|), q the degree-5 fit of log2 Phi(-t)."""
    t = x.abs()
    f = lambda c: torch.full_like(t, c)                                         # noqa: E731
    q = _fma32(f(-4.732937668e-04), t, f(7.084457669e-03))
    for c in (-5.182715505e-02, -4.599926770e-01, -1.150787711e+00, -1.000037670e+00):
        q = _fma32(q, t, f(c))
    return _fma32(-t, torch.exp2(q), x.clamp(min=0.0))


def conv0_f32(wav, lens, normalize, w, bias, gamma, beta, mode):
    """A float32 restatement of csrc/wavlm.hip's arithmetic on the CPU, for the measurement of CONV0_LAMBDA only: the waveform statistics
    in float64 and mean / rstd rounded to fp32, (x - mean) * rstd in fp32, the ten taps as an fma chain with tap 0 first; group mode:
    fp32 sums of y and y^2 in frame order per block of 512 frames, the blocks added in float64, var = E[y^2] - m^2 in float64, the affine
    folded into y * sc + sh; layer mode: the chain starts at the bias, eight channels per lane summed in order and the 64 lanes by an
    xor butterfly, the variance centred; the polynomial GELU of common.h.  -> the fp32 values before the bf16 store, [B, T0, C]."""
    B, L = wav.shape
    C = w.shape[0]
    T0 = conv0_frames(L)
    wf, gm, bt = w.float(), gamma.float(), beta.float()
    out = torch.zeros(B, T0, C, dtype=torch.float32)
    for b in range(B):
        n = L if lens is None else int(lens[b])
        Tb = conv0_frames(n)
        if Tb == 0:
            continue
        x = wav[b, :n].float()
        if normalize:
            s, q = x.double().sum(), (x.double() ** 2).sum()
            m = s / n
            var = q / n - m * m
            x = (x - m.float()) * (1.0 / torch.sqrt(var.clamp(min=0.0) + 1e-7)).float()
        win = x.unfold(0, 10, 5)[:Tb]                                            # [Tb, 10]
        y = (bias.float()[None, :].expand(Tb, C) if (bias is not None and mode == "layer") else torch.zeros(Tb, C)).contiguous()
        for j in range(10):
            y = _fma32(wf[None, :, j].expand(Tb, C), win[:, j:j + 1].expand(Tb, C), y)
        if mode == "group":
            S, Q = torch.zeros(C, dtype=F64), torch.zeros(C, dtype=F64)
            for t0 in range(0, Tb, 512):
                sa, qa = torch.zeros(C), torch.zeros(C)
                for t in range(t0, min(t0 + 512, Tb)):
                    sa = sa + y[t]
                    qa = _fma32(y[t], y[t], qa)
                S, Q = S + sa.double(), Q + qa.double()
            m = S / Tb
            var = Q / Tb - m * m
            sc = (1.0 / torch.sqrt(var.clamp(min=0.0) + 1e-5)).float() * gm
            sh = _fma32(-m.float(), sc, bt)
            v = _fma32(y, sc[None, :].expand(Tb, C), sh[None, :].expand(Tb, C))
        else:
            def lanes(z):                                                        # [Tb, C] -> the wave's sum: 8 per lane in order, butterfly
                zl = F.pad(z, (0, 512 - C)).view(Tb, 64, 8)
                acc = torch.zeros(Tb, 64)
                for e in range(8):
                    acc = acc + zl[:, :, e]
                idx = torch.arange(64)
                for o in (32, 16, 8, 4, 2, 1):
                    acc = acc + acc[:, idx ^ o]
                return acc[:, :1]
            mu = lanes(y) / C
            d = y - mu
            zl = F.pad(d, (0, 512 - C)).view(Tb, 64, 8)
            acc = torch.zeros(Tb, 64)
            for e in range(8):
                acc = _fma32(zl[:, :, e], zl[:, :, e], acc)
            idx = torch.arange(64)
            for o in (32, 16, 8, 4, 2, 1):
                acc = acc + acc[:, idx ^ o]
            rs = 1.0 / torch.sqrt(acc[:, :1] / C + 1e-5)
            v = _fma32(d * rs, gm[None, :].expand(Tb, C), bt[None, :].expand(Tb, C))
        out[b, :Tb] = gelu_f32(v)
    return out


# (mode, C, T0, r, ragged, wstats, bias, pair): L = 5 (T0 - 1) + 10 + r; ragged: lens = [L, 5 * 199 + 13, 9]; T0 = 8200: the layer
# kernel's grid-stride path (its grid stops at 2048 blocks of four frames).  Group mode does not read the bias: one case passes one.
CONV0_CASES = [
    ("group", 8, 1, 0, False, True, False, False), ("group", 8, 3, 4, False, False, False, True),
    ("group", 32, 3, 0, False, True, False, True), ("group", 32, 511, 4, True, True, False, False),
    ("group", 32, 512, 0, True, False, False, True), ("group", 32, 513, 4, False, True, False, True),
    ("group", 8, 513, 0, True, True, False, False), ("group", 512, 1, 4, False, True, False, True),
    ("group", 512, 513, 0, True, True, False, True), ("group", 512, 1030, 4, True, True, False, False),
    ("group", 32, 1030, 0, False, False, False, True), ("group", 512, 512, 4, False, True, True, False),
    ("group", 8, 1030, 0, True, False, False, True),
    ("layer", 8, 1, 0, False, True, True, False), ("layer", 8, 3, 4, False, False, False, True),
    ("layer", 32, 3, 0, False, True, True, True), ("layer", 32, 511, 4, True, True, True, True),
    ("layer", 32, 512, 0, False, True, False, False), ("layer", 8, 513, 4, True, False, True, True),
    ("layer", 512, 1, 0, False, True, True, True), ("layer", 512, 513, 4, True, True, True, False),
    ("layer", 512, 1030, 0, True, True, True, True), ("layer", 32, 1030, 4, False, False, True, False),
    ("layer", 512, 3, 4, False, True, True, False), ("layer", 32, 8200, 0, True, True, True, True),
    ("layer", 32, 8200, 4, False, True, False, False),
]
CONV0_RAGGED_LEN = 5 * 199 + 13
CONV0_LOWVAR = 2                          # channel with weights 100 x smaller: conv variance ~1e-5, where GroupNorm's eps matters


def conv0_id(case):
    mode, C, T0, r, ragged, ws, bias, pair = case
    return f"{mode}_C{C}_T{T0}_r{r}_ragged{int(ragged)}_ws{int(ws)}_bias{int(bias)}_pair{int(pair)}"


def conv0_inputs(case, fill=float("nan")):
    """-> dict.  wav [3, L]: noise at 0.1 + DC 0.02 + a slow sine, clip 2 all zero; ragged: `fill` behind each length.  Weights N(0, 0.1),
    channel 0 all positive, channel 1 all zero (variance 0: the output is gelu(beta) in group mode), channel 2 scaled by 0.01."""
    mode, C, T0, r, ragged, ws, bias, pair = case
    L = 5 * (T0 - 1) + 10 + r
    g = _gen(8000 + C + 7 * T0 + r)
    t = torch.arange(L, dtype=F64)
    wav = 0.1 * torch.randn(3, L, generator=g) + 0.02 + (0.05 * torch.sin(2.0 * math.pi * t / 3000.0)).float()[None, :]
    wav[2] = 0.0
    lens = [L, CONV0_RAGGED_LEN, 9] if ragged else None
    if ragged and fill is not None:
        for b, n in enumerate(lens):
            wav[b, n:] = fill
    w = 0.1 * torch.randn(C, 10, generator=g)
    w[0] = w[0].abs() + 0.01
    w[1] = 0.0
    w[CONV0_LOWVAR] *= 0.01
    return {"mode": mode, "C": C, "T0": T0, "L": L, "lens": lens, "normalize": ws, "pair": pair, "wav": wav, "w": w,
            "bias": 0.2 * torch.randn(C, generator=g) if bias else None, "gamma": 1.0 + 0.1 * torch.randn(C, generator=g),
            "beta": 0.1 * torch.randn(C, generator=g)}


def conv0_case_ref(c, **wrong):
    return conv0_ref(c["wav"], c["lens"], c["normalize"], c["w"], c["bias"], c["gamma"], c["beta"], c["mode"], with_scale=True, **wrong)


def conv0_valid(c):
    n = torch.tensor([c["T0"]] * 3 if c["lens"] is None else [conv0_frames(x) for x in c["lens"]])
    return torch.arange(c["T0"])[None, :] < n[:, None]


# bound: the store -- 2^-8 |ref| for hi alone, as posconv_bound's bf16 store, 2^-15 |ref| for a hi + lo pair -- plus CONV0_LAMBDA * scale,
# scale = |gamma| r (|y - mu| + |mu| + 1 / r + A) + |beta|: layernorm_bound's form with the conv's own magnitude A = sum_j |w_j x_j| added.
# CONV0_LAMBDA = 4 x the largest err / scale of conv0_f32 (the CPU restatement of the kernel's fp32 arithmetic, before the store) against
# conv0_ref over CONV0_CASES; the 4 covers what the device's exp2, rsqrt and reciprocal do differently by a few ulp.  It is never fitted
# to the kernel's output.  tests/test_ops_ref_cpu.py::test_conv0_lambda_is_the_restatements recomputes the measurement.
# Measured on the CPU: 2.5e-7 .. 5.2229e-7 over the 26 cases; the largest at group_C512_T1_r4_ragged0_ws1_bias0_pair1 -- one frame, so
# y = mu and the affine y * sc + sh cancels two numbers of size |mu| r |gamma| ~ 100 (the |mu| term of the scale), on top of the
# polynomial GELU's own 6.4e-7.  (What the kernel itself came to on MI355X: the table in tests/test_gpu_ops_frontend.py.)
CONV0_LAMBDA_MEASURED = 5.2229e-7
CONV0_LAMBDA = 4 * CONV0_LAMBDA_MEASURED


def conv0_bound(ref, scale, pair):
    return (2.0 ** -15 if pair else 2.0 ** -8) * ref.abs() + CONV0_LAMBDA * scale


def frac_outside_nan(wrong, right, bound, factor=2.0):
    """frac_outside, with a wrong reference that is not finite counted as outside (no finite output can be near it)."""
    return float((((wrong - right).abs() > factor * bound) | ~torch.isfinite(wrong)).double().mean())


# ------------------------------------------------------------------------------------------------------------------ GEMM modes
# Float64 references of what one GemmArgs launch computes (csrc/common.h; include/wfl_asr.h, wfl_op_gemm_ex), piece by piece, for
# tests/test_gpu_ops_gemm_modes.py.  Every function takes the operand VALUES the kernel reads (bf16 values, e4m3 bytes decoded, fp32
# scales) as float64 matrices of the VALID rows only -- gathering rows out of the frame-row buffers is the test's business -- and
# returns the value together with `mag`, the same expression with every term replaced by its absolute value: the scale an fp32
# accumulation error is proportional to, and what the tests' tolerances hang on.
def e4m3_decode(b):
    """uint8 tensor of OCP e4m3 (fn) bytes -> float64, by the format's definition: 1 sign, 4 exponent (bias 7), 3 mantissa bits, no
    infinities, S.1111.111 = NaN, exponent 0 subnormal."""
    b = b.to(torch.int64)
    s, e, m = b >> 7, (b >> 3) & 15, b & 7
    v = torch.where(e == 0, m.double() / 8 * 2.0 ** -6, (1 + m.double() / 8) * torch.exp2((e - 7).double()))
    v = torch.where((e == 15) & (m == 7), torch.full_like(v, math.nan), v)
    return torch.where(s == 1, -v, v)


def gemm_ref(a, w, bias=None, row_scale=None, col_scale=None):
    """a [M, K], w [N, K] values; row_scale [M] (fp8 activations' per-row scale), col_scale [N] (fp8 weights' per-channel scale).
    -> (v, mag) [M, N]:  v = rs_m cs_n sum_k a w + bias,  mag = |rs_m| |cs_n| sum_k |a| |w| + |bias|."""
    a, w = a.to(F64), w.to(F64)
    v, mag = a @ w.T, a.abs() @ w.abs().T
    if col_scale is not None:
        v, mag = v * col_scale.to(F64)[None, :], mag * col_scale.to(F64).abs()[None, :]
    if row_scale is not None:
        v, mag = v * row_scale.to(F64)[:, None], mag * row_scale.to(F64).abs()[:, None]
    if bias is not None:
        v, mag = v + bias.to(F64), mag + bias.to(F64).abs()
    return v, mag


def gemm_table_terms(v, mag, B, T, clip_bias=None, clip_idx=None, act=None, pos=None):
    """The per-clip bias row (before the activation) and the positional table (after it) of a [B * T, N] result:
         v = act(v + clip_bias[clip_idx[b]][n]) + pos[t][n].
    clip_bias [rows, >= N], clip_idx list of B rows, pos [>= T, >= N]; act None / "gelu" / "relu".  mag follows (an activation with
    Lipschitz constant L leaves at most L mag: the caller applies its factor)."""
    N = v.shape[1]
    v, mag = v.view(B, T, N).clone(), mag.view(B, T, N).clone()
    if clip_bias is not None:
        cb = clip_bias.to(F64)[torch.as_tensor(list(clip_idx), dtype=torch.long)][:, None, :N]
        v, mag = v + cb, mag + cb.abs()
    if act == "gelu":
        v = F.gelu(v)
    elif act == "relu":
        v = F.relu(v)
    elif act is not None:
        raise ValueError(act)
    if pos is not None:
        pt = pos.to(F64)[None, :T, :N]
        v, mag = v + pt, mag + pt.abs()
    return v.reshape(B * T, N), mag.reshape(B * T, N)


def residual_pair_ref(v, mag, res_hi, res_lo=None, alpha=1.0):
    """out = res_hi + res_lo + alpha v  (the residual stream as a bf16 pair, GemmArgs::res / res_lo / alpha)."""
    out, m = res_hi.to(F64) + alpha * v, res_hi.to(F64).abs() + abs(alpha) * mag
    if res_lo is not None:
        out, m = out + res_lo.to(F64), m + res_lo.to(F64).abs()
    return out, m


def ragged_mask(B, T, clip_T=None):
    """bool [B, T]: the frames a launch stores -- t < T and t < clip_T[b]."""
    n = torch.tensor([T] * B if clip_T is None else [min(int(x), T) for x in clip_T])
    return torch.arange(T)[None, :] < n[:, None]


def tile_stats_ref(c):
    """The statistics producer (GemmArgs::stats_out): c [M, N] the bf16 values stored in C, N % 256 == 0.
    -> (stats [M, N / 256, 2], scale [M, N / 256, 2]): per row and 256-column tile (sum, sum of squares), and the absolute sums
    (sum |x|, sum x^2) a 256-term fp32 summation's error is proportional to."""
    M, N = c.shape
    t = c.to(F64).view(M, N // 256, 256)
    sq = (t * t).sum(-1)
    return torch.stack([t.sum(-1), sq], -1), torch.stack([t.abs().sum(-1), sq], -1)


def row_stats_slots(a, nsl):
    """What a producer leaves for a consumer whose K = 256 nsl: a [M, K] -> fp32 [M, 4, 2], slot j < nsl = (sum, sum of squares) of columns
    256 j .. 256 j + 255 (summed in float64, rounded once); the unused slots hold NaN -- a consumer must not read them."""
    M, K = a.shape
    assert K == 256 * nsl and 1 <= nsl <= 4
    st, _ = tile_stats_ref(a)
    out = torch.full((M, 4, 2), math.nan, dtype=torch.float32, device=a.device)
    out[:, :nsl] = st.float()
    return out


def ln_fold_ref(a, w, bias, stats, nsl, eps=1e-5, ln_s=None):
    """LayerNorm folded into the consuming GEMM, statistics given (GemmArgs::ln_s + stats_in):
         mean = sum_j stats[m, j, 0] / K,  var = sum_j stats[m, j, 1] / K - mean^2,  rstd = (var + eps)^-1/2,
         v = rstd (a w^T - mean ln_s) + bias,        ln_s[n] = sum_k w[n][k] unless given.
    a [M, K], w [N, K] (gamma already folded in), stats [M, >= nsl, 2].
    -> (v, mag, cancel): mag = rstd (sum |a||w| + |mean| sum |w|) (the bias is added once, exactly: no part of it);  cancel = (E[x^2] / var) |v - bias|, the factor by which the
    one-pass variance E[x^2] - mean^2 amplifies a relative error of its two terms, times the part of v that rstd multiplies."""
    a, w = a.to(F64), w.to(F64)
    K = a.shape[1]
    s = stats.to(F64)[:, :nsl].sum(1)
    mean, ex2 = s[:, 0] / K, s[:, 1] / K
    var = (ex2 - mean * mean).clamp_min(0)
    rstd = (var + eps) ** -0.5
    ls = w.sum(1) if ln_s is None else ln_s.to(F64)
    core = rstd[:, None] * (a @ w.T - mean[:, None] * ls[None, :])
    mag = rstd[:, None] * (a.abs() @ w.abs().T + mean.abs()[:, None] * w.abs().sum(1)[None, :])
    b = 0.0 if bias is None else bias.to(F64)[None, :]
    cancel = (ex2 / var.clamp_min(1e-300))[:, None] * core.abs()
    return core + b, mag, cancel


# Tolerances of the GEMM-mode tests: derived from the number formats, never from what a kernel gives.
GELU_LIPSCHITZ = 1.2          # max |gelu'| = 1.13


def tol_bf16(ref, mag, K, lip=1.0):
    """one bf16 rounding of the stored value + an fp32 accumulation over K terms"""
    return 2.0 ** -8 * ref.abs() + lip * K * 2.0 ** -24 * mag


def tol_pair(ref, mag, K):
    """a hi + lo pair keeps sixteen significant bits of the sum"""
    return 2.0 ** -15 * ref.abs() + K * 2.0 ** -24 * mag


def tol_ln_fold(ref, mag, cancel, K, lip=1.0):
    """tol_bf16 + the one-pass variance's cancellation: fp32 sums carry ~2^-23 each, two of them, amplified by E[x^2] / var"""
    return 2.0 ** -8 * ref.abs() + lip * (K * 2.0 ** -24 * mag + 2.0 ** -22 * cancel)
