"""Plain float64 references of the WavLM-path kernels and of attention's bias / ragged / split modes, and the seeded inputs of the
operator tests (tests/test_gpu_ops_wavlm.py runs the kernels on them, tests/test_ops_ref_cpu.py checks the references themselves and
that each test's bound separates a right reference from a wrong one).  Everything here runs on the CPU.

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
