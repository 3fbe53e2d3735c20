"""CPU: the float64 references of tests/ops_ref.py.  (1) They agree with the oracle's formulation of the same operations on fp32 random
input.  (2) Wrong-reference controls: on each GPU case's own inputs (the same seeded functions, run here on the CPU) a deliberately
wrong reference lies further than twice that case's bound from the right one on at least 5 % of the compared elements -- so an output
that passes the GPU test cannot be an output of the wrong computation."""
import math

import pytest
import torch
import torch.nn.functional as F

import ops_ref as R
from oracle import wfl_oracle as O

MIN_SHARE = 0.05


# ------------------------------------------------------------------------------------------------- agreement with the oracle
def test_attention_gate_and_table_references_agree_with_the_oracle():
    """oracle/wfl_oracle.py:280-296: bucketed position bias, gate, softmax(q k^T hd^-1/2 + gate * bias) v."""
    g = torch.Generator().manual_seed(1)
    B, T, heads, hd, nb, md, max_t = 2, 40, 3, 16, 32, 20, 64
    d = heads * hd
    h = torch.randn(B, T, d, generator=g)
    q, k, v = (torch.randn(B, T, d, generator=g) for _ in range(3))
    sd = {"g.weight": torch.randn(8, hd, generator=g) * 0.3, "g.bias": torch.randn(8, generator=g) * 0.3}
    const = torch.rand(1, heads, 1, 1, generator=g) + 0.5
    rel_emb = torch.randn(nb, heads, generator=g)
    # the oracle
    buckets = O._wavlm_rel_buckets(T, nb, md)
    pos_bias = rel_emb[buckets].permute(2, 0, 1)
    gh = h.view(B, T, heads, hd).permute(0, 2, 1, 3)
    proj = O._linear(gh, sd, "g").view(B, heads, T, 2, 4).sum(-1)
    ga, gb = torch.sigmoid(proj).chunk(2, dim=-1)
    gate = ga * (gb * const - 1.0) + 2.0
    bias = gate * pos_bias[None]
    qh = q.view(B, T, heads, hd).transpose(1, 2) * hd ** -0.5
    kh = k.view(B, T, heads, hd).transpose(1, 2)
    vh = v.view(B, T, heads, hd).transpose(1, 2)
    want = (torch.softmax(qh @ kh.transpose(2, 3) + bias, dim=-1) @ vh).transpose(1, 2).reshape(B, T, d)
    # the references, in the kernels' units: q scaled by hd^-1/2 log2 e, the table by log2 e
    full = O._wavlm_rel_buckets(max_t, nb, md)
    bod = torch.cat([full[1:, 0].flip(0), full[0, :]]).to(torch.int32)         # delta = -(max_t-1) .. max_t-1
    log2e = math.log2(math.e)
    table = R.relpos_table_ref(rel_emb.double() * log2e, bod, max_t, T)
    gate_r = R.relpos_gate_ref(h.double(), heads, sd["g.weight"], sd["g.bias"], const.reshape(heads))
    assert float((gate_r - gate[..., 0].double()).abs().max()) <= 1e-5
    got, _ = R.attention_ref(q.double() * hd ** -0.5 * log2e, k.double(), v.double(), heads, table, gate_r)
    assert float((got - want.double()).abs().max()) <= 1e-5


def test_posconv_reference_agrees_with_the_oracle():
    """oracle/wfl_oracle.py:272-275: x + gelu(conv1d(x, w, b, padding = K/2, groups)[..., :-1]); the reference multiplies unfolded windows
    with the PACKED weights instead."""
    g = torch.Generator().manual_seed(2)
    for groups, cpg, K in ((4, 16, 16), (2, 24, 8)):
        B, T, d = 2, 37, groups * cpg
        x = torch.randn(B, T, d, generator=g)
        w = torch.randn(d, cpg, K, generator=g) / math.sqrt(cpg * K)
        b = torch.randn(d, generator=g)
        pos = F.conv1d(x.transpose(1, 2), w, b, padding=K // 2, groups=groups)
        pos = pos[:, :, :-1]
        want = x + F.gelu(pos).transpose(1, 2)
        W, bias = R.pack_posconv(w, b, groups)
        got = R.posconv_ref(x, x, W, bias, cpg, K)
        assert float((got - want.double()).abs().max()) <= 1e-5
        # a shorter clip is the clip alone
        got2 = R.posconv_ref(x, x, W, bias, cpg, K, clip_T=[T, 11])
        alone = R.posconv_ref(x[1:, :11], x[1:, :11], W, bias, cpg, K)
        assert torch.equal(got2[0], got[0]) and float((got2[1, :11] - alone[0]).abs().max()) <= 1e-12 and bool((got2[1, 11:] == 0).all())


def test_layernorm_reference_agrees_with_torch():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 7, 128, generator=g) * 3 + 1
    gamma, beta = torch.randn(128, generator=g), torch.randn(128, generator=g)
    want = F.layer_norm(x, (128,), gamma, beta, 1e-5)
    assert float((R.layernorm_ref(x, gamma, beta, 1e-5) - want.double()).abs().max()) <= 1e-5
    assert float((R.layernorm_ref(x, gamma, beta, 1e-5, gelu=True) - F.gelu(want).double()).abs().max()) <= 1e-5
    # n_div: the statistics of the first 80 channels alone
    x[..., 80:] = 0
    want80 = F.layer_norm(x[..., :80], (80,), gamma[:80], beta[:80], 1e-5)
    assert float((R.layernorm_ref(x, gamma, beta, 1e-5, n_div=80)[..., :80] - want80.double()).abs().max()) <= 1e-5


def test_regroup_reference():
    buf = torch.arange(40 * 32, dtype=torch.float32).view(40, 32)
    xg = R.regroup_ref(buf, 2, 16, 4, 2, 16, 10, clip_T=[10, 3])
    assert xg.shape == (2, 40, 64) and bool((xg[:, :, 16:] == 0).all()) and bool((xg[:, :4] == 0).all())
    assert torch.equal(xg[1, 4 + 16 + 2, :16], buf[4 + 16 + 2, 16:]) and bool((xg[:, 4 + 16 + 3:] == 0).all())
    assert bool((xg[:, 14:20] == 0).all())


# ------------------------------------------------------------------------------------------------- wrong-reference controls
def _valid(c):
    n = torch.tensor([c["T"]] * c["B"] if c["clip_T"] is None else c["clip_T"])
    return torch.arange(c["T"])[None, :] < n[:, None]


def _attn_bound(c, ref, A):
    return R.attn_bound_split(ref, A) if c["pair"] else R.attn_bound_bf16(ref)


def _wrong(c, **over):
    q, k, v = R.attn_values(c, drop_lo=over.pop("drop_lo", False))
    a = {"table": c["table"], "gate": c["gate"], "clip_T": c["clip_T"]}
    a.update(over)
    return R.attention_ref(q, k, v, c["heads"], a["table"], a["gate"], a["clip_T"])[0]


def _share(c, wrong, ref, A):
    m = _valid(c)
    return R.frac_outside(wrong[m], ref[m], _attn_bound(c, ref, A)[m])


@pytest.mark.parametrize("hd,heads,T", R.ATTN_BIAS_CASES)
def test_control_bias_cases(hd, heads, T):
    c = R.bias_case(hd, heads, T)
    ref, A = R.attn_case_ref(c)
    shifted = _wrong(c, table=torch.roll(c["table"], 1, dims=1))                 # table shifted by one entry
    neighbour = _wrong(c, gate=torch.roll(c["gate"], 1, dims=1))                 # gate of the neighbouring head
    assert _share(c, shifted, ref, A) >= MIN_SHARE and _share(c, neighbour, ref, A) >= MIN_SHARE


@pytest.mark.parametrize("variant,hd", R.ATTN_CLIP_CASES)
def test_control_clip_cases(variant, hd):
    c = R.clip_case(variant, hd)
    ref, A = R.attn_case_ref(c)
    at_T = _wrong(c, clip_T=None)                                                # keys masked at T instead of clip_T[b]
    assert _share(c, at_T, ref, A) >= MIN_SHARE
    if variant == "bias":
        own = _wrong(c, gate=R.gate_own_length(c["gate"], c["clip_T"]))          # gate indexed with the clip's own length
        shifted = _wrong(c, table=torch.roll(c["table"], 1, dims=1))
        assert _share(c, own, ref, A) >= MIN_SHARE and _share(c, shifted, ref, A) >= MIN_SHARE
    if variant == "split":
        assert _share(c, _wrong(c, drop_lo=True), ref, A) >= MIN_SHARE


@pytest.mark.parametrize("hd,bias", R.ATTN_SPLIT_CASES)
def test_control_split_cases(hd, bias):
    c = R.split_case(hd, bias)
    ref, A = R.attn_case_ref(c)
    assert _share(c, _wrong(c, drop_lo=True), ref, A) >= MIN_SHARE               # lo halves dropped, at the measured kappa
    if bias:
        assert _share(c, _wrong(c, table=torch.roll(c["table"], 1, dims=1)), ref, A) >= MIN_SHARE


@pytest.mark.parametrize("groups,cpg,taps", R.POSCONV_CASES)
@pytest.mark.parametrize("pair", [False, True])
def test_control_posconv_taps_shifted_by_one_frame(groups, cpg, taps, pair):
    c = R.posconv_case(groups, cpg, taps, pair)
    x, res = c["x_hi"].double(), c["x_hi"].double() + c["x_lo"].double()
    for clip_T in (None, R.POSCONV_CLIP_T):
        ref, mag = R.posconv_ref(x, res, c["W"], c["bias"], cpg, taps, clip_T, with_mag=True)
        wrong = R.posconv_ref(torch.roll(x, 1, dims=1), res, c["W"], c["bias"], cpg, taps, clip_T)
        n = torch.tensor([c["T"]] * c["B"] if clip_T is None else clip_T)
        m = torch.arange(c["T"])[None, :] < n[:, None]
        assert R.frac_outside(wrong[m], ref[m], R.posconv_bound(ref, mag, pair)[m]) >= MIN_SHARE


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("gelu", [False, True])
def test_control_layernorm_statistics_over_all_columns(pair, gelu):
    c = R.layernorm_inputs(128, 80, 3, R.LN_T, pair)
    x = c["x_hi"].double() + c["x_lo"].double()
    ref, scale = R.layernorm_ref(x, c["gamma"], c["beta"], 1e-5, 80, gelu, with_scale=True)
    wrong = R.layernorm_ref(x, c["gamma"], c["beta"], 1e-5, 0, gelu)             # statistics over C instead of n_div
    assert R.frac_outside(wrong, ref, R.layernorm_bound(ref, scale, pair)) >= MIN_SHARE


@pytest.mark.parametrize("C,n_div,offset", [(64, 0, False), (2048, 0, False), (128, 80, False), (768, 0, True)])
def test_control_layernorm_low_halves_dropped(C, n_div, offset):
    """The pair bound with its measured lambda leaves no room for a kernel that reads x without x_lo."""
    c = R.layernorm_inputs(C, n_div, 3, R.LN_T, True, offset=offset)
    ref, scale = R.layernorm_ref(c["x_hi"].double() + c["x_lo"].double(), c["gamma"], c["beta"], 1e-5, n_div, False, with_scale=True)
    wrong = R.layernorm_ref(c["x_hi"].double(), c["gamma"], c["beta"], 1e-5, n_div, False)
    assert R.frac_outside(wrong, ref, R.layernorm_bound(ref, scale, True)) >= MIN_SHARE
