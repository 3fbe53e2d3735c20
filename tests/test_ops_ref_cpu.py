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


# ====================================================================================================== the front-end kernels
# (tests/test_gpu_ops_frontend.py runs the kernels on the same seeded inputs)
from types import SimpleNamespace


def _report(what, share):
    print(f"control {what}: {share:.3f} of the reachable elements beyond twice the bound")
    return share


# ------------------------------------------------------------------------------------------------- agreement with the oracle
@pytest.mark.parametrize("n_mels", [80, 128])
def test_logmel_reference_agrees_with_the_oracle(n_mels):
    """oracle/wfl_oracle.py, whisper_log_mel (torch.stft in fp32): shorter than, equal to and longer than n_samples, and `lens` as explicit
    zero padding.  Tolerance: the fp32 transform's own error on broadband input (5.5e-5 at most on the inputs tried), 1e-4."""
    g = torch.Generator().manual_seed(4)
    n = 32000
    for L in (n, 5000, n + 777):
        wav = 0.1 * torch.randn(2, L, generator=g)
        want = O.whisper_log_mel(wav, n_mels, n).double()
        r = R.logmel_ref(wav, None, n_mels, n)
        assert r["out"].shape == want.shape and float((r["out"] - want).abs().max()) <= 1e-4
        # ... and that fp32 path lies inside the bound, with room: a right output passes
        assert float(((r["out"] - want).abs() / R.logmel_bound(r)).max()) <= 0.5
    wav = 0.1 * torch.randn(3, n, generator=g)
    lens = [n, 7001, 0]
    padded = wav.clone()
    for b, k in enumerate(lens):
        padded[b, k:] = 0.0
    wav[1, 7001:] = float("nan")
    assert torch.equal(R.logmel_ref(wav, lens, n_mels, n)["out"], R.logmel_ref(padded, None, n_mels, n)["out"])
    assert bool((R.logmel_ref(wav, lens, n_mels, n)["out"][2] == -1.5).all())          # no sample at all: the clamp, floored by itself


@pytest.mark.parametrize("mode", ["group", "layer"])
@pytest.mark.parametrize("normalize", [False, True])
def test_conv0_reference_agrees_with_the_oracle(mode, normalize):
    """oracle/wfl_oracle.py: level 0 of wavlm_feature_encoder after wavlm_normalize (F.conv1d, F.group_norm / F.layer_norm, F.gelu in fp32)."""
    g = torch.Generator().manual_seed(5)
    C, L = 24, 1234
    wav = 0.1 * torch.randn(2, L, generator=g) + 0.03
    w = 0.1 * torch.randn(C, 10, generator=g)
    bias = 0.2 * torch.randn(C, generator=g) if mode == "layer" else None
    gamma, beta = 1.0 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    p = "encoder.feature_extractor.conv_layers.0."
    sd = {p + "conv.weight": w[:, None, :], p + "layer_norm.weight": gamma, p + "layer_norm.bias": beta}
    if bias is not None:
        sd[p + "conv.bias"] = bias
    arch = SimpleNamespace(conv_kernel=(10,), conv_stride=(5,), feat_extract_norm=mode)
    want = O.wavlm_feature_encoder(O.wavlm_normalize(wav, normalize), sd, arch).double()
    got = R.conv0_ref(wav, None, normalize, w, bias, gamma, beta, mode)
    assert got.shape == want.shape == (2, O.wavlm_num_frames(L, arch), C)
    assert float((got - want).abs().max()) <= 1e-5
    # a shorter clip is the clip alone, and nothing beyond its own frames
    got2 = R.conv0_ref(wav, [L, 509], normalize, w, bias, gamma, beta, mode)
    alone = R.conv0_ref(wav[1:, :509], None, normalize, w, bias, gamma, beta, mode)
    assert torch.equal(got2[0], got[0]) and torch.equal(got2[1, :100], alone[0]) and bool((got2[1, 100:] == 0).all())


def test_conv0_lambda_is_the_restatements():
    """ops_ref.CONV0_LAMBDA is four times what the float32 restatement of the kernel's arithmetic (conv0_f32) measures against conv0_ref
    over every case of the GPU test, on the CPU -- recomputed here, so the constant cannot drift from its provenance."""
    worst, at = 0.0, None
    for case in R.CONV0_CASES:
        c = R.conv0_inputs(case)
        ref, scale = R.conv0_case_ref(c)
        v = R.conv0_f32(c["wav"], c["lens"], c["normalize"], c["w"], c["bias"], c["gamma"], c["beta"], c["mode"]).double()
        m = R.conv0_valid(c)
        assert bool((v[~m] == 0).all()) and bool((scale[m] > 0).all())
        ratio = float(((v - ref).abs() / scale)[m].max())
        if ratio > worst:
            worst, at = ratio, R.conv0_id(case)
    print(f"conv0 restatement: max err / scale {worst:.4e} at {at}")
    assert abs(worst - R.CONV0_LAMBDA_MEASURED) <= 1e-3 * R.CONV0_LAMBDA_MEASURED, (worst, at)
    assert R.CONV0_LAMBDA == 4 * R.CONV0_LAMBDA_MEASURED


def test_wav_stats_and_clip_frames_references():
    wav, lens = R.wav_stats_case(1025)
    st, bd = R.wav_stats_ref(wav, lens)
    for b, n in enumerate(lens):
        v = wav[b, :n].double()
        assert abs(float(st[b, 0] - v.sum())) <= float(bd[b, 0]) and abs(float(st[b, 1] - (v * v).sum())) <= float(bd[b, 1])
    assert st[2].tolist() == [0.0, 0.0] and bd[2].tolist() == [0.0, 0.0]
    # clip_frames: the oracle's frame count at every level, zero below a kernel, min_len, the clamp to [0, L]
    arch = SimpleNamespace(conv_kernel=R.WAVLM_STACK[0], conv_stride=R.WAVLM_STACK[1])
    out = R.clip_frames_ref([32000, 400, 399, 9, -3, 40000], 32000, *R.WAVLM_STACK, 0)
    assert out[-1][0] == O.wavlm_num_frames(32000, arch) == 99 and out[-1][1] == O.wavlm_num_frames(400, arch) == 1
    assert out[-1][2] == 0 and [lv[3] for lv in out] == [0] * 7 and [lv[4] for lv in out] == [0] * 7 and out[-1][5] == 99
    assert R.clip_frames_ref([200, 201, 32000, 32005], 32000, (0,), (160,), 201) == [[0, 2, 201, 201]]


# ------------------------------------------------------------------------------------------------- log-mel controls
def _lm(n_mels, mp, shape, fill=float("nan"), **wrong):
    n = 2 * mp * 160
    wav, L, lens, kinds = R.logmel_case(n, shape, fill)
    return R.logmel_ref(wav[:, :L], lens, n_mels, n, **wrong), kinds


def _clips(kinds, names):
    return [b for b, k in enumerate(kinds) if k in names]


@pytest.mark.parametrize("n_mels,mp", R.LOGMEL_MODELS)
def test_control_logmel(n_mels, mp):
    """Each wrong reading of the log-mel definition, on the GPU test's own batches, counted over the elements it can reach:
      symmetric padding                    the first two and last two frames of the clips with energy at their edges (noise, DC + noise, impulses)
      symmetric Hann, the fold's missing 1/2 at sample 200, frames shifted by one, the bank shifted by one bin, the HTK bank
                                           every element of the noise and DC + noise clips (a silent frame of the impulse clip sits at the
                                           floor under any of them; on a pure tone only 2-6 % of the elements move)
      one maximum for the whole batch      the silent clip: its floor comes from another clip's maximum
      reflection about L - 1               the last frame of every clip of the "longer" batch -- the only one whose window passes n_samples
      lens ignored                         the clips of the ragged batch shorter than n_samples."""
    r, kinds = _lm(n_mels, mp, "exact")
    ref, bound = r["out"], R.logmel_bound(r)
    nf = ref.shape[2]

    def share(wrong, clips, frames=None):
        f = torch.arange(nf) if frames is None else torch.tensor(frames)
        ix = (torch.tensor(clips)[:, None, None], torch.arange(n_mels)[None, :, None], f[None, None, :])
        return R.frac_outside(wrong[ix], ref[ix], bound[ix])

    edgy, broad = _clips(kinds, R.LOGMEL_BROADBAND), _clips(kinds, ["noise", "dc_noise"])
    shares = {
        "symmetric padding": share(_lm(n_mels, mp, "exact", pad="symmetric")[0]["out"], edgy, [0, 1, nf - 2, nf - 1]),
        "symmetric Hann": share(_lm(n_mels, mp, "exact", window=R.hann400(periodic=False))[0]["out"], broad),
        "fold without 1/2": share(_lm(n_mels, mp, "exact", fold200=2.0)[0]["out"], broad),
        "frames shifted": share(_lm(n_mels, mp, "exact", frame_shift=1)[0]["out"], broad),
        "bank shifted": share(_lm(n_mels, mp, "exact", bank=torch.roll(R.mel_bank(n_mels), 1, dims=0))[0]["out"], broad),
        "HTK bank": share(_lm(n_mels, mp, "exact", bank=R.mel_bank(n_mels, htk=True))[0]["out"], broad),
        "batch-wide maximum": share(_lm(n_mels, mp, "exact", batch_max=True)[0]["out"], _clips(kinds, ["silence"])),
    }
    # L > n_samples: the tail of 50.0 must be cut before the reflection
    r2, kinds2 = _lm(n_mels, mp, "longer")
    assert torch.equal(r2["out"], ref)
    wrong = _lm(n_mels, mp, "longer", reflect_about_L=True)[0]["out"]
    shares["reflection about L - 1"] = share(wrong, list(range(len(kinds2))), [nf - 1])
    # lens: the ragged batch against the same clips read to their end
    r3, kinds3 = _lm(n_mels, mp, "ragged")
    wav, L, lens, _ = R.logmel_case(2 * mp * 160, "ragged", fill=None)
    wrong = R.logmel_ref(wav, None, n_mels, 2 * mp * 160)["out"]
    b3 = R.logmel_bound(r3)
    short = [b for b, k in enumerate(lens) if k < 2 * mp * 160]
    shares["lens ignored"] = R.frac_outside(wrong[short], r3["out"][short], b3[short])
    for what, s in shares.items():
        assert _report(f"log-mel {n_mels} x {nf}, {what}", s) >= MIN_SHARE, what
    # the informative share the GPU test relies on: at most 1 % of a broadband clip's elements have a bound wider than 1e-2
    for b in edgy:
        assert float((bound[b] > R.LOGMEL_UNINFORMATIVE).double().mean()) <= 0.01


# ------------------------------------------------------------------------------------------------- conv0 controls
def _conv0_share(c, wrong, ref, scale, m):
    return R.frac_outside_nan(wrong[m], ref[m], R.conv0_bound(ref, scale, c["pair"])[m])


@pytest.mark.parametrize("case", R.CONV0_CASES, ids=R.conv0_id)
def test_control_conv0(case):
    """Each wrong reading of level 0, on the GPU case's own inputs (finite junk instead of NaN behind the lengths), counted over what it can reach:
      taps reversed                              every valid element; not the group cases of one frame, where y = mu and the output is
                                                 gelu(beta) under any taps
      unbiased GroupNorm variance                group cases with T0 <= 3 (at one frame it is 0 / 0: no finite output matches)
      GroupNorm eps 1e-7                         the low-variance channel of the group cases with T0 >= 511, clips with a signal
      statistics over the batch-wide T0          the shorter clip of the ragged group cases
      waveform mean over L, not lens[b]          the shorter clip of the ragged layer cases with normalisation (GroupNorm is blind to a
                                                 per-clip scale and offset of the waveform, so group mode cannot see it)
      LayerNorm divisor 512                      layer cases with C < 512
      tanh GELU                                  cases that store a hi + lo pair; bf16 alone (2^-8) is coarser than the two GELUs' distance
                                                 (4.7e-4 at most), so the hi-only cases cannot see it.  Nor can a group case of one
                                                 frame: its argument is beta ~ 0.1, where the two GELUs differ by 1e-6, and its bound
                                                 carries the cancellation of y sc against mu sc (lambda |mu| r ~ 2e-4)."""
    mode, C, T0, _, ragged, ws, _, pair = case
    c = R.conv0_inputs(case, fill=0.37)
    ref, scale = R.conv0_case_ref(c)
    m = R.conv0_valid(c)
    assert torch.equal(ref, R.conv0_case_ref(R.conv0_inputs(case))[0])                  # nothing behind a length is read
    shares = {}
    if not (mode == "group" and T0 == 1):
        shares["taps reversed"] = _conv0_share(c, R.conv0_case_ref(c, reverse_taps=True)[0], ref, scale, m)
    if mode == "group" and T0 <= 3:
        shares["unbiased variance"] = _conv0_share(c, R.conv0_case_ref(c, unbiased=True)[0], ref, scale, m)
    if mode == "group" and T0 >= 511:
        mm = torch.zeros_like(ref, dtype=torch.bool)
        mm[:2, :, R.CONV0_LOWVAR] = True                                               # (clip 2 is silence: y = mu under any eps)
        shares["GroupNorm eps 1e-7"] = _conv0_share(c, R.conv0_case_ref(c, gn_eps=1e-7)[0], ref, scale, mm & m[..., None])
    one = torch.zeros_like(m)
    one[1] = True
    if mode == "group" and ragged:
        shares["batch-wide T0"] = _conv0_share(c, R.conv0_case_ref(c, stats_T=T0)[0], ref, scale, m & one)
    if mode == "layer" and ragged and ws:
        shares["waveform mean over L"] = _conv0_share(c, R.conv0_case_ref(c, mean_over_L=True)[0], ref, scale, m & one)
    if mode == "layer" and C < 512:
        shares["LayerNorm divisor 512"] = _conv0_share(c, R.conv0_case_ref(c, ln_div=512)[0], ref, scale, m)
    if pair and not (mode == "group" and T0 == 1):
        shares["tanh GELU"] = _conv0_share(c, R.conv0_case_ref(c, tanh=True)[0], ref, scale, m)
    for what, s in shares.items():
        assert _report(f"conv0 {R.conv0_id(case)}, {what}", s) >= MIN_SHARE, what


# ------------------------------------------------------------------------------------------------- GEMM-mode references
def _bf(x):
    return x.to(torch.bfloat16).double()


def test_e4m3_decode_is_torch_float8_e4m3fn():
    b = torch.arange(256, dtype=torch.uint8)
    mine, theirs = R.e4m3_decode(b), b.view(torch.float8_e4m3fn).double()
    assert torch.equal(torch.isnan(mine), torch.isnan(theirs)) and int(torch.isnan(mine).sum()) == 2
    ok = ~torch.isnan(mine)
    assert torch.equal(mine[ok], theirs[ok]) and float(mine[ok].max()) == 448.0
    assert torch.equal(torch.signbit(mine[ok]), torch.signbit(theirs[ok]))


def test_gemm_reference_and_its_scales():
    g = torch.Generator().manual_seed(1)
    a, w, bias = _bf(torch.randn(37, 64, generator=g)), _bf(torch.randn(24, 64, generator=g)), torch.randn(24, generator=g).double()
    rs, cs = torch.rand(37, generator=g).double() + 0.5, -(torch.rand(24, generator=g).double() + 0.5)
    v, mag = R.gemm_ref(a, w, bias, rs, cs)
    want = F.linear(a * rs[:, None], w * cs[:, None], bias)
    assert torch.allclose(v, want, rtol=1e-12, atol=1e-12)
    assert bool((mag >= v.abs() - 1e-12).all()) and bool((mag > 0).all())
    assert torch.allclose(mag, F.linear((a * rs[:, None]).abs(), (w * cs[:, None]).abs(), bias.abs()), rtol=1e-12)
    # the bytes' product "of the very bytes given": e4m3 weights x per-channel scale
    wb = torch.randint(0, 256, (24, 64), generator=g, dtype=torch.uint8)
    wb[(wb & 0x7F) == 0x7F] = 0x3C
    v8, _ = R.gemm_ref(a, R.e4m3_decode(wb), None, None, cs)
    assert torch.allclose(v8, a @ (wb.view(torch.float8_e4m3fn).double() * cs[:, None]).T, rtol=1e-12, atol=1e-12)


def test_residual_pair_reference():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(9, 16, generator=g) * 3
    hi, lo = R.split(x)
    v, mag = torch.randn(9, 16, generator=g).double(), torch.rand(9, 16, generator=g).double() + 1
    out, m = R.residual_pair_ref(v, mag, hi.double(), lo.double(), alpha=0.5)
    assert torch.allclose(out, hi.double() + lo.double() + 0.5 * v, rtol=0, atol=1e-15)
    assert float((hi.double() + lo.double() - x.double()).abs().max()) <= 2.0 ** -16 * float(x.abs().max())
    assert torch.allclose(m, hi.double().abs() + lo.double().abs() + 0.5 * mag)
    out1, _ = R.residual_pair_ref(v, mag, hi.double(), None, alpha=1.0)
    assert torch.equal(out1, hi.double() + v)


@pytest.mark.parametrize("nsl", [1, 2, 3, 4])
def test_statistics_slots_are_the_256_column_sums(nsl):
    g = torch.Generator().manual_seed(3 + nsl)
    x = _bf(torch.randn(11, 256 * nsl, generator=g) + 0.3)
    st, sc = R.tile_stats_ref(x)
    assert torch.allclose(st[..., 0], x.view(11, nsl, 256).sum(-1), rtol=1e-13, atol=1e-13)
    assert torch.allclose(st[..., 1], (x * x).view(11, nsl, 256).sum(-1), rtol=1e-13)
    assert torch.allclose(sc[..., 0], x.abs().view(11, nsl, 256).sum(-1), rtol=1e-13)
    slots = R.row_stats_slots(x, nsl)
    assert slots.dtype == torch.float32 and slots.shape == (11, 4, 2)
    assert torch.equal(slots[:, :nsl], st.float()) and bool(torch.isnan(slots[:, nsl:]).all())
    # a column moved across a tile border changes two slots and leaves their sum alone: the slot order is visible, the row total is not
    y = x.clone()
    if nsl > 1:
        y[:, [255, 256]] = x[:, [256, 255]]
        st2, _ = R.tile_stats_ref(y)
        assert not torch.allclose(st2[:, 0], st[:, 0]) and torch.allclose(st2.sum(1), st.sum(1), rtol=1e-12)


@pytest.mark.parametrize("K,kind", [(256, "normal"), (512, "normal"), (768, "offset"), (1024, "outlier")])
def test_layernorm_fold_reference_is_layer_norm_then_linear(K, kind):
    g = torch.Generator().manual_seed(K)
    x = torch.randn(23, K, generator=g)
    if kind == "offset":
        x = x + 30
    if kind == "outlier":
        x[:, 5] *= 100
    x = _bf(x)
    gamma, beta = torch.randn(K, generator=g).double() * 0.2 + 1, torch.randn(K, generator=g).double() * 0.1
    w, b = torch.randn(40, K, generator=g).double() / K ** 0.5, torch.randn(40, generator=g).double()
    wf, bf_ = w * gamma[None, :], b + w @ beta                       # the fold: W' = gamma o W, bias = b + W beta
    stats, _ = R.tile_stats_ref(x)
    v, mag, cancel = R.ln_fold_ref(x, wf, bf_, stats, K // 256, eps=1e-5)
    want = F.layer_norm(x, (K,), gamma, beta, 1e-5) @ w.T + b
    assert torch.allclose(v, want, rtol=1e-9, atol=1e-9), float((v - want).abs().max())
    assert bool((mag + bf_.abs() >= v.abs() - 1e-9).all()) and bool((cancel >= 0).all())
    ratio = (x * x).mean(1) / x.var(1, unbiased=False)
    assert torch.allclose(cancel, ratio[:, None] * (v - bf_).abs(), rtol=1e-6)
    # controls: statistics of another row, an unfolded bias, a slot forgotten -- all far outside the bound.  (Not the first two on the
    # common-offset rows: there the bound itself is wide, |mean| sum |w'| K 2^-24 ~ 0.04, and rows differ by less.)
    tol = R.tol_ln_fold(v, mag, cancel, K)
    if kind != "offset":
        shifted, _, _ = R.ln_fold_ref(x, wf, bf_, stats.roll(1, 0), K // 256)
        assert float(((shifted - v).abs() > 2 * tol).double().mean()) > 0.5
        nobeta, _, _ = R.ln_fold_ref(x, wf, b, stats, K // 256)
        assert float(((nobeta - v).abs() > 2 * tol).double().mean()) > 0.5
    one_slot_short, _, _ = R.ln_fold_ref(x, wf, bf_, stats, max(K // 256 - 1, 1))
    if K > 256:
        assert float(((one_slot_short - v).abs() > 2 * tol).double().mean()) > 0.5


def test_table_clip_bias_and_ragged_references():
    g = torch.Generator().manual_seed(9)
    B, T, N = 3, 7, 16
    v0, mag0 = torch.randn(B * T, N, generator=g).double(), torch.rand(B * T, N, generator=g).double() + 1
    table = torch.randn(4, N + 8, generator=g).double()               # clip_ld > N
    idx = [2, 0, 2]
    pos = torch.randn(T + 5, N, generator=g).double()
    v, mag = R.gemm_table_terms(v0, mag0, B, T, table, idx, "gelu", pos)
    for b in range(B):
        for t in range(T):
            want = F.gelu(v0[b * T + t] + table[idx[b], :N]) + pos[t]
            assert torch.allclose(v[b * T + t], want, rtol=1e-13, atol=1e-13)
    assert torch.allclose(mag, (mag0.view(B, T, N) + table[idx][:, None, :N].abs() + pos[None, :T].abs()).reshape(B * T, N))
    # a table read one row off is a different result on every frame
    off, _ = R.gemm_table_terms(v0, mag0, B, T, None, None, None, pos[1:])
    plain, _ = R.gemm_table_terms(v0, mag0, B, T, None, None, None, pos)
    assert float(((off - plain).abs() > 1e-3).double().mean()) > 0.95
    m = R.ragged_mask(4, 10, [0, 1, 10, 6])
    assert m.sum(1).tolist() == [0, 1, 10, 6] and bool(m[3, :6].all()) and not bool(m[3, 6:].any())
    assert bool(R.ragged_mask(2, 5).all())


def test_gemm_tolerances_are_the_formats():
    ref, mag = torch.tensor([1.0, -3.0]).double(), torch.tensor([2.0, 8.0]).double()
    assert torch.equal(R.tol_bf16(ref, mag, 512), 2.0 ** -8 * ref.abs() + 512 * 2.0 ** -24 * mag)
    assert torch.equal(R.tol_bf16(ref, mag, 512, R.GELU_LIPSCHITZ), 2.0 ** -8 * ref.abs() + 1.2 * 512 * 2.0 ** -24 * mag)
    assert torch.equal(R.tol_pair(ref, mag, 256), 2.0 ** -15 * ref.abs() + 256 * 2.0 ** -24 * mag)
    x = torch.linspace(-6, 6, 20001, dtype=torch.float64, requires_grad=True)
    (d,) = torch.autograd.grad(F.gelu(x).sum(), x)
    assert 1.12 < float(d.abs().max()) < R.GELU_LIPSCHITZ
