"""Float64 reference of one BiLSTM layer's recurrence (csrc/lstm.hip, wfl_op_lstm), its inputs and its bounds.

    gates_t = gx_t + W_hh h_(t-1),   c_t = f c_(t-1) + i g,   h_t = o tanh(c_t),   zero initial state,

both directions, gx (the input projection with both biases) given in PyTorch's gate order i | f | g | o.  With per-clip lengths the
backward direction of a clip starts at the clip's own last frame and rows at t >= clip_T[b] stay zero.

`feedback` is what happens to h_t before it is fed back and returned:
    exact    nothing
    bf16     rounded to bf16                         (the default kernel's defined arithmetic)
    pair     rounded to a bf16 pair hi + lo          (the split kernel's, `model.precision: high`)
    pair32   as pair, and the whole step in float32  (what a float32 implementation of the split form can reach)
W_hh is rounded by the caller (`round_weights`): to bf16 for the bf16 form, to hi + lo for the split form.  gx is taken as it is.

`mistake` builds one deliberate error into the recurrence.  The bounds the GPU tests hold the kernel to (`Case`) must reject each of them
(tests/test_lstm_ref_cpu.py): a bound that lets one through is no test of the kernel.

The bounds are measured from this reference alone, per case, never from a kernel:
    E_q = max |ref(bf16) - ref(exact)|,  M_q = the mean of the same,  on the bf16 weights
    E_p = max |ref(pair32) - ref(exact)|                              on the pair weights
    bf16 form:   max |out - ref(exact)| <= 2^-9 + 2 E_q   and   mean |out - ref(exact)| <= 2 M_q
                 (2^-9: half a bf16 ulp of |h| <= 1.  2: the kernel's rounding decisions differ from the reference's at ties and
                  near-ties, and each flip costs one more rounding.)
    split form:  max |out + out_lo - ref(exact)| <= 4 E_p
                 (4: sigmoid and tanh are built from the hardware's v_exp_f32 and v_rcp_f32, about 1 ulp each and three per
                  activation, not from correctly rounded float32 functions.)
Maxima and means run over the frames that exist (t < clip_T[b])."""
import functools

import torch

FEEDBACKS = ("exact", "bf16", "pair", "pair32")
MISTAKES = ("swap_if", "bwd_start", "stale_h", "reset_c")
SWAP_UNIT = 3                 # swap_if: the unit (forward direction) whose input and forget gates are exchanged
RESET_STEP = 8                # reset_c: the step at which the cell state is cleared
HIDDEN_SIZES = (32, 64, 128, 192, 256, 384, 512, 640)


def round_bf16(x):
    return x.float().to(torch.bfloat16).to(x.dtype)


def round_pair(x):
    hi = round_bf16(x)
    return hi + round_bf16(x - hi)


def round_weights(whh, form):
    """fp32 weight_hh -> float64 values of what a kernel form holds: `exact`, `bf16` or `pair` (hi + lo)."""
    w = whh.double()
    return {"exact": lambda: w, "bf16": lambda: round_bf16(w), "pair": lambda: round_pair(w)}[form]()


def lstm_ref(gx, whh, clip_T=None, feedback="exact", mistake=None):
    """gx [B, T, 2, 4H] (direction, PyTorch gate order), whh [2, 4H, H] (already rounded), clip_T a list of B lengths or None.
    -> h [B, T, 2H] float64 (forward | backward), zero at t >= clip_T[b]."""
    assert feedback in FEEDBACKS and (mistake is None or mistake in MISTAKES)
    B, T, _, H4 = gx.shape
    H = H4 // 4
    dt = torch.float32 if feedback == "pair32" else torch.float64
    g, W = gx.to(dt), whh.to(dt)
    Tc = torch.full((B,), T, dtype=torch.long) if clip_T is None else torch.as_tensor(list(clip_T), dtype=torch.long)
    assert Tc.shape == (B,) and int(Tc.min()) >= 0 and int(Tc.max()) <= T
    last = torch.full((B,), T - 1, dtype=torch.long) if mistake == "bwd_start" else Tc - 1      # where the backward direction reads first
    ar = torch.arange(B)
    h = torch.zeros(B, 2, H, dtype=dt)
    c, h_before = torch.zeros_like(h), torch.zeros_like(h)
    out = torch.zeros(B, T, 2, H, dtype=torch.float64)
    for s in range(int(Tc.max())):
        act = s < Tc
        t_rd = (last - s).clamp(0, T - 1)                # the backward direction's gx row
        t_wr = (Tc - 1 - s).clamp(0, T - 1)              # and the row its h belongs to
        x = torch.stack([g[:, s, 0], g[ar, t_rd, 1]], 1)
        pre = x + torch.einsum("bdk,dnk->bdn", h_before if mistake == "stale_h" else h, W)
        i, f, gg, o = pre.view(B, 2, 4, H).unbind(2)
        if mistake == "swap_if":
            i, f = i.clone(), f.clone()
            i[:, 0, SWAP_UNIT], f[:, 0, SWAP_UNIT] = pre[:, 0, H + SWAP_UNIT], pre[:, 0, SWAP_UNIT]
        if mistake == "reset_c" and s == RESET_STEP:
            c = torch.zeros_like(c)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        hn = torch.sigmoid(o) * torch.tanh(c)
        if feedback == "bf16":
            hn = round_bf16(hn)
        elif feedback != "exact":
            hn = round_pair(hn)
        h_before, h = h, hn
        out[ar[act], s, 0] = hn[act, 0].double()
        out[ar[act], t_wr[act], 1] = hn[act, 1].double()
    return out.reshape(B, T, 2 * H)


def kernel_columns(gx):
    """gx [B, T, 2, 4H] in PyTorch's gate order -> [B, T, 8H] in the kernel's: column dir * 4H + 4 * unit + gate."""
    B, T, _, H4 = gx.shape
    return gx.view(B, T, 2, 4, H4 // 4).permute(0, 1, 2, 4, 3).reshape(B, T, 2 * H4).contiguous()


class Case:
    """One set of inputs with the references and bounds both kernel forms are held to (computed on first use, then kept)."""

    def __init__(self, gx, whh, clip_T=None):
        self.gx, self.whh, self.clip_T = gx, whh, None if clip_T is None else list(clip_T)
        self.B, self.T, self.H = gx.shape[0], gx.shape[1], gx.shape[3] // 4
        Tc = torch.full((self.B,), self.T) if clip_T is None else torch.tensor(self.clip_T)
        self.valid = torch.arange(self.T)[None, :] < Tc[:, None]                  # [B, T]: the frames that exist

    def ref(self, weights, feedback="exact", mistake=None):
        return lstm_ref(self.gx, round_weights(self.whh, weights), self.clip_T, feedback, mistake)

    def errors(self, out, ref):
        """-> (max, mean) of |out - ref| over the frames that exist"""
        e = (out.double() - ref).abs()[self.valid]
        return float(e.max()), float(e.mean())

    @functools.cached_property
    def exact_bf16w(self):
        return self.ref("bf16")

    @functools.cached_property
    def exact_pairw(self):
        return self.ref("pair")

    @functools.cached_property
    def EM_q(self):
        return self.errors(self.ref("bf16", "bf16"), self.exact_bf16w)

    @functools.cached_property
    def E_p(self):
        return self.errors(self.ref("pair", "pair32"), self.exact_pairw)[0]

    def sub(self, clips):
        """the same inputs restricted to some clips (the references of a clip do not depend on the batch it is in)"""
        return Case(self.gx[clips].contiguous(), self.whh, None if self.clip_T is None else [self.clip_T[b] for b in clips])

    # ---- the bounds
    def bf16_bounds(self):
        E_q, M_q = self.EM_q
        return 2.0 ** -9 + 2 * E_q, 2 * M_q

    def bf16_form_ok(self, out):
        """out [B, T, 2H] of the bf16 form -> (passes, max err, mean err)"""
        mx, mean = self.errors(out, self.exact_bf16w)
        bmax, bmean = self.bf16_bounds()
        return mx <= bmax and mean <= bmean, mx, mean

    def split_bound(self):
        return 4 * self.E_p

    def split_form_ok(self, out):
        """out [B, T, 2H] = hi + lo of the split form -> (passes, max err)"""
        mx, _ = self.errors(out, self.exact_pairw)
        return mx <= self.split_bound(), mx


def ragged_lengths(B, T, seed):
    """lengths that mix T, 1 and values in between; the last clip -- alone in its group when B = 16 k + 1 -- gets one in between"""
    g = torch.Generator().manual_seed(1000 + seed)
    L = torch.randint(2, T, (B,), generator=g).tolist()
    L[0], L[1 % B] = T, 1
    if B > 3:
        L[B // 2] = T
    return L


@functools.lru_cache(maxsize=None)
def make_case(H, B, T, kind="plain", ragged=False, seed=0, clip_T=None):
    """W_hh ~ U(-H^-1/2, H^-1/2) (nn.LSTM's init), gx ~ N(0, 1), fp32, fixed seeds.
    kind: plain / saturated (gx x 8) / long (+4 on the forget gate's pre-activations: the cell state integrates over hundreds of steps)."""
    g = torch.Generator().manual_seed(7919 * H + 31 * B + T + 104729 * seed)
    whh = (torch.rand(2, 4 * H, H, generator=g) * 2 - 1) * H ** -0.5
    gx = torch.randn(B, T, 2, 4 * H, generator=g)
    if kind == "saturated":
        gx = gx * 8
    elif kind == "long":
        gx[..., H:2 * H] += 4
    else:
        assert kind == "plain"
    if clip_T is None and ragged:
        clip_T = ragged_lengths(B, T, seed)
    return Case(gx, whh, clip_T)
