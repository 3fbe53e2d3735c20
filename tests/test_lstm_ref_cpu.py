"""CPU (-m "not gpu"): the float64 BiLSTM recurrence of tests/lstm_ref.py is nn.LSTM, handles per-clip lengths as running each clip
alone does, and the bounds measured from it (lstm_ref.Case) reject a recurrence with one deliberate mistake -- the controls of
tests/test_gpu_ops_lstm.py, which holds csrc/lstm.hip to the same bounds."""
import pytest
import torch

import lstm_ref as L


def _nn_lstm_case(H, B, T, D, seed):
    torch.manual_seed(seed)
    m = torch.nn.LSTM(D, H, batch_first=True, bidirectional=True, dtype=torch.float64)
    x = torch.randn(B, T, D, dtype=torch.float64)
    gx = torch.stack([x @ getattr(m, "weight_ih_l0" + suf).T + getattr(m, "bias_ih_l0" + suf) + getattr(m, "bias_hh_l0" + suf)
                      for suf in ("", "_reverse")], 2)
    whh = torch.stack([m.weight_hh_l0, m.weight_hh_l0_reverse]).detach()
    return m, x, gx.detach(), whh


@pytest.mark.parametrize("H,B,T", [(8, 3, 11), (32, 2, 40)])
def test_exact_reference_is_nn_lstm(H, B, T):
    m, x, gx, whh = _nn_lstm_case(H, B, T, 24, seed=H + T)
    with torch.no_grad():
        want = m(x)[0]
    got = L.lstm_ref(gx, whh)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12


def test_lengths_agree_with_running_each_clip_alone():
    """per-clip lengths (T, 1, 0 and values in between): every clip equals nn.LSTM and the reference on that clip's frames alone --
    its backward direction starts at its own last frame -- and rows beyond its length are zero"""
    H, B, T = 16, 6, 13
    m, x, gx, whh = _nn_lstm_case(H, B, T, 24, seed=5)
    lens = [13, 1, 0, 7, 6, 12]
    got = L.lstm_ref(gx, whh, lens)
    for b, n in enumerate(lens):
        assert float(got[b, n:].abs().max()) == 0.0 if n < T else True
        if n == 0:
            continue
        with torch.no_grad():
            want = m(x[b:b + 1, :n])[0][0]
        assert float((got[b, :n] - want).abs().max()) <= 1e-12, (b, n)
        alone = L.lstm_ref(gx[b:b + 1, :n], whh)[0]
        assert float((alone - got[b, :n]).abs().max()) <= 1e-13, (b, n)     # (the matrix product's summation order follows the batch size)
    # the rounded forms keep clips independent too: at most a rounding that fell the other way
    for fb, tol in (("bf16", 2.0 ** -7), ("pair", 2.0 ** -15), ("pair32", 2.0 ** -15)):
        got = L.lstm_ref(gx, whh, lens, fb)
        assert float((L.lstm_ref(gx[3:4, :7], whh, None, fb)[0] - got[3, :7]).abs().max()) <= tol, fb


def test_feedback_forms_round_as_named():
    c = L.make_case(32, 3, 9)
    w = L.round_weights(c.whh, "bf16")
    q = L.lstm_ref(c.gx, w, None, "bf16")
    assert torch.equal(q, L.round_bf16(q))                                   # what is returned is what was fed back
    p = L.lstm_ref(c.gx, w, None, "pair")
    assert torch.equal(p, L.round_pair(p)) and not torch.equal(p, L.round_bf16(p))
    e = L.lstm_ref(c.gx, w)
    assert 0 < float((p - e).abs().max()) < 2.0 ** -14 < float((q - e).abs().max()) < 2.0 ** -6
    # the pair weights are sixteen bits of W_hh, the bf16 weights eight
    x = c.whh.double()
    assert bool(((L.round_weights(c.whh, "pair") - x).abs() <= 2.0 ** -16 * x.abs()).all())
    assert bool(((w - x).abs() <= 2.0 ** -8 * x.abs()).all()) and float((w - x).abs().max()) > 2.0 ** -12
    # kernel_columns: column dir * 4H + 4 * unit + gate
    k = L.kernel_columns(c.gx)
    assert float(k[1, 2, 1 * 128 + 4 * 5 + 2]) == float(c.gx[1, 2, 1, 2 * 32 + 5])


# The cases the bounds must bite on: the ragged "every instantiation" shape at two hidden sizes, and the three T = 600 kinds.
BITE_CASES = {"ragged_h32": dict(H=32, B=17, T=40, ragged=True), "ragged_h256": dict(H=256, B=17, T=40, ragged=True),
              "plain_t600": dict(H=32, B=4, T=600), "saturated_t600": dict(H=32, B=4, T=600, kind="saturated"),
              "long_t600": dict(H=32, B=4, T=600, kind="long")}


@pytest.mark.parametrize("name", sorted(BITE_CASES))
def test_bounds_pass_the_defined_arithmetic_and_reject_each_mistake(name):
    """A recurrence with one mistake -- forget and input gate exchanged in one unit, the backward direction started at T - 1 instead of
    clip_T - 1, h fed back from step s - 2, the cell state reset at step 8 -- lands outside the bound of both forms of the same case;
    the defined arithmetic itself (bf16 feedback; pair feedback in float32) lands inside."""
    c = L.make_case(**BITE_CASES[name])
    E_q, M_q = c.EM_q
    print(f"{name}: E_q {E_q:.3e}  M_q {M_q:.3e}  E_p {c.E_p:.3e}")
    assert c.bf16_form_ok(c.ref("bf16", "bf16"))[0]
    assert c.split_form_ok(c.ref("pair", "pair32"))[0]
    assert 0 < M_q < 2.0 ** -10 and E_q < 2.0 ** -4 and 0 < c.E_p < 2.0 ** -14    # contractive on these inputs: roundings do not pile up
    for mistake in L.MISTAKES:
        if mistake == "bwd_start" and c.clip_T is None:
            continue                                                 # (every clip ends at T - 1: the mistake changes nothing)
        ok, mx, mean = c.bf16_form_ok(c.ref("bf16", "bf16", mistake))
        print(f"  {mistake}: bf16 form max {mx:.3e} mean {mean:.3e} (bounds {c.bf16_bounds()[0]:.3e}, {c.bf16_bounds()[1]:.3e})")
        assert not ok, (name, mistake, mx, mean, c.bf16_bounds())
        ok, mx = c.split_form_ok(c.ref("pair", "pair32", mistake))
        print(f"  {mistake}: split form max {mx:.3e} (bound {c.split_bound():.3e})")
        assert not ok, (name, mistake, mx, c.split_bound())
