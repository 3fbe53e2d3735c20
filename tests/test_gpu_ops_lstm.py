"""-m gpu: the BiLSTM recurrence (csrc/lstm.hip) at the operator level, through wfl_op_lstm, against the float64 recurrence of
tests/lstm_ref.py (checked on the CPU by tests/test_lstm_ref_cpu.py, which also shows that the bounds used here reject a recurrence
with one wrong gate, a wrong backward start, a stale h or a cleared cell state).

Every template instantiation of launch_lstm_t is run: eight hidden sizes x equal-length / ragged x the bf16 form / the three-pass split
form (above H = 256 the four-wave form without a loader wave), then the step counts around the gx prefetch depth (6) and the ring (8),
clips of length 1 and 0, every slice width, a batch cut into two launches, T = 600 of plain, saturated and long-memory inputs, reuse of
the exchange buffer over stale tags, and padded leading dimensions.

Conventions of every launch (`_run`)
  * inputs from lstm_ref.make_case: W_hh ~ U(-H^-1/2, H^-1/2), gx ~ N(0, 1), fp32, fixed seeds; W_hh packed by the library's own
    wfl_op_lstm_pack_whh; frame rows with lead = 8 and P = T + 8; gx rows no clip owns are NaN;
  * out (and out_lo) are filled with a bf16 sentinel first, and everything outside rows t < clip_T[b] x columns < 2H must still hold it:
    the lead, the gaps between clips, the tail, the rows behind a clip's own length, the columns beyond 2H when ldo > 2H;
  * the status word must read 0 (a hand-off wait that gives up sets bit 0);
  * bounds per case from the reference alone (lstm_ref.Case):  bf16 form  max |out - ref| <= 2^-9 + 2 E_q, mean <= 2 M_q;
    split form  max |out + out_lo - ref| <= 4 E_p.  The measured figures go to `_note` (parity_stats.jsonl) and are summarised in
    profiles/lstm_op_tests.txt."""
import pytest
import torch

import gpu_util as G
import lstm_ref as L
from test_gpu_model import _note

pytestmark = pytest.mark.gpu

SENT = 77.0                       # exact in bf16
LEAD, GAP, TAIL = 8, 8, 8
FORMS = ("bf16", "split")


def _rows(B, T, valid):
    """-> (P, R, [n] buffer rows of the frames that exist, in the order of valid.nonzero())"""
    P = T + GAP
    b, t = valid.nonzero(as_tuple=True)
    return P, LEAD + B * P + TAIL, LEAD + b * P + t


def _run(case, form, U=0, ldgx=None, ldo=None, exchange=None):
    """One wfl_op_lstm launch of a lstm_ref.Case -> h [B, T, 2H] float64 on the CPU (hi, lo or None), zero where no frame exists.
    Asserts the sentinels and the status word."""
    H, B, T = case.H, case.B, case.T
    split = form == "split"
    ldgx, ldo = ldgx or 8 * H, ldo or 2 * H
    P, R, rows = _rows(B, T, case.valid)
    gx = torch.full((R, ldgx), float("nan"))
    gx[LEAD:LEAD + B * P].view(B, P, ldgx)[:, :T, :8 * H] = L.kernel_columns(case.gx)
    gx = gx.cuda()
    whh, whh_lo = G.lstm_pack_whh(case.whh, H, U, lo=split)
    out = torch.full((R, ldo), SENT, dtype=torch.bfloat16, device="cuda")
    out_lo = torch.full_like(out, SENT) if split else None
    clip_T = None if case.clip_T is None else torch.tensor(case.clip_T, dtype=torch.int32, device="cuda")
    if exchange is None:
        exchange = torch.zeros(G.lstm_exchange_bytes(H, B), dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    G.lstm(gx, ldgx, whh, out, ldo, LEAD, B, T, P, H, exchange, status, U=U, whh_lo=whh_lo, out_lo=out_lo, clip_T=clip_T)
    torch.cuda.synchronize()
    assert int(status.item()) == 0, f"status {int(status.item())}: a hand-off wait timed out"
    res = []
    for o in (out, out_lo):
        if o is None:
            res.append(None)
            continue
        o = o.cpu()
        keep = torch.ones(R, ldo, dtype=torch.bool)
        keep[rows, :2 * H] = False
        assert bool((o[keep] == SENT).all()), "a row or column outside the clips' own frames was written"
        h = torch.zeros(B, T, 2 * H, dtype=torch.float64)
        h[case.valid] = o[rows, :2 * H].double()
        res.append(h)
    return res


def _check(case, form, tag, **kw):
    """launch, hold the result to the case's bound, note the figures -> (hi, lo)"""
    hi, lo = _run(case, form, **kw)
    if not bool(case.valid.any()):
        return hi, lo
    if form == "bf16":
        ok, mx, mean = case.bf16_form_ok(hi)
        bmax, bmean = case.bf16_bounds()
        E_q, M_q = case.EM_q
        _note(f"lstm_op_{tag}_bf16", max_err=mx, mean_err=mean, E_q=E_q, M_q=M_q, bound_max=bmax, bound_mean=bmean)
        print(f"{tag} bf16: max {mx:.3e} (E_q {E_q:.3e}, bound {bmax:.3e})  mean {mean:.3e} (M_q {M_q:.3e}, bound {bmean:.3e})")
        assert ok, (tag, mx, bmax, mean, bmean)
    else:
        ok, mx = case.split_form_ok(hi + lo)
        _note(f"lstm_op_{tag}_split", max_err=mx, E_p=case.E_p, bound_max=case.split_bound())
        print(f"{tag} split: max {mx:.3e} (E_p {case.E_p:.3e}, bound {case.split_bound():.3e})")
        assert ok, (tag, mx, case.split_bound())
        assert bool((lo.abs() <= 2.0 ** -8 * hi.abs()).all()), "out_lo is not the remainder of out"
    return hi, lo


def _alone_equals_batch(case, form, clip, got, **kw):
    """clip `clip` launched alone (same T and clip_T) equals its rows of the batch bit for bit, hi and lo"""
    alone = _run(case.sub([clip]), form, **kw)
    for a, b in zip(alone, got):
        if a is not None:
            n = int(case.valid[clip].sum())
            assert torch.equal(a[0, :n], b[clip, :n]), (form, clip)


# ------------------------------------------------------------------------------------------------------------------------------------
# every instantiation: H x {equal, ragged} x {bf16, split}.  B = 17: two clip groups, the second holding one clip, so 15 of its 16 lanes
# run on the clamped clip; clip 16 alone must equal its rows of the batch (the header's promise)
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ragged", [False, True], ids=["equal", "ragged"])
@pytest.mark.parametrize("H", L.HIDDEN_SIZES)
def test_every_instantiation(H, ragged, form):
    case = L.make_case(H, 17, 40, ragged=ragged)
    if ragged:
        assert max(case.clip_T) == 40 and min(case.clip_T) == 1 and 1 < case.clip_T[16] < 40
    got = _check(case, form, f"all_h{H}_{'ragged' if ragged else 'equal'}")
    _alone_equals_batch(case, form, 16, got)


# ------------------------------------------------------------------------------------------------------------------------------------
# step counts around the gx prefetch depth (LSTM_DL = 6) and the ring (LSTM_NR = 8); T = 1 publishes nothing
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 5, 6, 7, 8, 9, 17])
@pytest.mark.parametrize("H,form", [(64, "bf16"), (64, "split"), (256, "bf16"), (256, "split"), (384, "split")])
def test_step_count_edges(H, form, T):
    _check(L.make_case(H, 3, T), form, f"steps_h{H}_t{T}")


# ------------------------------------------------------------------------------------------------------------------------------------
# clips of length T, 1, 0 and in between: a clip without frames is within the contract (wfl_forward: a clip below the front end's
# minimum), and its rows stay untouched
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("H", [32, 256, 512])
def test_ragged_edges(H, form):
    _check(L.make_case(H, 5, 12, clip_T=(12, 1, 0, 7, 6)), form, f"ragged_edges_h{H}")


# ------------------------------------------------------------------------------------------------------------------------------------
# slice widths: U = 8, 16, 32 at H = 32 (4, 2, 1 workgroups per direction) and H = 256, U = 8 at H = 192 (24 workgroups) -- the narrow
# slices, where waves beyond the slice's pairs compute and store nothing; and a batch cut into launches of two clip groups and one
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ragged", [False, True], ids=["equal", "ragged"])
@pytest.mark.parametrize("H,U", [(32, 8), (32, 16), (32, 32), (256, 8), (256, 16), (256, 32), (192, 8)])
def test_slice_widths(H, U, ragged, form):
    _check(L.make_case(H, 17, 40, ragged=ragged), form, f"width_h{H}_u{U}_{'ragged' if ragged else 'equal'}", U=U)


@pytest.mark.parametrize("form", FORMS)
def test_batch_cut_into_two_launches(form):
    """H = 256, U = 8: 32 slices per direction, so 128 workgroups hold two clip groups; B = 33 is three -- launches of two and one"""
    case = L.make_case(256, 33, 40, ragged=True)
    got = _check(case, form, "cut_h256_u8_b33", U=8)
    _alone_equals_batch(case, form, 32, got, U=8)


# ------------------------------------------------------------------------------------------------------------------------------------
# accumulation over many steps: plain, saturated (gx x 8) and long-memory (+4 on the forget gate) inputs
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", ["plain", "saturated", "long"])
@pytest.mark.parametrize("H", [32, 256])
def test_six_hundred_steps(H, kind, form):
    _check(L.make_case(H, 4, 600, kind=kind), form, f"t600_h{H}_{kind}")


@pytest.mark.parametrize("form", FORMS)
def test_widest_hidden_size_over_64_steps(form):
    _check(L.make_case(640, 4, 64), form, "t64_h640")


# ------------------------------------------------------------------------------------------------------------------------------------
# the exchange buffer is reused: after a longer launch, and over well-formed granules that carry stale tags.  The launcher's clearing
# fill is what keeps them from validating; without it the kernel would consume h = 1.0 and the values would be off (nothing would wait)
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,form", [(64, "bf16"), (256, "bf16"), (256, "split"), (384, "split")])
def test_exchange_reuse(H, form):
    B = 17
    long_case, case = L.make_case(H, B, 40), L.make_case(H, B, 9)
    fresh = _check(case, form, f"reuse_h{H}_t9")
    ex = torch.zeros(G.lstm_exchange_bytes(H, B), dtype=torch.uint8, device="cuda")
    _run(long_case, form, exchange=ex)
    again = _run(case, form, exchange=ex)
    for a, b in zip(again, fresh):
        assert a is None or torch.equal(a, b), "after a T = 40 launch on the same exchange buffer"
    gran = ex.view(torch.int32).view(-1, 2)
    for tag in range(1, 41):
        gran[:, 0] = 0x3F803F80                    # two bf16 1.0
        gran[:, 1] = tag
        again = _run(case, form, exchange=ex)
        for a, b in zip(again, fresh):
            assert a is None or torch.equal(a, b), f"over stale granules with tag {tag}"


# ------------------------------------------------------------------------------------------------------------------------------------
# leading dimensions beyond the data: ldgx = 8H + 4, ldo = 2H + 16 (the columns beyond 2H keep the sentinel: `_run`)
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_padded_leading_dimensions(form):
    H = 128
    case = L.make_case(H, 17, 40, ragged=True)
    got = _check(case, form, "ld_h128", ldgx=8 * H + 4, ldo=2 * H + 16)
    tight = _run(case, form)
    for a, b in zip(got, tight):
        assert a is None or torch.equal(a, b)
