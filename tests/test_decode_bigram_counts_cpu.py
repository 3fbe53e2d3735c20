"""CPU (-m "not gpu"): the host side of the bigram adaptation -- the float64 expected successions of tests/bio_bigram_counts_ref.py
against its brute force and against the gammas of tests/bio_bigram_posterior_ref.py, phonotactics.reestimate, the EM bound over a few
rounds in float64, the ABI entries and the argument errors of `python -m wfl_asr_amd.adapt_bigram` that need no GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import bio_bigram_counts_ref as BC
import bio_bigram_posterior_ref as BP
import bio_bigram_ref as R
from wfl_asr_amd import decode as DC
from wfl_asr_amd import phonotactics as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE3 = (1, [(2, 0)])                   # P = 1, C = 4: O = 1, B = 2, I = 0, class 3 is never chosen
TABLE5 = (1, [(2, 3), (4, -1)])          # P = 2, C = 5: class 0 is never chosen, O = 1, a (B, I) pair, a B alone
TABLE6 = (0, [(1, 2), (3, 4)])           # P = 2, C = 6: class 5 is never chosen, two (B, I) pairs


def _random_table(n, rng, forbid):
    W = -6.0 * rng.random((n + 1, n + 1))
    mask = rng.random(W.shape) < forbid
    mask[:, 0] = False
    W[mask] = -np.inf
    return W


@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("C,table", [(4, TABLE3), (5, TABLE5), (6, TABLE6)])
def test_reference_equals_brute_force(T, C, table):
    P = len(table[1])
    rng = np.random.default_rng(40 + 7 * T + C)
    seen_forced = seen_forbidden = 0
    for trial in range(12):
        z = rng.standard_normal((T, C)) * 2
        W = _random_table(P, rng, 0.3 if trial % 2 else 0.0)
        forced = rng.random(T) < 0.3 if trial % 3 == 0 else None
        logz, counts = BC.expected_counts(z, table, W, forced)
        want_z, want = BC.brute_force(z, table, W, forced)
        assert abs(logz - want_z) <= 1e-10, (trial, logz, want_z)
        assert np.abs(counts - want).max() <= 1e-10, trial
        assert counts[0, 0] == 0.0 and (counts[np.isneginf(W)] == 0.0).all() and (counts >= 0).all()
        c32 = BC.expected_counts(z, table, W, forced, dtype=np.float32)
        assert abs(c32[0] - logz) <= 1e-4 and np.abs(c32[1] - counts).max() <= 1e-4
        if forced is not None:
            seen_forced += int(forced.sum())
        seen_forbidden += int(np.isneginf(W).sum())
    assert seen_forbidden and seen_forced


def test_reference_against_the_posterior_reference():
    """logZ is the posterior reference's; column q >= 1 is sum_t gamma_t(B-q); column O is sum_t gamma_t(O) minus the O-after-O mass."""
    rng = np.random.default_rng(11)
    table = (0, [(1, 2), (3, 4), (5, -1)])
    for T, forbid in ((1, 0.0), (7, 0.3), (60, 0.0), (60, 0.3)):
        z = rng.standard_normal((T, 8)) * 3
        forced = rng.random(T) < 0.2
        W = _random_table(3, rng, forbid)
        ids, _ = R.viterbi(z, table, W, forced)
        logz, counts = BC.expected_counts(z, table, W, forced)
        ref = BP.forward_backward(z, table, W, forced, ids, want_gamma=True)
        gO, gB = ref[3], ref[4]
        assert abs(logz - ref[0]) <= 1e-12 * max(1.0, abs(ref[0]))
        assert np.abs(counts[:, 1:].sum(axis=0) - gB.sum(axis=0)).max() <= 1e-12 * max(1, T)
        # gamma_t(O) = sum over s of the mass that enters O from s at t, s = O included: column O lacks exactly the O-after-O mass
        oo = _o_after_o(z, table, W, forced, logz)
        assert abs(counts[:, 0].sum() - (gO.sum() - oo)) <= 1e-11 * max(1, T), (T, forbid)
        assert counts[0, 0] == 0.0 and (counts[np.isneginf(W)] == 0.0).all()


def _o_after_o(z, table, W, forced, logz):
    """sum_t P(frame t - 1 in O (the virtual frame for t = 0) and frame t in O) = sum_t exp(alpha_{t-1}(O) + e_t(O) + beta_t(O) - logZ),
    from recurrences written out here by the definition."""
    T = len(z)
    tot = 0.0
    aO = _alpha_o(z, table, W, forced)
    bO = _beta_o(z, table, W, forced)
    for t in range(T):
        prev = 0.0 if t == 0 else aO[t - 1]
        tot += np.exp(prev + z[t, table[0]] + bO[t] - logz)
    return tot


def _alpha_o(z, table, W, forced):
    """log alpha_t(O), float64, by the definition (no shared code with the references)."""
    o = table[0]
    B = [b for b, _ in table[1]]
    I = [i for _, i in table[1]]
    P, T = len(B), len(z)
    W = np.array(W, np.float64)
    O, Bs, Is = 0.0, np.full(P, -np.inf), np.full(P, -np.inf)
    out = np.empty(T)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            end = np.concatenate([[O], np.logaddexp(Bs, Is)])
            f = bool(forced is not None and forced[t])
            nO = z[t, o] + np.logaddexp(O, np.logaddexp.reduce(end[1:] + W[1:, 0]) if P else -np.inf)
            nB = np.array([-np.inf if f else z[t, B[q]] + np.logaddexp.reduce(end + W[:, q + 1]) for q in range(P)])
            nI = np.array([-np.inf if f or I[q] < 0 else z[t, I[q]] + end[q + 1] for q in range(P)])
            O, Bs, Is = nO, nB, nI
            out[t] = O
    return out


def _beta_o(z, table, W, forced):
    """log beta_t(O), float64, by the definition."""
    o = table[0]
    B = [b for b, _ in table[1]]
    I = [i for _, i in table[1]]
    P, T = len(B), len(z)
    W = np.array(W, np.float64)
    W[0, 0] = 0.0
    bO, bX = 0.0, np.zeros(P)
    out = np.empty(T)
    with np.errstate(invalid="ignore"):
        for t in range(T - 1, -1, -1):
            out[t] = bO
            if t == 0:
                break
            f = bool(forced is not None and forced[t])
            u = np.concatenate([[z[t, o] + bO], [-np.inf if f else z[t, B[q]] + bX[q] for q in range(P)]])
            cont = np.array([-np.inf if f or I[q] < 0 else z[t, I[q]] + bX[q] for q in range(P)])
            nO = np.logaddexp.reduce(W[0] + u)
            nX = np.array([np.logaddexp(np.logaddexp.reduce(W[p + 1] + u), cont[p]) for p in range(P)])
            bO, bX = nO, nX
    return out


# --------------------------------------------------------------------------------------------------------------- reestimate
SYMS = ["O", "a", "b", "c"]


def _prior():
    with np.errstate(divide="ignore"):
        lp = np.log(np.array([[0.0, 0.5, 0.25, 0.25], [0.4, 0.0, 0.6, 0.0], [0.2, 0.3, 0.1, 0.4], [1.0, 0.0, 0.0, 0.0]]))
    return PH.Bigram(SYMS, lp)


def test_reestimate_rows_normalise_and_forbidden_stays_forbidden():
    rng = np.random.default_rng(0)
    counts = rng.random((4, 4)) * 10
    bg = PH.reestimate(counts, SYMS, smoothing=0.5)
    p = np.exp(bg.log_prob)
    assert p[0, 0] == 0.0 and np.isneginf(bg.log_prob[0, 0])
    assert np.abs(p.sum(axis=1) - 1).max() <= 1e-12
    want = counts + 0.5
    want[0, 0] = 0
    assert np.abs(p - want / want.sum(axis=1, keepdims=True)).max() <= 1e-12
    prior = _prior()
    bg = PH.reestimate(counts, SYMS, prior, prior_count=2.0, smoothing=0.5)
    p = np.exp(bg.log_prob)
    shut = np.isneginf(prior.log_prob)
    assert (p[shut] == 0).all() and (p[~shut] > 0).all(), "smoothing resurrected a forbidden succession, or closed an allowed one"
    assert np.abs(p.sum(axis=1) - 1).max() <= 1e-12
    want = np.where(shut, 0.0, counts + 2.0 * np.exp(prior.log_prob) + 0.5)
    assert np.abs(p - want / want.sum(axis=1, keepdims=True)).max() <= 1e-12


def test_reestimate_zero_row_and_infinite_prior_count():
    prior = _prior()
    counts = np.array([[0, 3, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1], [2, 0, 0, 0]], np.float64)
    bg = PH.reestimate(counts, SYMS, prior)
    assert np.abs(np.exp(bg.log_prob[1]) - np.exp(prior.log_prob[1])).max() <= 1e-15, "a zero row keeps the prior's row"
    # without a prior: uniform over the allowed successions
    c2 = counts.copy()
    c2[:, 0] += 1.0                                     # (a way into O from every phoneme)
    c2[1] = 0.0
    bg = PH.reestimate(c2, SYMS)
    assert np.abs(np.exp(bg.log_prob[1]) - 0.25).max() <= 1e-15
    assert np.abs(np.exp(PH.reestimate(np.zeros((4, 4)), SYMS).log_prob[0]) - np.array([0, 1, 1, 1]) / 3).max() <= 1e-15
    # prior_count -> infinity returns the prior
    bg = PH.reestimate(counts, SYMS, prior, prior_count=1e15)
    assert np.abs(np.exp(bg.log_prob) - np.exp(prior.log_prob)).max() <= 1e-12
    assert (np.isneginf(bg.log_prob) == np.isneginf(prior.log_prob)).all()


def test_reestimate_refuses_a_table_without_a_way_into_O():
    counts = np.array([[0, 3, 1, 1], [1, 0, 2, 0], [0, 1, 1, 1], [2, 0, 0, 0]], np.float64)
    with pytest.raises(ValueError, match=r"'O'.*\bb\b"):
        PH.reestimate(counts, SYMS)
    assert np.isfinite(PH.reestimate(counts, SYMS, smoothing=0.1).log_prob[1:, 0]).all()
    assert np.isfinite(PH.reestimate(counts, SYMS, _prior(), prior_count=1.0).log_prob[1:, 0]).all()
    for bad, word in ((dict(counts=counts[:3]), "table"), (dict(counts=-counts), ">= 0"), (dict(symbols=["a", "O", "b", "c"]), "begin with"),
                      (dict(smoothing=-1.0), ">= 0"), (dict(prior=PH.Bigram(["O", "a", "c", "b"], _prior().log_prob)), "same symbols")):
        kw = dict(counts=counts, symbols=SYMS, smoothing=0.1)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            PH.reestimate(**kw)


def test_reestimate_round_trip_through_the_file_and_the_table(tmp_path):
    labels = ["O", "B-a", "I-a", "B-b", "I-b", "B-c"]
    ct = DC.class_table(labels)
    from wfl_asr_amd import adapt_bigram as AB
    assert AB.symbols_of(labels) == SYMS
    rng = np.random.default_rng(3)
    bg = PH.reestimate(rng.random((4, 4)) * 5, SYMS, _prior(), prior_count=1.0, smoothing=0.2)
    PH.save(bg, tmp_path / "bg.json")
    back = PH.load(tmp_path / "bg.json")
    assert back.symbols == SYMS and np.array_equal(np.isneginf(back.log_prob), np.isneginf(bg.log_prob))
    fin = np.isfinite(bg.log_prob)
    assert np.abs(back.log_prob[fin] - bg.log_prob[fin]).max() <= 1e-15
    W = PH.transition_table(back, ct, labels, 0.5, 2.0)
    assert W.dtype == np.float32 and W.shape == (4, 4)
    DC.check_transitions(W, 3)
    want = np.where(fin, 2.0 * np.where(fin, bg.log_prob, 0.0) - 0.5, -np.inf)
    want[0, 0] = -0.5
    assert np.array_equal(np.isneginf(W), np.isneginf(want)) and np.abs(W[np.isfinite(want)] - want[np.isfinite(want)]).max() <= 1e-6


def test_em_rounds_never_lower_the_sum_of_logz():
    """Five float64 EM rounds on eight seeded clips at weight 1, penalty 0, smoothing 0, from the uniform table: the EM bound."""
    from wfl_asr_amd import adapt_bigram as AB
    P, C = 4, 10
    table = (0, [(1, 2), (3, 4), (5, 6), (7, -1)])           # classes 8 and 9 are never chosen
    labels = ["O", "B-a", "I-a", "B-b", "I-b", "B-c", "I-c", "B-d", "x", "y"]
    ct = DC.class_table(labels)
    assert ct.o_id == table[0] and [tuple(p) for p in ct.pairs.tolist()] == table[1]
    syms = AB.symbols_of(labels)
    rng = np.random.default_rng(5)
    clips = [rng.standard_normal((int(rng.integers(20, 60)), C)) * 2 for _ in range(4)]
    clips += [R.plant(int(rng.integers(30, 60)), C, table, rng, margin=2.0, scale=1.5)[0].astype(np.float64) for _ in range(4)]
    bg = AB.uniform_bigram(syms)
    assert np.abs(np.exp(bg.log_prob).sum(axis=1) - 1).max() <= 1e-12 and np.isneginf(bg.log_prob[0, 0])
    totals = []
    for k in range(6):
        W = PH.transition_table(bg, ct, labels, 0.0, 1.0).astype(np.float64)
        W = np.where(np.isneginf(W), -np.inf, np.where(np.isfinite(bg.log_prob), bg.log_prob, 0.0))      # (no float32 rounding)
        W[0, 0] = 0.0
        tot, counts = 0.0, np.zeros((P + 1, P + 1))
        for z in clips:
            lz, c = BC.expected_counts(z, table, W, None)
            tot += lz
            counts += c
        totals.append(tot)
        bg = PH.reestimate(counts, syms)
    print("sum logZ per round:", " ".join(f"{t:.6f}" for t in totals))
    assert len(totals) == 6 and all(b >= a - 1e-9 for a, b in zip(totals, totals[1:])), totals
    assert totals[-1] > totals[0] + 1e-3, "the rounds did not move the table (test setup)"


# ------------------------------------------------------------------------------------------------------- ABI and Python entry
def test_abi_entries():
    from wfl_asr_amd import _lib
    src = open(os.path.join(ROOT, "include", "wfl_asr.h")).read()
    for name in ("wfl_decode_bigram_counts_workspace_bytes", "wfl_decode_bigram_counts"):
        assert re.search(rf"\b{name}\s*\(", src) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["wfl_decode_bigram_counts"][1]) == 17
    assert int(re.search(r"#define\s+WFL_ABI_VERSION\s+(\d+)", src).group(1)) == 2
    import __graft_entry__ as g
    g.build()
    lib = _lib.load()
    assert lib.wfl_decode_bigram_counts is not None
    T = np.array([10, 0, 7], np.int32)
    # per clip with T > 0: round_up_64(T (N + 1)) + 2 round_up_64(T) words
    assert DC.bigram_counts_workspace_bytes(T, 0) == 4 * 2 * (64 + 2 * 64)
    assert DC.bigram_counts_workspace_bytes(T, 70) == 4 * ((768 + 128) + (512 + 128))
    assert DC.bigram_counts_workspace_bytes(np.array([15000], np.int32), 191) == 4 * (15000 * 193 + 40 + 2 * 15040)
    assert DC.bigram_counts_workspace_bytes(T, 192) == 0                # over the cap: nothing is counted


def test_the_entry_validates_its_arguments_without_gpu():
    import ctypes
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import _lib
    lib = _lib.load()
    V = ctypes.c_void_p
    buf = (ctypes.c_char * 64)()
    d = ctypes.cast(buf, V)                        # never dereferenced: every call below fails on the host
    fo = np.zeros(1, np.int64)
    T = np.array([10], np.int32)
    h = lambda a: a.ctypes.data_as(V)              # noqa: E731

    def call(C=141, o_id=0, ldl=141, fo_=fo, T_=T, ws=None, ws_bytes=0, logits=d, n=1, pairs=d, n_pairs=70, trans=d, thr=0.0,
             logz=d, counts=d, status=d):
        return lib.wfl_decode_bigram_counts(logits, ldl, C, o_id, h(fo_) if fo_ is not None else None, h(T_), n, pairs, n_pairs, trans,
                                            thr, ws, ws_bytes, logz, counts, status, None)

    need = lib.wfl_decode_bigram_counts_workspace_bytes(h(T), 1, 70)
    assert need == 4 * (768 + 2 * 64)
    for kw, word in ((dict(C=0), b"C < 1"), (dict(o_id=141), b"o_id"), (dict(ldl=100), b"ldl"), (dict(n=-1), b"negative count"),
                     (dict(n_pairs=-1), b"negative count"), (dict(thr=-0.1), b"threshold"),
                     (dict(fo_=None, ws=d, ws_bytes=need), b"null host"),
                     (dict(T_=np.array([-2], np.int32), ws=d, ws_bytes=need), b"negative"),
                     (dict(logits=None, ws=d, ws_bytes=need), b"null device"), (dict(logz=None, ws=d, ws_bytes=need), b"null device"),
                     (dict(counts=None, ws=d, ws_bytes=need), b"null device"), (dict(status=None, ws=d, ws_bytes=need), b"null device"),
                     (dict(pairs=None, ws=d, ws_bytes=need), b"null device"), (dict(trans=None, ws=d, ws_bytes=need), b"null device"),
                     (dict(ws=d, ws_bytes=need - 1), b"workspace"), (dict(ws=None, ws_bytes=need), b"workspace")):
        assert call(**kw) != 0, kw
        err = lib.wfl_last_error()
        assert b"wfl_decode_bigram_counts" in err and word in err, (kw, err)
    assert call(n=0) == 0                          # nothing to do
    assert call(n=0, trans=None, counts=None) == 0
    size = lib.wfl_decode_bigram_counts_workspace_bytes
    assert size(h(T), -1, 70) < 0 and size(h(T), 1, -1) < 0 and size(None, 1, 70) < 0 and size(None, 0, 70) == 0


def test_parameter_lists():
    assert list(inspect.signature(DC.bigram_expected_counts).parameters) == ["logits", "n_frames", "table", "trans", "threshold",
                                                                             "frame_offsets", "stream"]
    assert list(inspect.signature(DC.bigram_counts_workspace_bytes).parameters) == ["n_frames", "n_pairs"]
    assert list(inspect.signature(PH.reestimate).parameters) == ["counts", "symbols", "prior", "prior_count", "smoothing"]
    from wfl_asr_amd.infer import Labeler
    assert list(inspect.signature(Labeler.expected_successions).parameters) == ["self", "audio_paths", "trans", "lang_id",
                                                                                "confidence_threshold", "verbose"]


# ----------------------------------------------------------------------------------------------------------------- the tool
def _model_dir(tmp_path, labels):
    save = tmp_path / "model"
    save.mkdir()
    (save / "phonemes.txt").write_text("\n".join(labels) + "\n")
    cfg = tmp_path / "config.yaml"
    cfg.write_text(f"output:\n  save_dir: {save}\npostprocess:\n  decode: viterbi\n")
    return str(cfg)


def test_the_tool_refuses_bad_requests_before_any_model_is_loaded(tmp_path, capsys):
    from wfl_asr_amd import adapt_bigram as AB
    from wfl_asr_amd import infer

    class NoModel:
        def __init__(self, *a, **k):
            raise AssertionError("a model was asked for")
    saved = infer.Labeler
    infer.Labeler = NoModel
    try:
        labels = ["O", "B-a", "I-a", "B-b"]
        cfg = _model_dir(tmp_path, labels)
        wav = tmp_path / "x.wav"
        wav.write_bytes(b"RIFF")
        out = str(tmp_path / "out.json")
        base = ["-ckpt", "none.pt", "-c", cfg, "-o", out]

        def refused(args, word):
            with pytest.raises(SystemExit) as e:
                AB.main(args)
            assert e.value.code == 2
            assert word in capsys.readouterr().err, word
        # no audio found (an empty folder, a path that does not exist)
        empty = tmp_path / "empty"
        empty.mkdir()
        refused([str(empty), str(tmp_path / "nothing.wav")] + base, "no audio file found")
        # an --init that the label set or the search refuses
        PH.save(PH.Bigram(["O", "a", "z"], np.log(np.full((3, 3), 0.5))), tmp_path / "other.json")
        refused([str(wav)] + base + ["--init", str(tmp_path / "other.json")], "lacks phonemes of the label set")
        lp = np.log(np.full((3, 3), 0.5))
        lp[2, 0] = -np.inf
        PH.save(PH.Bigram(["O", "a", "b"], lp), tmp_path / "shut.json")
        refused([str(wav)] + base + ["--init", str(tmp_path / "shut.json")], "[p][O]")
        refused([str(wav)] + base + ["--iterations", "0"], "--iterations")
        refused([str(wav)] + base + ["--smoothing", "-1"], ">= 0")
        refused([str(wav)] + base + ["--prior-count", "2"], "--prior-count needs --init")
        # a label set above 191 phonemes
        big = tmp_path / "big"
        big.mkdir()
        cfg_big = _model_dir(big, ["O"] + [f"B-p{i}" for i in range(192)])
        refused([str(wav), "-ckpt", "none.pt", "-c", cfg_big, "-o", out], "at most 191")
        # a good request gets as far as the model
        PH.save(PH.Bigram(["O", "a", "b"], np.log(np.full((3, 3), 0.5))), tmp_path / "good.json")
        with pytest.raises(AssertionError, match="a model was asked for"):
            AB.main([str(wav)] + base + ["--init", str(tmp_path / "good.json")])
        assert not os.path.exists(out)
    finally:
        infer.Labeler = saved


def test_start_tables():
    from wfl_asr_amd import adapt_bigram as AB
    labels = ["O", "B-b", "I-b", "B-a"]
    assert AB.symbols_of(labels) == ["O", "b", "a"]
    u = AB.start_bigram(labels)
    assert np.isneginf(u.log_prob[0, 0]) and np.abs(np.exp(u.log_prob) - np.array([[0, .5, .5], [1 / 3] * 3, [1 / 3] * 3])).max() <= 1e-15
    DC.check_transitions(PH.transition_table(u, DC.class_table(labels), labels), 2)
