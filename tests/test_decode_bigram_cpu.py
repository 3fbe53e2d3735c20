"""CPU (-m "not gpu"): the phone-bigram decode's host side -- the float64 reference against its brute force, the bigram estimator,
its JSON file, the transition table, the option validation and the ABI entries."""
import json
import os
import re

import numpy as np
import pytest

import bio_bigram_ref as R
import bio_viterbi_ref as V
from wfl_asr_amd import decode as DC
from wfl_asr_amd import phonotactics as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE5 = (1, [(2, 3), (4, -1)])          # C = 5: class 0 is never chosen, O = 1, a (B, I) pair, a B alone


def _random_table(P, rng, forbid):
    W = -6.0 * rng.random((P + 1, P + 1))
    mask = rng.random(W.shape) < forbid
    mask[:, 0] = False
    W[mask] = -np.inf
    return W


@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_reference_equals_brute_force(T):
    rng = np.random.default_rng(10 + T)
    seen_forced = seen_forbidden = 0
    for trial in range(40):
        z = rng.standard_normal((T, 5)) * 2
        W = _random_table(2, rng, 0.3 if trial % 2 else 0.0)
        forced = rng.random(T) < 0.25 if trial % 3 == 0 else None
        ids, obj = R.viterbi(z, TABLE5, W, forced)
        _, best = R.brute_force(z, TABLE5, W, forced)
        assert np.isfinite(best)
        assert abs(obj - best) <= 1e-9, (trial, obj, best)
        assert R.legal(ids, TABLE5)
        assert abs(R.objective(ids, z, TABLE5, W, forced) - obj) <= 1e-9
        assert R.forbidden_successions(ids, TABLE5, W) == 0
        if forced is not None:
            assert (ids[forced] == 1).all()
            seen_forced += int(forced.sum())
        seen_forbidden += int(np.isneginf(W).sum())
    assert seen_forced and seen_forbidden


@pytest.mark.parametrize("lam", [0.0, 1.5, 4.0])
def test_a_flat_table_is_the_switch_penalty(lam):
    rng = np.random.default_rng(3)
    table = (0, [(1, 2), (3, 4), (5, -1)])
    for T in (1, 7, 60):
        z = rng.standard_normal((T, 8)) * 3
        forced = rng.random(T) < 0.2
        W = np.full((4, 4), -lam)
        ids, obj = R.viterbi(z, table, W, forced)
        _, want = V.viterbi(z, table, lam, forced)
        assert abs(obj - want) <= 1e-9
        assert abs(V.objective(ids, z, table, lam, forced) - want) <= 1e-9
        assert abs(R.score(ids, z, table, W, forced) - V.score(ids, z, table, lam, forced)) <= 1e-9


def _write_labs(d):
    """Three hand-written files.  a: a leading gap, then a i (touching) and a gap before k.  b: starts at 0, a a (a repeated phoneme),
    a 10 ms gap (below min_gap: no O) before i.  c: one segment k at 0."""
    labs = {"a.lab": "5000000 6000000 a\n6000000 7000000 i\n9000000 9500000 k\n",
            "b.lab": "0 1000000 a\n1000000 2000000 a\n2100000 3000000 i\n",
            "c.lab": "0 4000000 k\n"}
    for n, txt in labs.items():
        (d / n).write_text(txt)
    return [str(d / n) for n in sorted(labs)]


def test_estimate_counts_and_log_probabilities_by_hand(tmp_path):
    paths = _write_labs(tmp_path)
    bg = PH.estimate(paths, smoothing=1.0, min_gap=0.02)
    assert bg.symbols == ["O", "a", "i", "k"]
    # a.lab: O->a, a->i, i->O, O->k;  b.lab: O->a, a->a, a->i;  c.lab: O->k
    want = np.array([[0, 2, 0, 2],
                     [0, 1, 2, 0],
                     [1, 0, 0, 0],
                     [0, 0, 0, 0]])
    assert (bg.counts == want).all()
    # add-one over the three phonemes for row O (O -> O is no succession), over all four symbols for the other rows
    lp = np.log(np.array([[np.nan, 3 / 7, 1 / 7, 3 / 7],
                          [1 / 7, 2 / 7, 3 / 7, 1 / 7],
                          [2 / 5, 1 / 5, 1 / 5, 1 / 5],
                          [1 / 4, 1 / 4, 1 / 4, 1 / 4]]))
    assert np.isneginf(bg.log_prob[0, 0])
    m = ~np.isnan(lp)
    assert np.allclose(bg.log_prob[m], lp[m], rtol=0, atol=1e-12)
    # without smoothing what was never seen is forbidden; a row never seen is forbidden altogether
    raw = PH.estimate(paths, smoothing=0.0)
    assert np.isclose(raw.log_prob[1, 2], np.log(2 / 3)) and np.isneginf(raw.log_prob[1, 3]) and np.isneginf(raw.log_prob[3]).all()
    # a larger min_gap: the 200 ms gap of a.lab is no O either, only the leading one (which costs nothing: the file starts after O)
    wide = PH.estimate(paths, min_gap=0.3)
    assert wide.counts[2].tolist() == [0, 0, 0, 1] and wide.counts[0].tolist() == [0, 2, 0, 1]
    # given symbols: their order, phonemes without a count included; a phoneme of the files outside them is named
    given = PH.estimate(paths, symbols=["k", "zz", "O", "i", "a"])
    assert given.symbols == ["O", "k", "zz", "i", "a"] and given.counts[0].tolist() == [0, 2, 0, 0, 2]
    assert np.isfinite(given.log_prob[2, 1:]).all()
    with pytest.raises(ValueError, match="i, k"):
        PH.estimate(paths, symbols=["a"])


def test_save_and_load_round_trip(tmp_path):
    paths = _write_labs(tmp_path)
    for k in (1.0, 0.0):
        bg = PH.estimate(paths, smoothing=k)
        f = tmp_path / f"bg{k}.json"
        PH.save(bg, str(f))
        raw = json.loads(f.read_text())
        assert raw["symbols"] == bg.symbols and raw["log_prob"][0][0] is None
        assert (k > 0) or raw["log_prob"][1][3] is None
        back = PH.load(str(f))
        assert back.symbols == bg.symbols
        assert (np.isneginf(back.log_prob) == np.isneginf(bg.log_prob)).all()
        fin = np.isfinite(bg.log_prob)
        assert (back.log_prob[fin] == bg.log_prob[fin]).all()
    bad = tmp_path / "bad.json"
    bad.write_text('{"symbols": ["a", "O"], "log_prob": [[0, 0], [0, 0]]}')
    with pytest.raises(ValueError, match="begin with 'O'"):
        PH.load(str(bad))
    bad.write_text('{"symbols": ["O", "a"], "log_prob": [[0, 0]]}')
    with pytest.raises(ValueError, match="2 x 2"):
        PH.load(str(bad))


def test_transition_table_orders_weighs_and_refuses():
    labels = ["B-k", "I-k", "O", "B-a", "I-a", "B-q"]                  # class_table order: k (0, 1), a (3, 4), q (5, -1)
    table = DC.class_table(labels)
    assert table.o_id == 2 and table.pairs.tolist() == [[0, 1], [3, 4], [5, -1]]
    syms = ["O", "a", "q", "k"]
    lp = -np.arange(16, dtype=np.float64).reshape(4, 4) / 4
    lp[1, 2] = -np.inf
    bg = PH.Bigram(syms, lp)
    W = PH.transition_table(bg, table, labels, switch_penalty=0.5, weight=2.0)
    assert W.dtype == np.float32 and W.shape == (4, 4)
    order = [0, 3, 1, 2]                                               # O, k, a, q in the file's indices
    for i, a in enumerate(order):
        for j, b in enumerate(order):
            if (i, j) == (0, 0):
                continue
            want = -np.inf if np.isneginf(lp[a, b]) else np.float32(2.0 * lp[a, b] - 0.5)
            assert W[i, j] == want, (i, j)
    assert np.isneginf(W[2, 3])                                        # a -> q stays forbidden
    DC.check_transitions(W, 3)
    flat = PH.transition_table(bg, table, labels, switch_penalty=1.25, weight=0.0)
    assert (flat == np.float32(-1.25)).all()                           # weight 0: the plain search, forbidden entries included
    with pytest.raises(ValueError, match="lacks phonemes of the label set: k"):
        PH.transition_table(PH.Bigram(["O", "a", "q"], lp[:3, :3]), table, labels)
    with pytest.raises(ValueError, match="the label set lacks: zz"):
        PH.transition_table(PH.Bigram(syms + ["zz"], np.zeros((5, 5))), table, labels)
    with pytest.raises(ValueError, match="bigram_weight"):
        PH.transition_table(bg, table, labels, weight=-1.0)


def test_the_command_line_tool_emits_every_phoneme_of_the_label_set(tmp_path):
    _write_labs(tmp_path)
    labels = ["O", "B-a", "I-a", "B-i", "I-i", "B-k", "I-k", "B-zz", "I-zz"]
    (tmp_path / "phonemes.txt").write_text("\n".join(labels) + "\n")
    out = tmp_path / "out" / "phoneme_bigram.json"
    PH.main([str(tmp_path), "-o", str(out), "--phonemes", str(tmp_path / "phonemes.txt"), "--smoothing", "0.5", "--min-gap", "0.02"])
    bg = PH.load(str(out))
    assert bg.symbols == ["O", "a", "i", "k", "zz"]
    W = PH.transition_table(bg, DC.class_table(labels), labels, 0.0, 1.0)
    DC.check_transitions(W, 4)
    assert np.isclose(W[1, 2], np.log(2.5 / 5.5), atol=1e-6)


def test_option_validation():
    """(how the options are resolved against the config, and the rules: tests/test_options_cpu.py)"""
    from wfl_asr_amd.infer import infer_audio
    with pytest.raises(ValueError, match="need decode='viterbi'"):      # refused before any model is loaded
        infer_audio("x.wav", decode="argmax", phoneme_bigram="bg.json")


def test_check_transitions():
    W = np.zeros((3, 3), np.float32)
    assert DC.check_transitions(W, 2) is not None
    for bad, what in ((np.nan, "NaN"), (np.inf, r"\+inf")):
        Wb = W.copy()
        Wb[1, 2] = bad
        with pytest.raises(ValueError, match=what):
            DC.check_transitions(Wb, 2)
    with pytest.raises(ValueError, match=r"\[3, 3\]"):
        DC.check_transitions(np.zeros((2, 3), np.float32), 2)
    with pytest.raises(ValueError, match="float32"):
        DC.check_transitions(W.astype(np.float64), 2)
    Wb = W.copy()
    Wb[2, 0] = -np.inf
    with pytest.raises(ValueError, match=r"\[p\]\[O\]"):
        DC.check_transitions(Wb, 2)
    for v in (-np.inf, np.nan, np.inf):                 # [O][O] is never read: anything may stand there
        Wb = W.copy()
        Wb[0, 0] = v
        assert np.isfinite(DC.check_transitions(Wb, 2)).all() and Wb[0, 0] != 0


def test_abi_entries_and_the_symbol_cap():
    from wfl_asr_amd import _lib
    src = open(os.path.join(ROOT, "include", "wfl_asr.h")).read()
    for name in ("wfl_decode_bigram_workspace_bytes", "wfl_decode_bigram"):
        assert re.search(rf"\b{name}\s*\(", src) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["wfl_decode_bigram"][1]) == 17
    cap = int(re.search(r"#define\s+WFL_DECODE_BIGRAM_MAX_SYMBOLS\s+(\d+)", src).group(1))
    assert cap == DC.MAX_BIGRAM_SYMBOLS == 192
    import __graft_entry__ as g
    g.build()
    T = np.array([10, 0, 7], np.int32)
    # per clip with T > 0: round_up_64(T ceil(N / 2)) + 2 round_up_64(T) words
    assert DC.bigram_workspace_bytes(T, 70) == 4 * ((384 + 128) + (256 + 128))
    assert DC.bigram_workspace_bytes(T, 191) == 4 * ((960 + 128) + (704 + 128))
    assert DC.bigram_workspace_bytes(T, 192) == 0                       # over the cap: nothing is searched


def test_decode_bigram_validates_its_arguments_without_gpu():
    """wfl_decode_bigram's host side: the bad arguments of test_decode_cpu.py's list that the entry has (it takes no lambda), a null
    `trans` with frames present, and the workspace rule in full."""
    import ctypes
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    buf = (ctypes.c_char * 64)()
    d = ctypes.cast(buf, P)                        # never dereferenced: every call below fails on the host
    fo = np.zeros(1, np.int64)
    T = np.array([10], np.int32)
    h = lambda a: a.ctypes.data_as(P)              # noqa: E731

    def call(C=141, o_id=0, ldl=141, fo_=fo, T_=T, ws=None, ws_bytes=0, logits=d, n=1, ids=d, pairs=d, n_pairs=70, trans=d, thr=0.0,
             score=d, status=d):
        return lib.wfl_decode_bigram(logits, ldl, C, o_id, h(fo_) if fo_ is not None else None, h(T_), n, pairs, n_pairs, trans, thr, ws,
                                     ws_bytes, ids, score, status, None)

    need = lib.wfl_decode_bigram_workspace_bytes(h(T), 1, 70)
    assert need > 0
    for kw, word in ((dict(C=0), b"C < 1"), (dict(o_id=141), b"o_id"), (dict(o_id=-1), b"o_id"), (dict(ldl=100), b"ldl"),
                     (dict(n=-1), b"negative count"), (dict(n_pairs=-1), b"negative count"), (dict(thr=-0.1), b"threshold"),
                     (dict(thr=float("nan")), b"threshold"), (dict(fo_=None, ws=d, ws_bytes=need), b"null host"),
                     (dict(T_=np.array([-2], np.int32), ws=d, ws_bytes=need), b"negative"),
                     (dict(fo_=np.array([-1], np.int64), ws=d, ws_bytes=need), b"negative offset"),
                     (dict(logits=None, ws=d, ws_bytes=need), b"null device"), (dict(ids=None, ws=d, ws_bytes=need), b"null device"),
                     (dict(score=None, ws=d, ws_bytes=need), b"null device"), (dict(status=None, ws=d, ws_bytes=need), b"null device"),
                     (dict(pairs=None, ws=d, ws_bytes=need), b"null device"), (dict(trans=None, ws=d, ws_bytes=need), b"null device"),
                     (dict(ws=d, ws_bytes=need - 1), b"workspace"), (dict(ws=None, ws_bytes=need), b"workspace")):
        assert call(**kw) != 0, kw
        err = lib.wfl_last_error()
        assert b"wfl_decode_bigram" in err and word in err, (kw, err)
    assert call(n=0) == 0                          # nothing to do

    # per clip with T > 0: round_up_64(T ceil(N / 2)) + 2 round_up_64(T) words, N = n_pairs + 1; nothing is searched over the cap
    r64 = lambda v: (v + 63) // 64 * 64            # noqa: E731
    Ts = [1500, 1, 0, 63, 64, 65]
    Tn = np.array(Ts, np.int32)
    size = lib.wfl_decode_bigram_workspace_bytes
    for n_pairs in (0, 1, 70, 190, 191):
        want = sum(4 * (r64(t * ((n_pairs + 2) // 2)) + 2 * r64(t)) for t in Ts if t > 0)
        assert size(h(Tn), len(Ts), n_pairs) == want, n_pairs
    assert size(h(Tn), len(Ts), 192) == 0
    assert size(h(Tn), -1, 70) < 0 and size(h(Tn), 1, -1) < 0
    assert size(h(np.array([-1], np.int32)), 1, 70) < 0
    assert size(None, 1, 70) < 0
    assert size(None, 0, 70) == 0
