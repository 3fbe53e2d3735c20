"""CPU (-m "not gpu"): the float64 restatement of wfl_decode_duration (tests/bio_duration_ref.py) against the enumeration of every class
string, its reduction to the bigram search without a prior, the rules of `postprocess.decode_duration_prior` (options.py), the naming
rule of decode.duration_symbol_rows, durations.check's refusals, and the host side of the C ABI entry (no GPU is touched: every bad
call returns before a launch)."""
import ctypes

import numpy as np
import pytest

import bio_bigram_ref as RB
import bio_duration_ref as R
from wfl_asr_amd import decode as DC
from wfl_asr_amd import durations as DU
from wfl_asr_amd import options as OPT
from wfl_asr_amd.options import PostOptions, resolve

# O, two phonemes with an I class, one without: six classes (the smallest table with all three kinds)
TABLE = (1, [(0, 2), (3, 4), (5, -1)])
C = 6


def _tiny_case(seed):
    rng = np.random.default_rng(seed)
    T, D = int(rng.integers(1, 7)), int(rng.integers(1, 4))
    z = rng.standard_normal((T, C)) * 2
    W = -3.0 * rng.random((4, 4))
    mask = rng.random((4, 4)) < 0.2
    mask[:, 0] = False
    W[mask] = -np.inf
    dur = -4.0 * rng.random((3, D + 1))
    dur[rng.random((3, D + 1)) < 0.25] = -np.inf
    dur[rng.random(3) < 0.3, D] = -np.inf
    sd = rng.integers(-1, 3, size=3)
    forced = rng.random(T) < 0.2
    return z, W, dur, sd, forced


def test_the_reference_s_optimum_is_the_enumeration_s():
    seen_D, seen_tail, seen_forced = set(), 0, 0
    for seed in range(240):
        z, W, dur, sd, forced = _tiny_case(seed)
        ids, obj = R.viterbi(z, TABLE, W, dur, sd, forced)
        _, best = R.brute_force(z, TABLE, W, dur, sd, forced)
        assert R.legal(ids, TABLE) and (ids[forced] == TABLE[0]).all()
        assert abs(R.objective(ids, z, TABLE, W, dur, sd, forced) - obj) <= 1e-9, seed
        assert abs(best - obj) <= 1e-9, (seed, best, obj)
        D = dur.shape[1] - 1
        seen_D.add(D)
        seen_tail += any(k > D for _, _, k in R.run_lengths(ids, TABLE))
        seen_forced += bool(forced.any())
    assert seen_D == {1, 2, 3} and seen_tail >= 10 and seen_forced >= 50      # the cases do reach the tail and forced frames


def test_objective_and_run_lengths_on_a_path_by_hand():
    o, (b, i), (b2, _) = TABLE[0], TABLE[1][0], TABLE[1][2]
    ids = np.array([b, i, i, i, o, b2, b], np.int32)
    assert R.run_lengths(ids, TABLE) == [(1, 0, 4), (3, 5, 1), (1, 6, 1)]
    z = np.zeros((7, C))
    W = -np.arange(16.0).reshape(4, 4)
    dur = np.array([[-1.0, -2.0, -0.5], [-10.0, -20.0, -30.0]])
    sd = [0, -1, 1]
    #   O->1, 1->O, O->3, 3->1;  L_1(4) = L(2) + 2 tail, L_3(1) = row 1's L(1), L_1(1)
    want = (W[0, 1] + W[1, 0] + W[0, 3] + W[3, 1]) + (-2.0 + 2 * -0.5) + -10.0 + -1.0
    assert R.objective(ids, z, TABLE, W, dur, sd) == want
    assert R.objective(ids, z, TABLE, W, dur, sd, forced=np.array([0, 0, 1, 0, 0, 0, 0], bool)) == -np.inf
    dur[0, 2] = -np.inf                         # no run of phoneme 0 beyond 2 frames
    assert R.objective(ids, z, TABLE, W, dur, sd) == -np.inf and R.forbidden_durations(ids, TABLE, dur, sd) == 1


@pytest.mark.parametrize("prior", ["none", "zero"])
def test_without_a_prior_the_search_is_the_bigram_s(prior):
    for seed in range(30):
        rng = np.random.default_rng(900 + seed)
        T, D = int(rng.integers(1, 60)), int(rng.integers(1, 9))
        z = rng.standard_normal((T, C)) * 2
        W = -3.0 * rng.random((4, 4))
        forced = rng.random(T) < 0.1
        dur = np.zeros((2, D + 1))
        sd = [-1, -1, -1] if prior == "none" else [0, 1, 0]
        a = RB.viterbi(z, TABLE, W, forced)
        b = R.viterbi(z, TABLE, W, dur, sd, forced)
        assert (a[0] == b[0]).all() and abs(a[1] - b[1]) <= 1e-9


def test_options_defaults_and_rules():
    plain = resolve({})
    assert plain.decode_duration_prior is None and plain.decode_duration_prior_weight == 1.0
    assert OPT.DEFAULT_DURATION_PRIOR_WEIGHT == 1.0
    a = resolve({"decode": "viterbi", "decode_duration_prior": "d.json"})
    assert a.decode_duration_prior == "d.json" and a.decode_duration_prior_weight == 1.0 and a.duration_prior is None
    assert isinstance(a, PostOptions) and len(a) == 8 and a != resolve({"decode": "viterbi"}) and hash(a) != hash(resolve({"decode": "viterbi"}))
    assert "decode_duration_prior='d.json'" in repr(a) and a._asdict()["decode_duration_prior_weight"] == 1.0
    assert a._replace(decode_duration_prior=None) == resolve({"decode": "viterbi"})
    assert len(PostOptions._KEYWORD) == len(PostOptions._KEYWORD_DEFAULTS)
    assert resolve({"decode": "viterbi"}, decode_duration_prior="x", decode_duration_prior_weight=0).decode_duration_prior_weight == 0.0
    assert resolve({"decode": "viterbi", "decode_duration_prior": "d.json"}, decode_duration_prior="").decode_duration_prior is None
    # with a bigram and with a switch penalty it stands
    b = resolve({"decode": "viterbi", "phoneme_bigram": "b.json", "switch_penalty": 1.5, "decode_duration_prior": "d.json"})
    assert b.phoneme_bigram == "b.json" and b.decode_duration_prior == "d.json"
    # the alignment's prior is another key: neither implies the other
    c = resolve({"align": "viterbi", "duration_prior": "t.json"})
    assert c.duration_prior == "t.json" and c.decode_duration_prior is None
    for post, message in (
            ({"decode_duration_prior": "d.json"}, "need decode='viterbi'"),
            ({"decode": "argmax", "decode_duration_prior": "d.json"}, "need decode='viterbi'"),
            ({"decode_duration_prior_weight": 2.0}, "need decode='viterbi'"),
            ({"decode": "viterbi", "decode_duration_prior_weight": 2.0}, "decode_duration_prior_weight needs a decode_duration_prior"),
            ({"decode": "viterbi", "decode_duration_prior": "d.json", "decode_duration_prior_weight": -1}, "finite number >= 0"),
            ({"decode": "viterbi", "decode_duration_prior": "d.json", "decode_duration_prior_weight": float("inf")}, "finite number >= 0"),
            ({"decode": "viterbi", "decode_duration_prior": "d.json", "decode_duration_prior_weight": True}, "finite number >= 0"),
            ({"decode": "viterbi", "decode_duration_prior": "d.json", "decode_duration_prior_weight": "much"}, "finite number >= 0"),
            ({"decode": "viterbi", "decode_duration_prior": "d.json", "decode_scores": True}, OPT.DECODE_DURATION_PRIOR_ERROR),
            ({"decode": "viterbi", "decode_duration_prior": "d.json", "phoneme_bigram": "b.json", "bigram_scores": True},
             OPT.DECODE_DURATION_PRIOR_ERROR)):
        with pytest.raises(ValueError) as err:
            resolve(post)
        assert message in str(err.value), (post, str(err.value))
    assert "decode_scores" in OPT.DECODE_DURATION_PRIOR_ERROR and "bigram_scores" in OPT.DECODE_DURATION_PRIOR_ERROR


def test_duration_symbol_rows_follows_the_output_names():
    labels = ["O", "B-a", "I-a", "B-aa", "I-aa", "B-k", "B-t", "I-t", "I-x"]
    table = DC.class_table(labels)
    assert [labels[b][2:] for b, _ in table.pairs] == ["a", "aa", "k", "t"]
    row = np.array([-1.0, -2.0])
    prior = DU.DurationPrior(0.02, 2, ["t", "A", "k", "q"], [row, row, None, row], np.full(4, -0.5))
    # two phonemes, one output name: both take its row; k's row is null; t by its own name; q is nobody's
    got = DC.duration_symbol_rows(prior, table, labels, {"a": "A", "aa": "A"})
    assert got.dtype == np.int32 and got.tolist() == [1, 1, -1, 0]
    assert DC.duration_symbol_rows(prior, table, labels).tolist() == [-1, -1, -1, 0]       # without a map the label names are the output names
    assert DU.table(prior).shape == (4, 3)                                                  # the rows are the prior's own numbering


def test_check_refuses_another_clock_and_an_unknown_phoneme():
    prior = DU.flat(["a", "k"], 4, 0.02)
    DU.check(prior, ["a", "k", "t"], 0.02)
    with pytest.raises(ValueError, match="counted on frames of 0.01 s"):
        DU.check(DU.flat(["a"], 4, 0.01), ["a"], 0.02)
    with pytest.raises(ValueError, match="no output name of the label set: k"):
        DU.check(prior, ["a", "t"], 0.02, path="d.json")


def test_table_checks_of_the_python_entry():
    good = np.zeros((2, 5), np.float32)
    assert DC.check_duration_table(good).shape == (2, 5) and DC.check_duration_table(np.zeros((0, 3), np.float32)).shape == (0, 3)
    for bad, message in ((good.astype(np.float64), "dur must be float32"), (np.zeros((2, 1), np.float32), "D \\+ 1"),
                         (np.zeros((2, 34), np.float32), "D \\+ 1"), (np.zeros(5, np.float32), "D \\+ 1")):
        with pytest.raises(ValueError, match=message):
            DC.check_duration_table(bad)
    for v, message in ((np.nan, "NaN"), (np.inf, "\\+inf")):
        t = good.copy()
        t[1, 1] = v
        with pytest.raises(ValueError, match=message):
            DC.check_duration_table(t)
    t = good.copy()
    t[0, 4] = 1e-3
    with pytest.raises(ValueError, match="tail of dur"):
        DC.check_duration_table(t)
    t[0, 4] = -np.inf
    DC.check_duration_table(t)
    assert DC.check_symbol_rows(np.array([-1, 1, 0], np.int32), 3, 2).tolist() == [-1, 1, 0]
    for bad, message in ((np.array([0, 0, 0]), "int32"), (np.array([0, 0], np.int32), "one row per phoneme"),
                         (np.array([0, -2, 0], np.int32), "-1 .. 1"), (np.array([0, 2, 0], np.int32), "-1 .. 1")):
        with pytest.raises(ValueError, match=message):
            DC.check_symbol_rows(bad, 3, 2)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import _lib
    return _lib.load()


def test_the_abi_entry_is_declared_and_bound(lib):
    from wfl_asr_amd import _lib
    assert len(_lib.SIGNATURES["wfl_decode_duration"][1]) == 21
    assert len(_lib.SIGNATURES["wfl_decode_duration_workspace_bytes"][1]) == 4
    assert lib.wfl_decode_duration is not None and DC.MAX_DURATION == DU.MAX_FRAMES == 32


def test_workspace_bytes_formula(lib):
    h = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    size = lib.wfl_decode_duration_workspace_bytes
    r64 = lambda x: (x + 63) // 64 * 64                   # noqa: E731
    T = np.array([300, 0, 17], np.int32)

    def want(P, D):
        N = P + 1
        HS = r64(N)
        table = (max(4 * N * N, 128 * ((N + 1) // 2)) + 15) // 16 * 16
        H = 0 if table + 8448 + 4 * (2 * D + 1) * HS <= 163840 - 4416 else r64((2 * D + 1) * HS)
        return 4 * sum(r64(int(t) * ((N + 1) // 2)) + H + 2 * r64(int(t)) for t in T if t > 0)
    for P, D in ((1, 1), (70, 32), (140, 32), (170, 8), (191, 1), (191, 2), (191, 32)):
        assert size(h(T), 3, P, D) == want(P, D) == DC.duration_workspace_bytes(T, P, D), (P, D)
    # the history is in LDS at 141 symbols for every D, at the cap for D = 1 alone
    assert size(h(T), 3, 140, 32) == lib.wfl_decode_bigram_workspace_bytes(h(T), 3, 140)
    assert size(h(T), 3, 191, 1) == lib.wfl_decode_bigram_workspace_bytes(h(T), 3, 191) < size(h(T), 3, 191, 2)
    assert size(h(T), 3, 192, 8) == 0                    # over the symbol cap: nothing is searched
    for bad_D in (0, 33, -1):
        assert size(h(T), 3, 70, bad_D) == -1
    assert size(None, 3, 70, 8) == -1 and size(h(T), -1, 70, 8) == -1 and size(h(np.array([-1], np.int32)), 1, 70, 8) == -1
    with pytest.raises(Exception, match="wfl_decode_duration_workspace_bytes"):
        DC.duration_workspace_bytes(T, 70, 33)


def test_host_side_argument_checks(lib):
    """Every bad call returns a negative code and names the entry before anything is launched (the pointers are never read)."""
    P, Cn, D = 70, 141, 8
    T = np.array([100], np.int32)
    fo = np.array([0], np.int64)
    h = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    buf = (ctypes.c_char * 64)()
    dev = ctypes.cast(buf, ctypes.c_void_p)              # stands for a device pointer
    need = lib.wfl_decode_duration_workspace_bytes(h(T), 1, P, D)
    assert need > 0

    def call(**kw):
        a = dict(logits=dev, ldl=Cn, C=Cn, o_id=0, fo=fo, T=T, n=1, pairs=dev, n_pairs=P, trans=dev, sym_dur=dev, dur=dev, n_rows=4, D=D,
                 thr=0.5, ws=dev, ws_n=need, ids=dev, score=dev, status=dev)
        a.update(kw)
        return lib.wfl_decode_duration(a["logits"], a["ldl"], a["C"], a["o_id"], h(a["fo"]) if a["fo"] is not None else None,
                                       h(a["T"]) if a["T"] is not None else None, a["n"], a["pairs"], a["n_pairs"], a["trans"], a["sym_dur"],
                                       a["dur"], a["n_rows"], a["D"], a["thr"], a["ws"], a["ws_n"], a["ids"], a["score"], a["status"], None)
    for kw, word in ((dict(D=0), b"D must be 1 .. 32"), (dict(D=33), b"D must be 1 .. 32"), (dict(n_rows=-1), b"n_rows < 0"),
                     (dict(dur=None), b"null dur"), (dict(sym_dur=None), b"null sym_dur"), (dict(trans=None), b"null device pointer"),
                     (dict(ws_n=need - 4), b"workspace too small"), (dict(ws=None), b"workspace too small"),
                     (dict(C=0), b"C < 1"), (dict(o_id=Cn), b"o_id"), (dict(ldl=Cn - 1), b"ldl"), (dict(n=-1), b"negative count"),
                     (dict(n_pairs=-1), b"negative count"), (dict(thr=-0.5), b"threshold"), (dict(fo=None), b"null host array"),
                     (dict(T=np.array([-1], np.int32)), b"negative offset or frame count"), (dict(logits=None), b"null device pointer"),
                     (dict(ids=None), b"null device pointer"), (dict(score=None), b"null device pointer"),
                     (dict(status=None), b"null device pointer"), (dict(pairs=None), b"null device pointer")):
        rc = call(**kw)
        err = lib.wfl_last_error()
        assert rc < 0, kw
        assert b"wfl_decode_duration" in err and word in err, (kw, err)
    # an empty batch is fine and launches nothing; so is a null dur without rows and a null sym_dur without phonemes or frames
    assert call(n=0) == 0
    assert call(n=0, dur=None, n_rows=0, sym_dur=None) == 0
