"""CPU (-m "not gpu"): the definition of the explicit-duration forced alignment (tests/viterbi_duration_prior_ref.py against the
enumeration of every segmentation), its two special cases (no prior: viterbi_ref; a hard table: viterbi_min_ref), the packers and
`duration_rows`, the ABI entry's host-side checks, and the option rules of `postprocess.duration_prior`."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import viterbi_duration_prior_ref as DP
import viterbi_min_ref as M
import viterbi_ref as V
import viterbi_window_ref as W

NEG = -np.inf


@pytest.fixture(scope="module")
def AL():
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import align
    return align


def _table(n_rows, D, rng, p_inf=0.25):
    t = rng.uniform(-3, 0, (n_rows, D + 1))
    t[rng.random((n_rows, D + 1)) < p_inf] = NEG
    return t


# ------------------------------------------------------------------------------------------------ 1. the definition
def test_dp_equals_enumeration_of_all_segmentations():
    """T <= 7, N <= 3, D <= 3, -inf entries and -inf tails among them, with and without windows."""
    rng = np.random.default_rng(101)
    C = 9
    cases = finite = none = tails = changed = windowed = 0
    while cases < 300:
        T, N, D = int(rng.integers(1, 8)), int(rng.integers(0, 4)), int(rng.integers(1, 4))
        alts = [[(1 + 2 * k, 2 + 2 * k)] for k in range(N)]
        z = rng.standard_normal((T, C))
        table = _table(3, D, rng)
        rows = [int(r) for r in rng.integers(-1, 3, N)]
        wins = None
        if N and rng.random() < 0.3:
            wins = [(int(lo), int(lo) + int(rng.integers(0, 4))) for lo in rng.integers(0, T, N)]
            windowed += 1
        best = DP.brute_force(z, alts, [0, 7], rows, table, wins)
        ref = DP.viterbi(z, alts, [0, 7], rows, table, wins)
        cases += 1
        assert (ref is None) == (best is None), (T, N, D, rows, table)
        if ref is None:
            none += 1
            continue
        finite += 1
        states, score, runs = ref
        assert V.legal(states, N) and (wins is None or W.in_windows(states, wins))
        assert abs(score - best) < 1e-9 and abs(DP.path_score(states, z, alts, [0, 7], rows, table, wins) - best) < 1e-9
        assert runs.sum() == (states % 3 != 0).sum() and (runs >= 1).all()
        tails += int((runs > D).any())
        if N and T >= N:
            changed += abs(V.viterbi(z, alts, [0, 7])[1] - best) > 1e-9
    print(cases, finite, none, tails, changed, windowed)
    assert cases >= 200 and finite > 80 and none > 20 and tails >= 8 and changed > 50 and windowed > 30


def test_without_a_prior_it_is_the_plain_dp():
    rng = np.random.default_rng(102)
    for T, N in ((1, 0), (1, 1), (9, 3), (40, 12), (40, 40)):
        alts = [[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 9, N)]
        z = rng.standard_normal((T, 20))
        _, want = V.viterbi(z, alts, [0, 19])
        for rows, table in (([-1] * N, _table(2, 3, rng)), ([0] * N, np.zeros((1, 5)))):
            states, score, _ = DP.viterbi(z, alts, [0, 19], rows, table)
            assert abs(score - want) < 1e-9 and abs(V.path_score(states, z, alts, [0, 19]) - want) < 1e-9
    assert DP.viterbi(rng.standard_normal((2, 20)), [[(1, 2)]] * 3, [0], [-1] * 3, np.zeros((1, 2))) is None


def test_a_hard_table_is_the_minimum_duration_dp():
    """L(d) = -inf below D_k, 0 from there on, tail 0."""
    rng = np.random.default_rng(103)
    table = np.zeros((8, 9))
    for d in range(1, 9):
        table[d - 1, :d - 1] = NEG
    for T, N in ((12, 2), (30, 5), (60, 9)):
        alts = [[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 9, N)]
        z = rng.standard_normal((T, 20))
        D = rng.choice([1, 2, 3, 8], N)
        path, want = M.viterbi(z, alts, [0, 19], D)
        got = DP.viterbi(z, alts, [0, 19], (D - 1).tolist(), table)
        if path is None:
            assert got is None
            continue
        assert abs(got[1] - want) < 1e-9 and (got[2] >= D).all()
    # and a tail of -inf is a hard maximum
    z = np.zeros((20, 5))
    z[:, 1:3] = 5.0                                                      # the token's classes win every frame
    states, _, runs = DP.viterbi(z, [[(1, 2)]], [0], [0], np.array([[0.0, 0.0, 0.0, NEG]]))
    assert runs[0] == 3 and V.legal(states, 1)
    assert DP.viterbi(z, [[(1, 2)]], [0], [0], np.array([[0.0, 0.0, 0.0, 0.0]]))[2][0] == 20


# ------------------------------------------------------------------------------------------------ 2. the host side
def test_pack_durations(AL):
    N = np.array([2, 0, 1], np.int32)
    d = AL._pack_durations([[3, -1], None, None], N)
    assert d.dtype == np.int32 and d.tolist() == [3, -1, -1]
    assert AL._pack_durations([None, None, [99]], N).tolist() == [-1, -1, 99]       # (out of range: the kernel's status 4, not the packing's)
    assert AL._pack_durations([], np.zeros(0, np.int32)).tolist() == [-1]
    with pytest.raises(ValueError, match="2 tokens"):
        AL._pack_durations([[3], None, None], N)
    with pytest.raises(ValueError, match="one entry per clip"):
        AL._pack_durations([None], N)
    for bad in ([2.0, 1], [True, 1], ["2", 1]):
        with pytest.raises(ValueError, match="ints"):
            AL._pack_durations([bad, None, None], N)
    with pytest.raises(ValueError, match="int32"):
        AL._pack_durations([[2 ** 31, 1], None, None], N)
    sig = inspect.signature(AL.viterbi_align_duration_prior).parameters
    assert list(sig)[:7] == ["logits", "n_frames", "token_classes", "gap_classes", "o_id", "tok_rows", "table"]
    assert all(sig[k].default is None for k in ("frame_offsets", "stream", "packed", "windows"))
    assert callable(AL.upload_durations) and AL.MAX_PRIOR_FRAMES == 32
    assert AL.AlignBatch._fields[-1] == "durs" and AL.AlignBatch._field_defaults["durs"] is None


def test_duration_rows(AL):
    from wfl_asr_amd.durations import DurationPrior
    prior = DurationPrior(0.02, 2, ["a", "b", "SP"], [np.zeros(2), None, np.zeros(2)], np.zeros(3))
    assert AL.duration_rows(["a", "SP", "b", "zz", "a"], prior) == [0, 2, -1, -1, 0]
    assert AL.duration_rows([], prior) == []
    assert all(type(x) is int for x in AL.duration_rows(["a", "b"], prior))


def test_the_abi_entry_checks_its_arguments(AL):
    from wfl_asr_amd import _lib
    lib = _lib.load()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wfl_asr.h")).read()
    assert "wfl_align_duration_prior(" in src and hasattr(ctypes.CDLL(_lib.LIB_PATH), "wfl_align_duration_prior")
    assert len(_lib.SIGNATURES["wfl_align_duration_prior"][1]) == len(_lib.SIGNATURES["wfl_align_windowed"][1]) + 4
    Pv = ctypes.c_void_p
    buf = (ctypes.c_char * 64)()
    d = ctypes.cast(buf, Pv)                       # never dereferenced: every call below fails on the host
    fo, ko = np.zeros(1, np.int64), np.zeros(1, np.int32)
    T, N = np.array([10], np.int32), np.array([3], np.int32)
    h = lambda a: a.ctypes.data_as(Pv)             # noqa: E731
    need = lib.wfl_align_duration_prior_workspace_bytes(h(T), h(N), 1, 8)
    assert need == 4 * 64 * 10                     # a byte per slot and frame: 64 words per frame at N <= 127, the ring in LDS
    assert lib.wfl_align_duration_prior_workspace_bytes(h(T), h(N), 1, 0) == -1
    assert lib.wfl_align_duration_prior_workspace_bytes(h(T), h(N), 1, 33) == -1
    big_t, big_n = np.array([3000, 3000, 5000, 2], np.int32), np.array([600, 2048, 4096, 3], np.int32)

    def words(D):
        return lib.wfl_align_duration_prior_workspace_bytes(h(big_t), h(big_n), 4, D) // 4
    r64 = lambda x: (x + 63) // 64 * 64            # noqa: E731
    assert words(1) == 3000 * 256 + 3000 * 1536 + 5000 * 1536                         # every ring in LDS; T < N: no words
    assert words(9) == words(1) + r64(4608 * 9) * 2                                   # N > 2047: the ring in the workspace from D = 2
    assert words(32) == words(1) + r64(1024 * 32) + r64(4608 * 32) * 2                # N <= 1023: from D = 24

    def align(win=None, dur_rows=d, table=d, n_rows=4, D=8, ws_bytes=need, C=141):
        return lib.wfl_align_duration_prior(d, 141, C, 0, h(fo), h(T), h(ko), h(N), d, win, d, 1, dur_rows, table, n_rows, D, d, ws_bytes,
                                            d, d, d, d, None)
    for win in (None, d):                          # tok_win is nullable
        assert align(win, dur_rows=None) == -1 and b"wfl_align_duration_prior: null tok_dur" in lib.wfl_last_error()
        assert align(win, table=None) == -1 and b"null dur" in lib.wfl_last_error()
        assert align(win, n_rows=-1) == -1 and b"n_rows" in lib.wfl_last_error()
        for D in (0, 33, -1):
            assert align(win, D=D) == -1 and b"D must be 1 .. 32" in lib.wfl_last_error()
        assert align(win, C=0) != 0 and b"wfl_align_duration_prior: C must" in lib.wfl_last_error()
        assert align(win, ws_bytes=need - 1) != 0 and b"workspace" in lib.wfl_last_error()
    assert lib.wfl_align_duration_prior(d, 141, 141, 0, None, None, None, None, None, None, d, 0, None, None, 0, 8, None, 0, d, d, d, d,
                                        None) == 0


# ------------------------------------------------------------------------------------------------ 3. the options
def test_option_rules_35_to_38_and_their_order():
    from wfl_asr_amd.options import DURATION_PRIOR_ERROR, PostOptions, resolve
    d = resolve({})
    assert d.duration_prior is None and d.duration_prior_weight == 1.0
    a = resolve({"align": "viterbi", "duration_prior": "durations.json"})
    assert a.duration_prior == "durations.json" and a.duration_prior_weight == 1.0 and a != resolve({"align": "viterbi"})
    b = resolve({"align": "viterbi", "duration_prior": "d.json", "duration_prior_weight": "0.5"})
    assert b.duration_prior_weight == 0.5 and type(b.duration_prior_weight) is float
    assert resolve({"align": "viterbi", "duration_prior": "d.json"}, duration_prior_weight=0).duration_prior_weight == 0.0
    assert resolve({"align": "viterbi", "duration_prior": "d.json"}, duration_prior="e.json").duration_prior == "e.json"    # the argument wins
    assert resolve({"align": "viterbi", "duration_prior": "d.json"}, duration_prior="").duration_prior is None             # an empty path: none
    with pytest.raises(ValueError, match="duration_prior needs align='viterbi'"):                                          # rule 35
        resolve({}, duration_prior="d.json")
    for bad in (-1, True, "much", float("nan"), float("inf")):                                                           # rule 36
        with pytest.raises(ValueError, match="duration_prior_weight must be a finite number >= 0"):
            resolve({"align": "viterbi", "duration_prior": "d.json"}, duration_prior_weight=bad)
    with pytest.raises(ValueError, match="duration_prior_weight needs a duration_prior"):                                 # rule 37
        resolve({"align": "viterbi"}, duration_prior_weight=1.0)
    beside = [dict(align_draft="drafts"), dict(min_duration=0.06), dict(optional_tokens=["a"]), dict(filler_token="<unk>"),
              dict(align_scores=True), dict(align_edits=True), dict(align_insertions=True)]
    for more in beside:                                                                                                  # rule 38
        with pytest.raises(ValueError) as e:
            resolve({"align": "viterbi", "duration_prior": "d.json"}, **more)
        assert str(e.value) == DURATION_PRIOR_ERROR, more
    # duration_scores, optional_scores and filler_scores need what rule 38 refuses, so an earlier rule speaks for them
    for more, match in ((dict(duration_scores=True), "duration_scores needs a min_duration"),
                        (dict(optional_scores=True), "optional_scores needs optional_tokens"),
                        (dict(filler_scores=True), "filler_scores needs a filler_token")):
        with pytest.raises(ValueError, match=match):
            resolve({"align": "viterbi", "duration_prior": "d.json"}, **more)
    for name in ("align_draft", "min_duration", "optional_tokens", "filler_token", "align_scores", "align_edits", "align_insertions",
                 "duration_scores", "optional_scores", "filler_scores"):
        assert name in DURATION_PRIOR_ERROR
    # the earlier rule is reported: 34 before 35, 35 before 36, 36 before 37
    with pytest.raises(ValueError, match="filler_scores needs a filler_token"):
        resolve({}, filler_scores=True, duration_prior="d.json")
    with pytest.raises(ValueError, match="duration_prior needs"):
        resolve({}, duration_prior="d.json", duration_prior_weight=-1)
    with pytest.raises(ValueError, match="duration_prior_weight must be"):
        resolve({"align": "viterbi"}, duration_prior_weight=-1)
    # the record
    assert isinstance(a, PostOptions) and len(a) == 8 and len(PostOptions._fields) == 8
    assert "duration_prior" in PostOptions._KEYWORD and "duration_prior_weight" in PostOptions._KEYWORD
    assert a._replace(duration_prior=None) == resolve({"align": "viterbi"}) and hash(a) != hash(resolve({"align": "viterbi"}))
    assert a._asdict()["duration_prior"] == "durations.json" and "duration_prior='durations.json'" in repr(a)
    assert PostOptions._make(tuple(a), duration_prior="x").duration_prior == "x" and resolve({}) == tuple(resolve({}))
    with pytest.raises(AttributeError):
        a.duration_prior = None


def test_the_option_is_refused_before_any_model_is_loaded(monkeypatch, tmp_path):
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import infer as I

    def no_load(*a, **k):
        raise AssertionError("a model was loaded before the options were refused")
    for f in (I.infer_audio, I.infer_folder, I.Labeler.label_files):
        for name in ("duration_prior", "duration_prior_weight"):
            assert inspect.signature(f).parameters[name].default is None
    monkeypatch.setattr(I, "_labeler", no_load)
    monkeypatch.setattr(I, "Labeler", no_load)
    with pytest.raises(ValueError, match="duration_prior needs align='viterbi'"):
        I.infer_audio("x.wav", duration_prior="d.json")
    with pytest.raises(ValueError, match="duration_prior cannot be combined"):
        I.infer_folder("some_folder", align="viterbi", min_duration=0.06, duration_prior="d.json")
    cfg = tmp_path / "config.yaml"
    cfg.write_text("postprocess:\n  align: viterbi\n  duration_prior: d.json\n  duration_prior_weight: -2\n")
    with pytest.raises(ValueError, match="duration_prior_weight must be"):                             # from the config file
        I.infer_audio("x.wav", config_path=str(cfg))
