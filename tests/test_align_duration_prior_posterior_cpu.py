"""CPU (-m "not gpu"): the definition of the posteriors over the explicit-duration lattice (tests/duration_prior_posterior_ref.py
against the enumeration of every segmentation), its two special cases (no prior: posterior_ref; a hard table: duration_posterior_ref),
the ABI entry's host-side checks and workspace formula, the rows and formatters of the report, and the option rules of
`postprocess.duration_prior_scores`."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import duration_posterior_ref as DPR
import duration_prior_posterior_ref as R
import posterior_ref as P
import viterbi_duration_prior_ref as DP
import viterbi_min_ref as M

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


def _tok(states):
    s = np.asarray(states)
    return np.where(s % 3 == 0, -1, s // 3)


# ------------------------------------------------------------------------------------------------ 1. the definition
def test_the_sums_equal_the_enumeration_of_all_segmentations():
    """T <= 9, N <= 3, D in 1 .. 4: logZ, start, end and occ, with -inf entries, -inf tails, rows of -1 and windows; a lattice without
    a path is None in both."""
    rng = np.random.default_rng(401)
    C = 9
    cases = finite = none = windowed = tails = norow = 0
    worst = 0.0
    by_d = set()
    while cases < 260:
        T, N, D = int(rng.integers(1, 10)), int(rng.integers(0, 4)), int(rng.integers(1, 5))
        alts = [[(1 + 2 * k, 2 + 2 * k)] for k in range(N)]
        z = rng.standard_normal((T, C))
        table = _table(3, D, rng)
        rows = [int(r) for r in rng.integers(-1, 3, N)]
        wins = None
        if N and rng.random() < 0.3:
            wins = [(int(lo), int(lo) + int(rng.integers(0, 4))) for lo in rng.integers(0, T, N)]
            windowed += 1
        want = R.enumerate_segmentations(z, alts, [0, 7], rows, table, wins)
        got = R.forward_backward(z, alts, [0, 7], rows, table, windows=wins, full=True)
        cases += 1
        assert (want is None) == (got is None), (T, N, D, rows, table, wins)
        if want is None:
            none += 1
            continue
        finite += 1
        by_d.add(D)
        norow += int(-1 in rows)
        tails += int(N > 0 and T > D + N)
        for k in ("start", "end", "occ"):
            worst = max(worst, float(np.abs(want[k] - got[k]).max()) if N else 0.0)
        worst = max(worst, abs(want["logz"] - got["logz"]))
        if N:                                                             # a path opens and ends every token on exactly one frame
            assert np.allclose(got["start"].sum(axis=0), 1.0, atol=1e-12) and np.allclose(got["end"].sum(axis=0), 1.0, atol=1e-12)
            # the kernel's route to occ: starts so far minus ends before
            cum = np.cumsum(got["start"], axis=0) - np.concatenate([np.zeros((1, N)), np.cumsum(got["end"], axis=0)[:-1]])
            worst = max(worst, float(np.abs(cum - got["occ"]).max()))
    print(cases, finite, none, windowed, tails, norow, sorted(by_d), worst)
    assert worst < 1e-12
    assert finite > 80 and none > 20 and windowed > 30 and tails > 20 and norow > 40 and by_d == {1, 2, 3, 4}


def test_the_float32_restatement_stays_close_and_the_moments_follow_the_gammas():
    rng = np.random.default_rng(402)
    T, N, D, C = 70, 9, 4, 25
    alts = [[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 12, N)]
    z = rng.standard_normal((T, C)) * 2
    table = rng.uniform(-4, 0, (5, D + 1))
    table[1, :2] = NEG
    rows = [int(r) for r in rng.integers(-1, 5, N)]
    states, _, _ = DP.viterbi(z, alts, [0, C - 1], rows, table)
    tok = _tok(states)
    a = R.forward_backward(z, alts, [0, C - 1], rows, table, tok=tok, full=True)
    b = R.forward_backward(z, alts, [0, C - 1], rows, table, tok=tok, dtype=np.float32, renorm=16)
    assert abs(a["logz"] - b["logz"]) < 1e-3
    for k in R.OUTPUTS[1:]:
        assert np.abs(a[k] - b[k]).max() < 2e-3, k
    first = np.array([np.nonzero(tok == k)[0][0] for k in range(N)])
    last = np.array([np.nonzero(tok == k)[0][-1] for k in range(N)])
    t = np.arange(T)[:, None]
    assert np.allclose(a["start_mean"], (a["start"] * (t - first)).sum(axis=0), atol=1e-9)
    assert np.allclose(a["end_mean"], (a["end"] * (t - last)).sum(axis=0), atol=1e-9)
    # the expected length is frames + end_mean - start_mean: the sum of occ over the clip, by linearity
    assert np.allclose(a["occ"].sum(axis=0), (last - first + 1) + a["end_mean"] - a["start_mean"], atol=1e-9)
    assert ((a["tok_post"] >= 0) & (a["tok_post"] <= 1)).all()
    s = R.seven(z, alts, [0, C - 1], rows, table, tok)
    assert s[6] == 0 and len(s) == 7 and s[0] == a["logz"]
    assert R.seven(z[:3], alts, [0, C - 1], rows, table, tok[:3])[6] == 1


def test_without_a_prior_it_is_the_plain_forward_backward():
    rng = np.random.default_rng(403)
    for T, N, D in ((1, 0, 2), (1, 1, 1), (9, 3, 2), (40, 12, 3), (40, 40, 4)):
        alts = [[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 9, N)]
        z = rng.standard_normal((T, 20))
        path, _ = P.V.viterbi(z, alts, [0, 19])
        tok = _tok(path)
        want = P.forward_backward(z, alts, [0, 19], tok=tok, want_gamma=True)
        got = R.forward_backward(z, alts, [0, 19], [-1] * N, _table(2, D, rng), tok=tok, full=True)
        assert abs(want["logz"] - got["logz"]) < 1e-10
        if N:
            assert np.abs(want["gB"] - got["start"]).max() < 1e-10 and np.abs(want["gB"] + want["gI"] - got["occ"]).max() < 1e-10
            for k in ("tok_post", "start_mean", "start_sd"):
                assert np.abs(want[k] - got[k]).max() < 1e-9, k
    assert R.forward_backward(rng.standard_normal((2, 20)), [[(1, 2)]] * 3, [0], [-1] * 3, np.zeros((1, 2))) is None


def test_a_hard_table_is_the_minimum_duration_forward_backward():
    """L(d) = -inf below m, 0 from m on, tail 0."""
    rng = np.random.default_rng(404)
    table = np.zeros((8, 9))
    for d in range(1, 9):
        table[d - 1, :d - 1] = NEG
    seen = 0
    for T, N in ((12, 2), (30, 5), (60, 9)):
        alts = [[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 9, N)]
        z = rng.standard_normal((T, 20))
        D = rng.choice([1, 2, 3, 8], N)
        path, _ = M.viterbi(z, alts, [0, 19], D)
        if path is None:
            assert R.forward_backward(z, alts, [0, 19], (D - 1).tolist(), table) is None
            continue
        tok = _tok(path)
        want = DPR.forward_backward(z, alts, [0, 19], D, tok=tok)
        got = R.forward_backward(z, alts, [0, 19], (D - 1).tolist(), table, tok=tok)
        assert abs(want["logz"] - got["logz"]) < 1e-10
        for k in ("tok_post", "start_mean", "start_sd"):
            assert np.abs(want[k] - got[k]).max() < 1e-9, k
        seen += 1
    assert seen >= 2


# ------------------------------------------------------------------------------------------------ 2. the host side
def _cfg(N):
    """(slots, LDS room for the rings in bytes, words of the sums kept in the workspace) of the configuration that holds N tokens."""
    c = 0 if N <= 127 else 1 if N <= 511 else 2 if N <= 1023 else 3 if N <= 2047 else 4
    slots = (128, 512, 1024, 2048, 4608)[c]
    return slots, (148992, 112128, 99840, 75264, 9728)[c], 16 * slots if c >= 3 else 0


def _lds_rings(N, D):
    slots, room, _ = _cfg(N)
    return min(2, room // (4 * slots * D))


def _formula_words(T, N, D):
    """The header's per-clip workspace formula (include/wfl_asr.h, wfl_align_duration_prior_posterior)."""
    if T == 0:
        return 0
    r64 = lambda x: (x + 63) // 64 * 64            # noqa: E731
    slots, _, sums = _cfg(N)
    nblk = (T + 127) // 128
    return r64(T) + r64(2 * nblk) + nblk * (3 + D) * slots + 256 * slots + sums + (2 - _lds_rings(N, D)) * r64(slots * D)


def test_the_abi_entry_checks_its_arguments_and_sizes_its_workspace(AL):
    from wfl_asr_amd import _lib
    lib = _lib.load()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wfl_asr.h")).read()
    assert "wfl_align_duration_prior_posterior(" in src and hasattr(ctypes.CDLL(_lib.LIB_PATH), "wfl_align_duration_prior_posterior")
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "wfl_align_duration_prior_posterior_workspace_bytes")
    # the search's arguments without its four outputs, plus tok and the seven outputs
    assert len(_lib.SIGNATURES["wfl_align_duration_prior_posterior"][1]) == len(_lib.SIGNATURES["wfl_align_duration_prior"][1]) + 4
    assert AL._ENTRIES["wfl_align_duration_prior_posterior"] == ("wfl_align_duration_prior_posterior", True, False)
    Pv = ctypes.c_void_p
    buf = (ctypes.c_char * 64)()
    d = ctypes.cast(buf, Pv)                       # never dereferenced: every call below fails on the host
    fo, ko = np.zeros(1, np.int64), np.zeros(1, np.int32)
    T, N = np.array([10], np.int32), np.array([3], np.int32)
    h = lambda a: a.ctypes.data_as(Pv)             # noqa: E731
    ws = lib.wfl_align_duration_prior_posterior_workspace_bytes
    need = ws(h(T), h(N), 1, 8)
    assert need == 4 * _formula_words(10, 3, 8) > 0
    assert ws(h(T), h(N), 1, 0) == -1 and ws(h(T), h(N), 1, 33) == -1
    assert ws(h(np.array([-1], np.int32)), h(N), 1, 8) == -1
    assert AL.duration_prior_posterior_workspace_bytes([10], [3], 8) == need
    with pytest.raises(_lib.WflError):
        AL.duration_prior_posterior_workspace_bytes([10], [3], 33)
    # the formula, at every D and on both sides of every threshold at which a ring leaves LDS (per configuration: N <= 511 at D = 27 | 28,
    # N <= 1023 at 12 | 13 and 24 | 25, N <= 2047 at 4 | 5 and 9 | 10; N <= 127 keeps both at every D, N > 2047 none)
    for n_tok in (0, 3, 127, 128, 511, 512, 1023, 1024, 2047, 2048, 4096, 5000):
        for D in range(1, 33):
            for n_fr in (0, 1, 128, 129, 3000):
                got = ws(h(np.array([n_fr], np.int32)), h(np.array([n_tok], np.int32)), 1, D)
                assert got == 4 * _formula_words(n_fr, n_tok, D), (n_tok, D, n_fr)
    assert [_lds_rings(100, D) for D in (1, 32)] == [2, 2]
    assert [_lds_rings(300, D) for D in (27, 28, 32)] == [2, 1, 1]
    assert [_lds_rings(700, D) for D in (12, 13, 24, 25)] == [2, 1, 1, 0]
    assert [_lds_rings(1500, D) for D in (4, 5, 9, 10)] == [2, 1, 1, 0]
    assert [_lds_rings(2500, D) for D in (1, 32)] == [0, 0]
    batch_t, batch_n = np.array([3000, 0, 700, 2], np.int32), np.array([600, 5, 2048, 3], np.int32)
    assert ws(h(batch_t), h(batch_n), 4, 9) == 4 * sum(_formula_words(int(t), int(n), 9) for t, n in zip(batch_t, batch_n))

    def post(win=None, dur_rows=d, table=d, n_rows=4, D=8, ws_bytes=need, C=141, tok=d, out=(d, d, d, d, d, d, d)):
        return lib.wfl_align_duration_prior_posterior(d, 141, C, 0, h(fo), h(T), h(ko), h(N), d, win, d, 1, dur_rows, table, n_rows, D,
                                                      tok, d, ws_bytes, *out, None)
    fn = b"wfl_align_duration_prior_posterior: "
    for win in (None, d):                          # tok_win is nullable
        assert post(win, dur_rows=None) == -1 and fn + b"null tok_dur" in lib.wfl_last_error()
        assert post(win, table=None) == -1 and b"null dur" in lib.wfl_last_error()
        assert post(win, n_rows=-1) == -1 and b"n_rows" in lib.wfl_last_error()
        for D in (0, 33, -1):
            assert post(win, D=D) == -1 and b"D must be 1 .. 32" in lib.wfl_last_error()
        assert post(win, C=0) != 0 and fn + b"C must" in lib.wfl_last_error()
        assert post(win, ws_bytes=need - 1) != 0 and b"workspace" in lib.wfl_last_error()
        assert post(win, tok=None) == -1 and b"null device pointer" in lib.wfl_last_error()
        for miss in range(7):                      # logz, the five per-token outputs, status
            out = tuple(None if i == miss else d for i in range(7))
            assert post(win, out=out) == -1 and b"null device pointer" in lib.wfl_last_error(), miss
    assert lib.wfl_align_duration_prior_posterior(d, 141, 141, 0, None, None, None, None, None, None, d, 0, None, None, 0, 8, None, None, 0,
                                                  d, d, d, d, d, d, d, None) == 0
    sig = inspect.signature(AL.duration_prior_posteriors).parameters
    assert list(sig)[:8] == ["logits", "n_frames", "token_classes", "gap_classes", "o_id", "tok_rows", "table", "tok"]
    assert all(sig[k].default is None for k in ("frame_offsets", "stream", "packed", "windows"))


def test_the_rows_and_the_formatters(AL):
    from wfl_asr_amd import reports as RP
    toks = [AL.TokenScore("a", 0.0, 0.06, 0.9, 0.01, 0.0), AL.TokenScore("SP", 0.06, 0.08, 0.5, 0.0, 0.0),
            AL.TokenScore("b", 0.08, 0.2, 0.7, 0.02, -0.01)]
    table = np.array([[-1.0, -2.0, -0.5], [NEG, -3.0, NEG]])
    rows = AL.token_durations(toks, [3, 1, 6], [0, -1, 1], table, [0.9, 0.5, 0.7], [0.5, 0.0, -1.0], [1.0, 0.0, 2.0], [0.25, 0.0, 1.0],
                              [0.5, 0.0, 0.0], 0.02)
    assert [r.index for r in rows] == [0, 1, 2] and [r.token for r in rows] == ["a", "SP", "b"] and [r.frames for r in rows] == [3, 1, 6]
    assert rows[0].log_prior == pytest.approx(-2.0 + (3 - 2) * -0.5) and rows[1].log_prior is None and rows[2].log_prior == NEG
    assert AL.token_durations(toks[:1], [2], [0], table, [1], [0], [0], [0], [0], 0.02)[0].log_prior == -2.0
    assert rows[0].expected_frames == pytest.approx(3 + 0.25 - 0.5) and rows[2].expected_frames == pytest.approx(6 + 1.0 + 1.0)
    assert rows[0].start_shift_s == pytest.approx(0.01) and rows[0].start_sd_s == pytest.approx(0.02)
    assert rows[0].end_shift_s == pytest.approx(0.005) and rows[0].end_sd_s == pytest.approx(0.01)
    with pytest.raises(ValueError, match="one token"):
        AL.token_durations(toks, [3, 1], [0, -1, 1], table, [0.9, 0.5, 0.7], [0] * 3, [0] * 3, [0] * 3, [0] * 3, 0.02)
    head = ["index", "token", "start_s", "end_s", "frames", "log_prior", "posterior", "start_shift_s", "start_sd_s", "end_shift_s",
            "end_sd_s", "expected_frames"]
    assert RP.REPORTS["durations"].header.split("\t") == head and AL.TokenDuration._fields == tuple(head)
    lines = RP.file_text("durations", rows).split("\n")
    assert lines[0].split("\t") == head and len(lines) == 5 and lines[-1] == ""
    assert lines[1].split("\t") == ["0", "a", "0.0000000", "0.0600000", "3", "-2.500000", "0.900000", "0.0100000", "0.0200000",
                                    "0.0050000", "0.0100000", "2.7500"]
    assert lines[2].split("\t")[5] == "none" and lines[3].split("\t")[5] == "-inf"
    assert RP.file_text("durations", []) == "\t".join(head) + "\n"
    other = AL.token_durations(toks[:1], [1], [0], table, [0.4], [0], [0], [0], [0], 0.02)
    folder = RP.folder_text("durations", [("x.wav", rows), ("y.wav", other)]).split("\n")
    assert folder[0] == "file\t" + "\t".join(head) and len(folder) == 5            # the token without a row is left out
    assert [ln.split("\t")[0] for ln in folder[1:4]] == ["x.wav", "x.wav", "y.wav"]
    assert [float(ln.split("\t")[6]) for ln in folder[1:4]] == [NEG, -2.5, -1.0]   # the lowest log_prior first


# ------------------------------------------------------------------------------------------------ 3. the options
def test_option_rules_40_and_41_and_their_order():
    from wfl_asr_amd import options as O
    from wfl_asr_amd.options import DURATION_PRIOR_ERROR, DURATION_PRIOR_SCORES_ERROR, PostOptions, resolve
    base = {"align": "viterbi", "duration_prior": "d.json"}
    assert resolve({}).duration_prior_scores is False and resolve(base).duration_prior_scores is False
    a = resolve(base, duration_prior_scores=True)
    assert a.duration_prior_scores is True and a.scored and not resolve(base).scored
    assert resolve({**base, "duration_prior_scores": True}) == a                                       # from the config
    assert resolve({**base, "duration_prior_scores": True}, duration_prior_scores=False) == resolve(base)      # the argument wins
    for bad in (1, 0, "yes", "true", 1.0):                                                             # rule 40
        with pytest.raises(ValueError, match="duration_prior_scores must be true or false"):
            resolve(base, duration_prior_scores=bad)
    with pytest.raises(ValueError) as e:                                                               # rule 41
        resolve({"align": "viterbi"}, duration_prior_scores=True)
    assert str(e.value) == DURATION_PRIOR_SCORES_ERROR and "align_scores" in DURATION_PRIOR_SCORES_ERROR
    with pytest.raises(ValueError, match="duration_prior_scores needs a duration_prior"):
        resolve({}, duration_prior_scores=True)
    # 40 before 41; the earlier rules before both: 35, 37 and 38 are reported first
    with pytest.raises(ValueError, match="must be true or false"):
        resolve({"align": "viterbi"}, duration_prior_scores="yes")
    with pytest.raises(ValueError, match="duration_prior needs align='viterbi'"):
        resolve({}, duration_prior="d.json", duration_prior_scores=True)
    with pytest.raises(ValueError, match="duration_prior_weight needs a duration_prior"):
        resolve({"align": "viterbi"}, duration_prior_weight=1.0, duration_prior_scores=True)
    # the other scorers stay refused beside a prior, with the message byte for byte
    for more in (dict(align_scores=True), dict(align_edits=True), dict(align_insertions=True)):
        with pytest.raises(ValueError) as e:
            resolve(base, duration_prior_scores=True, **more)
        assert str(e.value) == DURATION_PRIOR_ERROR
    assert DURATION_PRIOR_ERROR == ("duration_prior cannot be combined with align_draft, min_duration, optional_tokens, filler_token, "
                                    "align_scores, align_edits, align_insertions, duration_scores, optional_scores or filler_scores: "
                                    "their lattices carry no duration term, and a search or a score must speak of one lattice; drop "
                                    "postprocess.duration_prior (--duration-prior) for that run")
    assert "duration_prior_scores" in O.__doc__ and " 40. " in O.__doc__ and " 41. " in O.__doc__
    # the record
    plain = resolve(base)
    assert isinstance(a, PostOptions) and len(a) == 8 and len(PostOptions._fields) == 8
    assert PostOptions._KEYWORD[-4:] == ("duration_prior_scores", "optional_scores", "filler_token", "filler_penalty")
    assert len(PostOptions._KEYWORD) == len(PostOptions._KEYWORD_DEFAULTS)
    assert a != plain and hash(a) != hash(plain) and a._replace(duration_prior_scores=False) == plain
    assert plain._replace(duration_prior_scores=True) == a and a._asdict()["duration_prior_scores"] is True
    assert "duration_prior_scores=True" in repr(a) and "duration_prior_scores=False" in repr(plain)
    assert PostOptions._make(tuple(a), duration_prior_scores=True).duration_prior_scores is True
    assert PostOptions(*tuple(a)).duration_prior_scores is False and resolve({}) == tuple(resolve({}))
    with pytest.raises(AttributeError):
        a.duration_prior_scores = False
    assert list(inspect.signature(resolve).parameters)[-2:] == ["duration_prior_weight", "duration_prior_scores"]


def test_the_option_is_refused_before_any_model_is_loaded(monkeypatch, tmp_path):
    from wfl_asr_amd import reports as RP
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import infer as I

    def no_load(*a, **k):
        raise AssertionError("a model was loaded before the options were refused")
    for f in (I.infer_audio, I.infer_folder, I.Labeler.label_files):
        names = list(inspect.signature(f).parameters)
        assert inspect.signature(f).parameters["duration_prior_scores"].default is None
        assert names[names.index("duration_prior_weight") + 1] == "duration_prior_scores" and names[-1] == "bigram_scores"
    monkeypatch.setattr(I, "_labeler", no_load)
    monkeypatch.setattr(I, "Labeler", no_load)
    with pytest.raises(ValueError, match="duration_prior_scores needs a duration_prior"):
        I.infer_audio("x.wav", align="viterbi", duration_prior_scores=True)
    with pytest.raises(ValueError, match="duration_prior_scores must be true or false"):
        I.infer_folder("some_folder", align="viterbi", duration_prior="d.json", duration_prior_scores="yes")
    cfg = tmp_path / "config.yaml"
    cfg.write_text("postprocess:\n  align: viterbi\n  duration_prior_scores: true\n")
    with pytest.raises(ValueError, match="duration_prior_scores needs a duration_prior"):              # from the config file
        I.infer_audio("x.wav", config_path=str(cfg))
    assert RP.file_path("durations", "out/x.lab") == os.path.join("out", "x.durations.tsv")
    assert "wfl_align_posterior" in I.DURATION_PRIOR_SCORES_PLAIN
