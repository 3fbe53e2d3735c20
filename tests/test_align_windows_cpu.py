"""CPU (-m "not gpu"): the windowed forced alignment's definition (tests/viterbi_window_ref.py against enumeration of every legal path),
the host rule that predicts infeasibility, the draft -> windows mapping through the chunk clock, the option rules of
`postprocess.align_draft` / `postprocess.draft_tolerance`, and the null check of the windowed ABI entries."""
import ctypes
import inspect

import numpy as np
import pytest

import posterior_ref as P
import viterbi_ref as V
import viterbi_window_ref as W


# ------------------------------------------------------------------------------------------------ 1. the definition
def _tiny_cases(seed, n):
    """Seeded tiny cases, N <= 3 and T <= 6, with random windows: open, narrow, or any (lo, hi) in -1 .. T, lo > hi among them."""
    rng = np.random.default_rng(seed)
    C = 9
    for _ in range(n):
        N = int(rng.integers(0, 4))
        T = int(rng.integers(1, 7))
        alts = [[(1 + 2 * int(p), 2 + 2 * int(p)) for p in rng.choice(3, size=int(rng.integers(1, 3)), replace=False)] for _ in range(N)]
        gaps = [0] if rng.random() < 0.5 else [0, 7, 8]
        wins = []
        for _k in range(N):
            u = rng.random()
            if u < 0.3:
                wins.append(W.OPEN)
            elif u < 0.65:                                              # a narrow window somewhere
                lo = int(rng.integers(-1, T + 1))
                wins.append((lo, lo + int(rng.integers(0, 3))))
            else:
                wins.append((int(rng.integers(-1, T + 1)), int(rng.integers(-1, T + 1))))
        yield rng.standard_normal((T, C)), alts, gaps, wins


@pytest.fixture(scope="module")
def AL():
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import align
    return align


def test_windowed_dp_and_logz_equal_enumeration_and_the_host_rule_predicts_infeasibility(AL):
    feasible = infeasible = changed = reversed_windows = 0
    for seed in range(6):
        for z, alts, gaps, wins in _tiny_cases(seed, 50):
            T, N = len(z), len(alts)
            best, logz, n_paths = W.brute_force(z, alts, gaps, wins)
            path, score = W.viterbi(z, alts, gaps, wins)
            fb = W.forward_backward(z, alts, gaps, wins)
            reversed_windows += any(lo > hi for lo, hi in wins)
            # the host rule == "the DP found a path" == "the enumeration found a path"
            assert AL.windows_feasible(T, wins) == (path is not None) == (n_paths > 0) == (fb is not None), (T, N, wins)
            if path is None:
                infeasible += 1
                continue
            feasible += 1
            assert V.legal(path, N) and W.in_windows(path, wins)
            assert abs(score - best) < 1e-9
            assert abs(V.path_score(path, z, alts, gaps) - score) < 1e-9      # (the unmasked score of the windowed optimum)
            assert abs(fb["logz"] - logz) < 1e-9
            changed += abs(V.viterbi(z, alts, gaps)[1] - score) > 1e-9
    print(feasible, infeasible, changed, reversed_windows)
    assert feasible >= 60 and infeasible >= 60 and changed >= 20 and reversed_windows >= 20, "the cases do not cover the ground"


def test_open_windows_are_the_unwindowed_reference(AL):
    for seed in range(3):
        for z, alts, gaps, _ in _tiny_cases(100 + seed, 30):
            N = len(alts)
            path, score = V.viterbi(z, alts, gaps)
            wpath, wscore = W.viterbi(z, alts, gaps, [W.OPEN] * N)
            if path is None:
                assert wpath is None and not AL.windows_feasible(len(z), [W.OPEN] * N)
                continue
            assert (path == wpath).all() and score == wscore
            assert W.forward_backward(z, alts, gaps, [W.OPEN] * N)["logz"] == P.forward_backward(z, alts, gaps)["logz"]
    assert AL.OPEN_WINDOW == W.OPEN


def test_windowed_posteriors_stay_inside_the_windows():
    rng = np.random.default_rng(4)
    alts = [[(1, 2)], [(3, 4)], [(1, 2)]]
    z = rng.standard_normal((6, 9))
    wins = [(0, 1), (2, 2), (3, 5)]
    path, _ = W.viterbi(z, alts, [0], wins)
    tok = V.outputs(path, z, alts, 0)[1]
    fb = W.forward_backward(z, alts, [0], wins, tok=tok, want_gamma=True)
    t = np.arange(6)
    for k, (lo, hi) in enumerate(wins):
        assert fb["gB"][(t < lo) | (t > hi), k].sum() == 0 and abs(fb["gB"][:, k].sum() - 1) < 1e-12
    assert fb["start_sd"][1] == 0 and fb["start_mean"][1] == 0        # lo == hi: the start is known


# ------------------------------------------------------------------------------------------------ 2. a draft's windows
def test_draft_windows_go_through_the_chunk_clock(AL):
    # chunk 1 begins at 30.013 s (no multiple of 0.02) and at row 1500 of the file's rows
    frames, clock, fd = [1500, 250], [0.0, 30.013], 0.02
    draft = [(0.03, 0.1, "a"), (29.99, 30.0, "b"), (30.013, 30.1, "c"), (30.034, 30.2, "d"), (34.0, 34.5, "e"), (99.0, 99.5, "f")]
    pin = AL.draft_windows(draft, frames, clock, 0.0, fd)
    # 29.99 s is in chunk 0 (its last frame); 30.013 s is frame 0 of chunk 1 = row 1500, where 30.013 / 0.02 would say 1500.65;
    # 30.034 s is 1.05 frames into chunk 1 = row 1501, where the global division would say 1501.7
    assert pin == [(1, 1), (1499, 1499), (1500, 1500), (1501, 1501), (1500 + 199, 1500 + 199), (1749, 1749)]
    assert int(34.0 / fd) != 1500 + 199                                # (the global division is off the row)
    w = AL.draft_windows(draft, frames, clock, 0.06, fd)
    assert w == [(0, 4), (1496, 1502), (1497, 1503), (1498, 1504), (1696, 1702), (1746, 1749)]      # -+ 3 frames, clipped to 0 .. T - 1
    assert AL.draft_windows(draft[:1], frames, clock, 0.05, fd) == [(0, 4)]                         # ceil(2.5) = 3 frames
    assert AL.draft_windows([(-1.0, 0, "x")], frames, clock, 0.0, fd) == [(0, 0)]
    # a start the .lab truncated to just below its frame's boundary still lands on that frame
    assert AL.draft_windows([(int(0.06 * 1e7 - 1) / 1e7, 0, "x")], frames, clock, 0.0, fd) == [(3, 3)]
    with pytest.raises(ValueError):
        AL.draft_windows(draft, frames, clock[:1], 0.0, fd)


def test_windows_feasible_rule(AL):
    assert AL.windows_feasible(5, [])
    assert not AL.windows_feasible(5, [(2, 2), (2, 2)])                # two tokens pinned to one frame
    assert AL.windows_feasible(5, [(2, 2), (2, 3)])
    assert not AL.windows_feasible(5, [(3, 2)])                        # lo > hi
    assert not AL.windows_feasible(5, [(5, 9)])                        # at or beyond T
    assert not AL.windows_feasible(2, [W.OPEN] * 3)                    # fewer frames than tokens
    assert not AL.windows_feasible(9, [(4, 6), (0, 3)])                # cannot be met in order
    assert AL.windows_feasible(9, [(0, 8), (0, 1)])


def test_read_draft_is_the_shared_htk_reader(AL, tmp_path):
    from wfl_asr_amd import phonotactics as PH
    p = tmp_path / "x.lab"
    p.write_text("300000 700000 a\n\n700000 900000 SP\nnot a line\n900000 1200000 b\n")
    assert AL.read_draft(str(p)) == PH.read_lab(str(p)) == [(0.03, 0.07, "a"), (0.07, 0.09, "SP"), (0.09, 0.12, "b")]


def test_pack_windows(AL):
    N = np.array([2, 0, 1], np.int32)
    w = AL._pack_windows([[(1, 2), (3, 4)], None, None], N)
    assert w.dtype == np.int32 and w.tolist() == [[1, 2], [3, 4], list(AL.OPEN_WINDOW)]
    with pytest.raises(ValueError, match="2 tokens"):
        AL._pack_windows([[(1, 2)], None, None], N)
    with pytest.raises(ValueError, match="one entry per clip"):
        AL._pack_windows([None], N)
    with pytest.raises(ValueError, match="int32"):
        AL._pack_windows([[(0, 2 ** 31), (0, 1)], None, None], N)


# ------------------------------------------------------------------------------------------------ 3. the options
def test_option_rules_10_and_11():
    from wfl_asr_amd.options import DEFAULT_DRAFT_TOLERANCE, PostOptions, resolve
    d = resolve({})
    assert d.align_draft is None and d.draft_tolerance == DEFAULT_DRAFT_TOLERANCE == 0.1
    a = resolve({"align": "viterbi", "align_draft": "drafts"})
    assert a.align_draft == "drafts" and a.draft_tolerance == 0.1 and a != resolve({"align": "viterbi"})
    b = resolve({"align": "viterbi", "align_draft": "drafts", "draft_tolerance": 0}, draft_tolerance="0.25")
    assert b.draft_tolerance == 0.25 and type(b.draft_tolerance) is float
    assert resolve({"align": "viterbi", "align_draft": "drafts", "draft_tolerance": 0}).draft_tolerance == 0.0
    assert resolve({"align": "viterbi", "align_draft": "drafts"}, align_draft="").align_draft is None   # an empty path takes it away
    assert isinstance(a, PostOptions) and "align_draft='drafts'" in repr(a) and hash(a) != hash(resolve({"align": "viterbi"}))
    with pytest.raises(AttributeError):
        a.align_draft = "other"
    # the tuple's helpers carry the two fields, and a plain tuple of the eight equals only a record with the default draft fields
    c = a._replace(align_scores=True)
    assert c.align_draft == "drafts" and c.align_scores is True and a._replace(draft_tolerance=0.5).draft_tolerance == 0.5
    assert a._asdict()["align_draft"] == "drafts" and PostOptions._make(tuple(a), align_draft="x").align_draft == "x"
    assert d == tuple(d) and hash(d) == hash(tuple(d)) and a != tuple(a)
    with pytest.raises(ValueError, match="align_draft needs align='viterbi'"):                         # rule 10
        resolve({}, align_draft="drafts")
    with pytest.raises(ValueError, match="align_draft needs align='viterbi'"):
        resolve({"align_draft": "drafts", "align": "viterbi"}, align="greedy")
    for bad in (-0.1, float("nan"), True, "wide"):                                                       # rule 11
        with pytest.raises(ValueError, match="draft_tolerance must be a number >= 0"):
            resolve({"align": "viterbi", "align_draft": "drafts"}, draft_tolerance=bad)
    with pytest.raises(ValueError, match="draft_tolerance needs an align_draft"):
        resolve({"align": "viterbi"}, draft_tolerance=0.05)
    with pytest.raises(ValueError, match="draft_tolerance needs an align_draft"):
        resolve({"align": "viterbi", "draft_tolerance": 0.05})
    # the earlier rule is reported: 9 before 10, 10 before 11
    with pytest.raises(ValueError, match="bigram_scores needs"):
        resolve({}, bigram_scores=True, align_draft="drafts")
    with pytest.raises(ValueError, match="align_draft needs"):
        resolve({}, align_draft="drafts", draft_tolerance=-1)


def test_the_draft_options_are_refused_before_any_model_is_loaded(monkeypatch, tmp_path):
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import infer as I

    def no_load(*a, **k):
        raise AssertionError("a model was loaded before the options were refused")
    for f in (I.infer_audio, I.infer_folder, I.Labeler.label_files):
        for name in ("align_draft", "draft_tolerance"):
            assert inspect.signature(f).parameters[name].default is None
    monkeypatch.setattr(I, "_labeler", no_load)
    monkeypatch.setattr(I, "Labeler", no_load)
    with pytest.raises(ValueError, match="align_draft needs align='viterbi'"):
        I.infer_audio("x.wav", align_draft="drafts")
    with pytest.raises(ValueError, match="draft_tolerance needs an align_draft"):
        I.infer_folder("some_folder", align="viterbi", draft_tolerance=0.1)
    cfg = tmp_path / "config.yaml"
    cfg.write_text("postprocess:\n  align: greedy\n  align_draft: drafts\n")
    with pytest.raises(ValueError, match="align_draft needs align='viterbi'"):                         # from the config file
        I.infer_audio("x.wav", config_path=str(cfg))
    with pytest.raises(ValueError, match="draft_tolerance must be a number"):
        I._refuse_before_load(str(cfg), align="viterbi", draft_tolerance=-2)
    with pytest.raises(SystemExit) as e:
        I.main(["x.wav", "-ckpt", "m.pt", "-c", "c.yaml", "--draft-tolerance", "wide"])
    assert e.value.code == 2                       # click: not a number, before anything is loaded


def test_draft_moves_and_their_tsv():
    import __graft_entry__
    __graft_entry__.build()
    from wfl_asr_amd import infer as I
    tok = np.array([-1, 0, 0, 1, -1, 2, 2], np.int32)
    draft = [(0.01, 0.05, "a"), (0.05, 0.07, "b"), (0.13, 0.2, "a")]
    segs = [(0.03, 0.07, "a"), (0.07, 0.09, "b"), (0.11, 0.14, "a")]
    mv = I.draft_moves(draft, segs, tok, [(0, 1), (2, 4), (5, 6)])
    assert [m.on_edge for m in mv] == [True, False, True]
    assert [m.token for m in mv] == ["a", "b", "a"] and mv[2].move_s == pytest.approx(-0.02)
    lines = I.format_draft_moves_tsv([("x.wav", mv)]).split("\n")
    assert lines[0].startswith("# file\tindex\ttoken") and lines[1] == "x.wav\t0\ta\t100000\t300000\t+0.0200\t1"
    assert lines[2].endswith("\t0") and lines[3].endswith("\t1") and lines[4] == ""


# ------------------------------------------------------------------------------------------------ 4. ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import _lib
    return _lib.load()


def test_windowed_symbols_are_declared_and_exported(lib):
    import os
    from wfl_asr_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wfl_asr.h")).read()
    for name in ("wfl_align_windowed", "wfl_align_posterior_windowed"):
        assert name + "(" in src and name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    # wfl_align's arguments plus tok_win, after tok_cls
    assert len(_lib.SIGNATURES["wfl_align_windowed"][1]) == len(_lib.SIGNATURES["wfl_align"][1]) + 1
    assert len(_lib.SIGNATURES["wfl_align_posterior_windowed"][1]) == len(_lib.SIGNATURES["wfl_align_posterior"][1]) + 1


def test_a_null_tok_win_is_refused_on_the_host(lib):
    Pv = ctypes.c_void_p
    buf = (ctypes.c_char * 64)()
    d = ctypes.cast(buf, Pv)                       # never dereferenced: every call below fails on the host
    fo, ko = np.zeros(1, np.int64), np.zeros(1, np.int32)
    T, N, N0 = np.array([10], np.int32), np.array([3], np.int32), np.array([0], np.int32)
    h = lambda a: a.ctypes.data_as(Pv)             # noqa: E731
    need = lib.wfl_align_workspace_bytes(h(T), h(N), 1)
    pneed = lib.wfl_align_posterior_workspace_bytes(h(T), h(N), 1)

    def align(win, N_=N, ws_bytes=need, C=141):
        return lib.wfl_align_windowed(d, 141, C, 0, h(fo), h(T), h(ko), h(N_), d, win, d, 1, d, ws_bytes, d, d, d, d, None)

    def post(win, N_=N, ws_bytes=pneed):
        return lib.wfl_align_posterior_windowed(d, 141, 141, 0, h(fo), h(T), h(ko), h(N_), d, win, d, 1, d, d, ws_bytes, d, d, d, d, d,
                                                None)
    assert align(None) == -1 and b"wfl_align_windowed: null device" in lib.wfl_last_error()
    assert post(None) == -1 and b"wfl_align_posterior_windowed: null device" in lib.wfl_last_error()
    # the other checks are wfl_align's own, under the new names
    assert align(d, C=0) != 0 and b"wfl_align_windowed: C must" in lib.wfl_last_error()
    assert align(d, ws_bytes=need - 1) != 0 and b"workspace" in lib.wfl_last_error()
    assert post(d, ws_bytes=pneed - 1) != 0 and b"workspace" in lib.wfl_last_error()
    assert lib.wfl_align_windowed(d, 141, 141, 0, None, None, None, None, None, None, d, 0, None, 0, d, d, d, d, None) == 0   # no clip
