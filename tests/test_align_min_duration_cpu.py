"""CPU (-m "not gpu"): the definition of the forced alignment with minimum durations (tests/viterbi_min_ref.py against the enumeration
of every legal path), the host rule that predicts infeasibility, `min_frames_for`, the option rules of `postprocess.min_duration`,
the packing, and the ABI entry's null check."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest

import viterbi_min_ref as M
import viterbi_ref as V
import viterbi_window_ref as W


@pytest.fixture(scope="module")
def AL():
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import align
    return align


def _window_sets(T, N, rng):
    """Open windows, then two random sets: narrow ones and any (lo, hi) in -1 .. T."""
    yield [W.OPEN] * N
    for _ in range(2):
        wins = []
        for _k in range(N):
            lo = int(rng.integers(-1, T + 1))
            wins.append((lo, lo + int(rng.integers(0, 3))) if rng.random() < 0.6 else (lo, int(rng.integers(-1, T + 1))))
        yield wins


# ------------------------------------------------------------------------------------------------ 1. the definition
def test_dp_equals_enumeration_and_the_host_rule_predicts_infeasibility(AL):
    """Every T <= 7, N <= 2, D <= 3, with and without windows."""
    rng = np.random.default_rng(71)
    C = 9
    feasible = infeasible = constrained = 0
    for T, N in itertools.product(range(1, 8), range(0, 3)):
        alts = [[(1 + 2 * k, 2 + 2 * k)] for k in range(N)]
        for D in itertools.product((1, 2, 3), repeat=N):
            z = rng.standard_normal((T, C))
            for wi, wins in enumerate(_window_sets(T, N, rng)):
                best, n_paths = M.brute_force(z, alts, [0, 7], wins, D)
                path, score = M.viterbi(z, alts, [0, 7], D, windows=wins if wi else None)
                assert AL.windows_feasible(T, wins, D) == (path is not None) == (n_paths > 0), (T, N, D, wins)
                if path is None:
                    infeasible += 1
                    assert score == 0.0
                    continue
                feasible += 1
                assert V.legal(path, N) and W.in_windows(path, wins) and (M.run_lengths(path, N) >= np.array(D)).all()
                assert abs(score - best) < 1e-9 and abs(V.path_score(path, z, alts, [0, 7]) - best) < 1e-9
                constrained += V.viterbi(z, alts, [0, 7])[1] > best + 1e-9
    print(feasible, infeasible, constrained)
    assert feasible > 80 and infeasible > 80 and constrained > 20         # (the cases cover both, and durations that change the optimum)


def test_all_ones_is_the_unconstrained_dp_exactly():
    rng = np.random.default_rng(72)
    for T, N in ((1, 0), (1, 1), (9, 3), (40, 12), (40, 40)):
        alts = [[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 9, N)]
        z = rng.standard_normal((T, 20))
        a, sa = V.viterbi(z, alts, [0, 19])
        b, sb = M.viterbi(z, alts, [0, 19], [1] * N)
        assert (a == b).all() and sa == sb
    assert M.viterbi(rng.standard_normal((2, 20)), [[(1, 2)]] * 3, [0], [1] * 3) == (None, 0.0)


def test_the_chain_is_walked_back_to_b(AL):
    """One token with D = 8 in 10 frames: B, then I to the end, wherever the logits would rather have a gap."""
    z = np.zeros((10, 5))
    z[:, 0] = 3.0                                                         # the gap class wins every frame ...
    z[4, 1] = 9.0                                                         # ... but the token opens best at frame 4: too late for 8 frames
    path, _ = M.viterbi(z, [[(1, 2)]], [0], [8])
    assert M.run_lengths(path, 1)[0] >= 8 and V.legal(path, 1)
    assert [int(s) for s in path].count(1) == 1
    assert not AL.windows_feasible(10, [(4, 4)], [8]) and AL.windows_feasible(10, [(2, 2)], [8])


# ------------------------------------------------------------------------------------------------ 2. the host side
def test_windows_feasible_with_durations(AL):
    assert AL.windows_feasible(5, [], [])
    assert AL.windows_feasible(6, [W.OPEN] * 2, [3, 3]) and not AL.windows_feasible(5, [W.OPEN] * 2, [3, 3])     # sum D > T
    assert not AL.windows_feasible(20, [(0, 5), (6, 7)], [8, 1])         # the window is narrower than the durations force
    assert AL.windows_feasible(20, [(0, 5), (6, 8)], [8, 1])
    assert not AL.windows_feasible(20, [(0, 5), (13, 19)], [8, 8]) and AL.windows_feasible(21, [(0, 5), (13, 19)], [8, 8])
    # the default keeps the rule without durations
    for T, w in ((5, [(2, 2), (2, 2)]), (5, [(2, 2), (2, 3)]), (2, [W.OPEN] * 3), (9, [(0, 8), (0, 1)]), (5, [(5, 9)])):
        assert AL.windows_feasible(T, w) == AL.windows_feasible(T, w, [1] * len(w)) == AL.windows_feasible(T, w, None)
    with pytest.raises(ValueError, match="one minimum duration per window"):
        AL.windows_feasible(5, [W.OPEN], [1, 1])


def test_min_frames_for(AL):
    fd = 0.02
    tr = ["a", "SP", "b", "a"]
    assert AL.min_frames_for(tr, 0.06, fd) == [3, 3, 3, 3]               # 0.06 / 0.02 = 3.0000000000000004 in floats: 3, not 4
    assert AL.min_frames_for(tr, 0.061, fd) == [4] * 4 and AL.min_frames_for(tr, 0.05, fd) == [3] * 4
    assert AL.min_frames_for(tr, 0, fd) == [1] * 4 and AL.min_frames_for(tr, 0.019, fd) == [1] * 4
    assert AL.min_frames_for(tr, 0.16, fd) == [8] * 4 and AL.min_frames_for([], 0.1, fd) == []
    assert AL.min_frames_for(tr, {"a": 0.1, "default": 0.04}, fd) == [5, 2, 2, 5]
    assert AL.min_frames_for(tr, {"a": 0.1}, fd) == [5, 1, 1, 5]          # no default: the others stay free
    assert AL.min_frames_for(tr, {"zz": 0.1, "b": 0.03}, fd) == [1, 1, 2, 1]      # a name the transcript lacks constrains nothing
    assert AL.min_frames_for(tr, (("a", 0.1), ("default", 0.04)), fd) == [5, 2, 2, 5]     # the form PostOptions carries
    assert all(type(x) is int for x in AL.min_frames_for(tr, 0.06, fd))
    with pytest.raises(ValueError, match="more than the 8"):
        AL.min_frames_for(tr, 0.17, fd)
    with pytest.raises(ValueError, match="more than the 8"):
        AL.min_frames_for(tr, {"b": 0.2}, fd)
    assert AL.MAX_MIN_FRAMES == M.MAX_MIN_FRAMES == 8


def test_pack_min_frames(AL):
    N = np.array([2, 0, 1], np.int32)
    d = AL._pack_min_frames([[3, 8], None, None], N)
    assert d.dtype == np.int32 and d.tolist() == [3, 8, 1]
    assert AL._pack_min_frames([None, None, [9]], N).tolist() == [1, 1, 9]          # (out of range: the kernel's status 4, not the packing's)
    assert AL._pack_min_frames([], np.zeros(0, np.int32)).tolist() == [1]
    with pytest.raises(ValueError, match="2 tokens"):
        AL._pack_min_frames([[3], None, None], N)
    with pytest.raises(ValueError, match="one entry per clip"):
        AL._pack_min_frames([None], N)
    for bad in ([2.0, 1], [True, 1], ["2", 1]):
        with pytest.raises(ValueError, match="ints"):
            AL._pack_min_frames([bad, None, None], N)
    with pytest.raises(ValueError, match="int32"):
        AL._pack_min_frames([[2 ** 31, 1], None, None], N)
    assert AL.PackedClips._fields[-2:] == ("d_win", "d_min") and AL.PackedClips._field_defaults["d_min"] is None
    for f in (AL.pack_clips, AL.viterbi_align):
        assert inspect.signature(f).parameters["min_frames"].default is None
    assert "min_frames" not in inspect.signature(AL.alignment_posteriors).parameters


def test_the_scoring_entries_refuse_a_batch_packed_with_durations(AL):
    packed = AL.PackedClips(0, None, None, None, None, None, None, None, d_min=object())
    for name in ("alignment_posteriors", "edit_scores", "insertion_scores"):
        with pytest.raises(ValueError, match=name + " scores the lattice without minimum durations"):
            AL._without_min_frames(packed, name)
    assert len(AL._without_min_frames(AL.PackedClips(0, 1, 2, 3, 4, 5, 6), "x")) == 8


def test_the_abi_entry_checks_its_pointers(AL):
    import os
    from wfl_asr_amd import _lib
    lib = _lib.load()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wfl_asr.h")).read()
    assert "wfl_align_min_duration(" in src and hasattr(ctypes.CDLL(_lib.LIB_PATH), "wfl_align_min_duration")
    assert len(_lib.SIGNATURES["wfl_align_min_duration"][1]) == len(_lib.SIGNATURES["wfl_align_windowed"][1]) + 1
    Pv = ctypes.c_void_p
    buf = (ctypes.c_char * 64)()
    d = ctypes.cast(buf, Pv)                       # never dereferenced: every call below fails on the host
    fo, ko = np.zeros(1, np.int64), np.zeros(1, np.int32)
    T, N = np.array([10], np.int32), np.array([3], np.int32)
    h = lambda a: a.ctypes.data_as(Pv)             # noqa: E731
    need = lib.wfl_align_workspace_bytes(h(T), h(N), 1)

    def align(win, dmin, ws_bytes=need, C=141):
        return lib.wfl_align_min_duration(d, 141, C, 0, h(fo), h(T), h(ko), h(N), d, win, dmin, d, 1, d, ws_bytes, d, d, d, d, None)
    for win in (None, d):                          # tok_win is nullable, tok_min is not
        assert align(win, None) == -1 and b"wfl_align_min_duration: null device" in lib.wfl_last_error()
        assert align(win, d, C=0) != 0 and b"wfl_align_min_duration: C must" in lib.wfl_last_error()
        assert align(win, d, ws_bytes=need - 1) != 0 and b"workspace" in lib.wfl_last_error()
    assert lib.wfl_align_min_duration(d, 141, 141, 0, None, None, None, None, None, None, None, d, 0, None, 0, d, d, d, d, None) == 0


# ------------------------------------------------------------------------------------------------ 3. the options
def test_option_rules_14_to_16_and_their_order():
    from wfl_asr_amd.options import MIN_DURATION_SCORES_ERROR, PostOptions, parse_min_duration, resolve
    d = resolve({})
    assert d.min_duration is None and resolve({"align": "viterbi", "min_duration": {}}).min_duration is None
    a = resolve({"align": "viterbi", "min_duration": 0.06})
    assert a.min_duration == 0.06 and type(a.min_duration) is float
    b = resolve({"align": "viterbi", "min_duration": {"default": 0.04, "a": "0.1", "SP": 0}})
    assert b.min_duration == (("SP", 0.0), ("a", 0.1), ("default", 0.04))
    assert resolve({"align": "viterbi", "min_duration": 0.06}, min_duration={"a": 0.1}).min_duration == (("a", 0.1),)    # the argument wins
    assert resolve({"align": "viterbi"}, min_duration=b.min_duration) == b                  # the normalised form is taken back
    assert resolve({"align": "viterbi", "min_duration": 0.16}).min_duration == 0.16         # the cap itself is allowed
    assert resolve({"align": "viterbi", "align_draft": "drafts", "min_duration": 0.06}).align_draft == "drafts"   # combines freely
    for bad in (-0.01, 0.17, True, "long", float("nan"), {"a": 0.2}, {"a": True}, {"default": "x"}, [0.1, 0.2]):     # rule 14
        with pytest.raises(ValueError, match="min_duration must be a number of seconds between 0 and 0.16"):
            resolve({"align": "viterbi"}, min_duration=bad)
    with pytest.raises(ValueError, match="min_duration needs align='viterbi'"):                                      # rule 15
        resolve({}, min_duration=0.06)
    with pytest.raises(ValueError, match="min_duration needs align='viterbi'"):
        resolve({"align": "viterbi", "min_duration": {"a": 0.1}}, align="greedy")
    for key in ("align_scores", "align_edits", "align_insertions"):                                                  # rule 16
        with pytest.raises(ValueError) as e:
            resolve({"align": "viterbi", "min_duration": 0.06, key: True})
        assert str(e.value) == MIN_DURATION_SCORES_ERROR
    # the earlier rule is reported: 13 before 14, 14 before 15, 15 before 16
    with pytest.raises(ValueError, match="align_insertions needs"):
        resolve({}, align_insertions=True, min_duration=9)
    with pytest.raises(ValueError, match="min_duration must be"):
        resolve({}, min_duration=9)
    with pytest.raises(ValueError, match="min_duration needs"):
        resolve({"align_scores": False}, min_duration=0.1)
    # the CLI's values
    assert parse_min_duration(()) is None and parse_min_duration(["0.06"]) == 0.06
    assert parse_min_duration(["a=0.1", "0.04", "SP=0"]) == {"a": 0.1, "default": 0.04, "SP": 0.0}
    assert parse_min_duration(["a=0.1"]) == {"a": 0.1} and parse_min_duration(["long"]) == "long"
    with pytest.raises(ValueError, match="min_duration must be"):
        resolve({"align": "viterbi"}, min_duration=parse_min_duration(["a=long"]))


def test_post_options_carry_the_field():
    from wfl_asr_amd.options import PostOptions, resolve
    plain = resolve({"align": "viterbi"})
    a = resolve({"align": "viterbi", "min_duration": {"a": 0.1, "default": 0.04}})
    assert isinstance(a, PostOptions) and len(a) == 8 and a[:8] == plain[:8]         # the eight positional fields stay
    assert a != plain and plain != a and hash(a) != hash(plain) and a != tuple(a) and plain == tuple(plain)
    assert a == resolve({"align": "viterbi", "min_duration": {"default": 0.04, "a": 0.1}}) and len({a, plain, a}) == 2
    assert "min_duration=(('a', 0.1), ('default', 0.04))" in repr(a) and "min_duration=None" in repr(plain)
    assert a._replace(align_draft="d").min_duration == a.min_duration and a._replace(min_duration=None) == plain
    assert plain._replace(min_duration=0.06).min_duration == 0.06
    assert a._asdict()["min_duration"] == a.min_duration and PostOptions._make(tuple(a), min_duration=0.02).min_duration == 0.02
    with pytest.raises(AttributeError):
        a.min_duration = None


def test_the_option_is_refused_before_any_model_is_loaded(monkeypatch, tmp_path):
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import infer as I

    def no_load(*a, **k):
        raise AssertionError("a model was loaded before the options were refused")
    for f in (I.infer_audio, I.infer_folder, I.Labeler.label_files):
        assert inspect.signature(f).parameters["min_duration"].default is None
    monkeypatch.setattr(I, "_labeler", no_load)
    monkeypatch.setattr(I, "Labeler", no_load)
    with pytest.raises(ValueError, match="min_duration needs align='viterbi'"):
        I.infer_audio("x.wav", min_duration=0.06)
    with pytest.raises(ValueError, match="cannot be combined with a min_duration"):
        I.infer_folder("some_folder", align="viterbi", align_scores=True, min_duration={"a": 0.1})
    cfg = tmp_path / "config.yaml"
    cfg.write_text("postprocess:\n  align: viterbi\n  min_duration:\n    a: 0.5\n")
    with pytest.raises(ValueError, match="min_duration must be"):                                      # from the config file
        I.infer_audio("x.wav", config_path=str(cfg))
