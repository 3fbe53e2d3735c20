"""CPU (-m "not gpu"): the definition of the forced alignment with optional tokens (tests/viterbi_optional_ref.py against the
enumeration of every legal path), that a labelling is one path, the feasibility rule, `optional_flags`, the segments of a path that
lacks tokens, the .tsv text, the option rules of `postprocess.optional_tokens` / `postprocess.skip_penalty`, the refusals before a
model is loaded, the ABI entry's argument checks and the signatures that stay."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest

import viterbi_optional_ref as R
import viterbi_ref as V
from test_align_cpu import LABELS, _names, _path, table  # noqa: F401  (the label table fixture and the path builder)


@pytest.fixture(scope="module")
def AL():
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import align
    return align


def _tok_of(states):
    return tuple(-1 if s % 3 == 0 else s // 3 for s in states)


# ------------------------------------------------------------------------------------------------ 1. the definition
def test_dp_equals_enumeration_and_a_labelling_is_one_path():
    """Every T <= 5, N <= 4, every flag set, lambda in {0, 0.5, 2}."""
    rng = np.random.default_rng(81)
    C = 11
    lattices = with_path = without_path = skipping_optima = 0
    for T, N in itertools.product(range(1, 6), range(0, 5)):
        alts = [[(1 + 2 * k, 2 + 2 * k)] for k in range(N)]
        for opt in itertools.product((0, 1), repeat=N):
            lattices += 1
            paths = R.all_paths(T, N, opt)
            assert len({_tok_of(p) for p in paths}) == len(paths), "two legal paths with one tok"
            assert all(R.legal(p, N, opt) for p in paths)
            for p in paths:                               # only optional tokens are skipped, never two in a row
                sk = R.skipped_of(p, N)
                assert all(opt[k] for k in np.nonzero(sk)[0]) and not (sk[:-1] & sk[1:]).any()
                assert R.tokens_of(p) == [k for k in range(N) if not sk[k]]
            assert bool(paths) == (T >= R.min_frames_needed(opt))
            if not any(opt):
                assert len(paths) == len([p for p in R.all_paths(T, N, [0] * N) if V.legal(p, N)])
            z = rng.standard_normal((T, C))
            for lam in (0.0, 0.5, 2.0):
                path, score = R.viterbi(z, alts, [0, 9], opt, lam)
                if not paths:
                    without_path += 1
                    assert path is None and score == 0.0
                    continue
                with_path += 1
                best = max(R.path_score(p, z, alts, [0, 9], lam) for p in paths)
                assert abs(score - best) < 1e-9 and tuple(int(s) for s in path) in set(paths)
                assert abs(R.path_score(path, z, alts, [0, 9], lam) - best) < 1e-9
                skipping_optima += bool(R.skipped_of(path, N).any())
    print(lattices, with_path, without_path, skipping_optima)
    assert lattices == 5 * 31 and without_path > 50 and skipping_optima > 100


def test_ties_go_to_the_unskipped_arcs():
    """The order is per state: B_1 at frame 1 with B_0 and G_0 - lambda of frame 0 exactly equal takes B_0, the arc that skips nothing;
    a hair less on B_0's class and it takes the skip."""
    alts = [[(1, 2)], [(3, 4)]]
    z = np.zeros((2, 6))
    z[1, 0] = z[1, 4] = -5.0                              # frame 1: neither the gap nor I_1, so the clip ends in B_1
    for lam in (0.0, 1.0):
        z[0, 1] = -lam                                    # B_0 at frame 0 == G_0 at frame 0 minus lambda
        path, _ = R.viterbi(z, alts, [0], [1, 0], lam)
        assert list(path) == [1, 4] and not R.skipped_of(path, 2).any()
        z[0, 1] = -lam - 1e-6
        path, _ = R.viterbi(z, alts, [0], [1, 0], lam)
        assert list(path) == [0, 4] and R.skipped_of(path, 2).tolist() == [1, 0]
    # the same order among the ends: G_N | I_{N-1} | B_{N-1} before the ends that skip token N - 1
    assert list(R.viterbi(np.zeros((1, 6)), [[(1, 2)]], [0], [1], 0.0)[0]) == [1]


def test_without_flags_it_is_the_plain_dp_exactly():
    rng = np.random.default_rng(82)
    for T, N in ((1, 0), (1, 1), (9, 3), (40, 12), (40, 40)):
        alts = [[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 9, N)]
        z = rng.standard_normal((T, 20))
        a, sa = V.viterbi(z, alts, [0, 19])
        for lam in (0.0, 3.0):
            b, sb = R.viterbi(z, alts, [0, 19], None, lam)
            assert (a == b).all() and sa == sb
            assert (R.viterbi(z, alts, [0, 19], [0] * N, lam)[0] == a).all()
    assert R.viterbi(rng.standard_normal((2, 20)), [[(1, 2)]] * 3, [0]) == (None, 0.0)


def test_the_feasibility_rule_against_the_dp(AL):
    rng = np.random.default_rng(83)
    some_t_below_n = 0
    for N in range(0, 6):
        alts = [[(1 + 2 * k, 2 + 2 * k)] for k in range(N)]
        for opt in itertools.product((0, 1), repeat=N):
            need = AL.min_frames_needed(opt)
            assert need == R.min_frames_needed(opt) == AL.min_frames_needed([bool(f) for f in opt])
            for T in range(0, 7):
                path, _ = R.viterbi(rng.standard_normal((T, 13)), alts, [0], opt, 0.5)
                assert (path is not None) == (T >= need if N else True), (T, opt)
                some_t_below_n += path is not None and T < N
    assert some_t_below_n > 50
    assert AL.min_frames_needed([]) == 1 and AL.min_frames_needed([1]) == 1 and AL.min_frames_needed([0]) == 1
    assert AL.min_frames_needed([1] * 5) == 2 and AL.min_frames_needed([1, 1, 0, 0]) == 3 and AL.min_frames_needed([0, 1, 1, 1, 0, 1]) == 3


def test_windows_mask_eb_alone_and_an_empty_window_forces_the_skip():
    rng = np.random.default_rng(84)
    alts = [[(1, 2)], [(3, 4)], [(5, 6)]]
    z = rng.standard_normal((8, 9))
    wins = [(0, 7), (5, 4), (0, 7)]
    path, _ = R.viterbi(z, alts, [0], [0, 1, 0], 1.0, windows=wins)
    assert R.skipped_of(path, 3).tolist() == [0, 1, 0]
    assert R.viterbi(z, alts, [0], [0, 0, 0], 1.0, windows=wins) == (None, 0.0)
    z2, st = R.plant(12, 3, 9, alts, [0], rng, skipped=[1], runs=[(1, 2), (2, 3)])
    assert list(st) == [0, 1, 2, 3, 3, 7, 8, 8, 9, 9, 9, 9]           # the gap in front of the skipped token waits in G_1
    assert (R.viterbi(z2, alts, [0], [0, 1, 0], 2.5)[0] == st).all()


# ------------------------------------------------------------------------------------------------ 2. the host side
def test_optional_flags(AL):
    tr = ["a", "cl", "b", "cl", "SP"]
    assert AL.optional_flags(tr, ["cl"]) == [False, True, False, True, False]
    assert AL.optional_flags(tr, ("cl", "SP", "zz")) == [False, True, False, True, True]
    assert AL.optional_flags(tr, "*") == [True] * 5 and AL.optional_flags([], "*") == [] and AL.optional_flags(tr, []) == [False] * 5
    with pytest.raises(ValueError, match="list of token names"):
        AL.optional_flags(tr, "cl")


def test_pack_optional_and_the_batch_record(AL):
    N = np.array([2, 0, 1], np.int32)
    f = AL._pack_optional([[True, False], None, [1]], N)
    assert f.dtype == np.int32 and f.tolist() == [1, 0, 1]
    assert AL._pack_optional([None, None, [2]], N).tolist() == [0, 0, 2]             # (not 0 | 1: the kernel's status 4, not the packing's)
    assert AL._pack_optional([], np.zeros(0, np.int32)).tolist() == [0]
    with pytest.raises(ValueError, match="2 tokens"):
        AL._pack_optional([[True], None, None], N)
    with pytest.raises(ValueError, match="one entry per clip"):
        AL._pack_optional([None], N)
    with pytest.raises(ValueError, match="bools"):
        AL._pack_optional([[0.5, 1], None, None], N)
    b = AL.AlignBatch.of(None, [5, 6], [[1, 2], [3]], [[0], [0]], 0, opts=[None, [True]])
    assert b.optional == [None, [True]] and b.select([1]).opts == [[True]] and b.select([0]).optional is None
    plain = AL.AlignBatch.of(None, [5, 6], [[1, 2], [3]], [[0], [0]], 0)
    assert plain.optional is None and plain.select([1]).optional is None
    assert AL.AlignBatch.of(None, [5], [[1]], [[0]], 0, opts=[[False]]).optional is None


def test_segments_of_a_path_that_lacks_tokens(AL, table):  # noqa: F811
    from wfl_asr_amd import reports as RP
    tr = ["a", "b", "a", "b"]
    remap, names = _names(table)
    alts, why = AL.token_alternatives(tr, table, remap, names, LABELS)
    assert why is None
    spec = [(-1, "", ""), (0, "B", "a"), (0, "I", "a"), (-1, "", ""), (2, "B", "a"), (2, "I", "a"), (-1, "", "")]
    ids, tok = _path(table, spec)
    args = (ids, tok, [7], [None], [0.0], table, alts, tr, 0.02)
    segs = AL.path_segments(*args, skipped=[0, 1, 0, 1])
    assert [s[2] for s in segs] == ["a", "a"] and all(a < b for a, b, _ in segs) and segs[0][1] <= segs[1][0]
    for bad in ([0, 0, 0, 1], [0, 1, 0, 0], [1, 1, 0, 1], [0, 1, 1, 1]):      # a token is missing without its flag / present with it
        with pytest.raises(RuntimeError, match="does not spell the transcript"):
            AL.path_segments(*args, skipped=bad)
    with pytest.raises(RuntimeError, match="does not spell the transcript"):
        AL.path_segments(*args)                           # without flags: every token, as ever
    with pytest.raises(ValueError, match="one skipped flag per transcript token"):
        AL.path_segments(*args, skipped=[0, 1, 0])
    full = [(0, "B", "a"), (1, "B", "b"), (2, "B", "a"), (3, "B", "b")]
    ids4, tok4 = _path(table, full)
    assert AL.path_segments(ids4, tok4, [4], [None], [0.0], table, alts, tr, 0.02, skipped=[0] * 4) == \
        AL.path_segments(ids4, tok4, [4], [None], [0.0], table, alts, tr, 0.02)
    # the records and the .tsv text
    rows = AL.skipped_tokens([0, 1, 0, 1], segs, tr)
    assert rows == [AL.SkippedToken(1, "b", "a", "a", segs[1][0]), AL.SkippedToken(3, "b", "a", "", segs[1][1])]
    assert AL.SkippedToken._fields == ("index", "token", "after", "before", "at_s")
    first = AL.skipped_tokens([1, 0, 1, 0], [(0.1, 0.2, "b"), (0.3, 0.4, "b")], tr)
    assert first == [AL.SkippedToken(0, "a", "", "b", 0.1), AL.SkippedToken(2, "a", "b", "b", 0.3)]
    assert AL.skipped_tokens([0, 0, 0, 0], [(0, 1, x) for x in tr], tr) == [] and AL.skipped_tokens([1], [], ["a"])[0].at_s == 0.0
    with pytest.raises(ValueError, match="one segment per kept token"):
        AL.skipped_tokens([0, 1, 0, 1], segs[:1], tr)
    text = RP.file_text("skipped", first)
    assert text == "index\ttoken\tafter\tbefore\tat_s\n0\ta\t\tb\t0.1000000\n2\ta\tb\tb\t0.3000000\n"
    assert RP.file_text("skipped", []) == "index\ttoken\tafter\tbefore\tat_s\n"
    folder = RP.folder_text("skipped", [("x.wav", first), ("y.wav", []), ("z.wav", first[:1])])
    assert folder.splitlines() == ["file\tindex\ttoken\tafter\tbefore\tat_s", "x.wav\t0\ta\t\tb\t0.1000000", "x.wav\t2\ta\tb\tb\t0.3000000",
                                   "z.wav\t0\ta\t\tb\t0.1000000"]


def test_draft_moves_has_rows_for_kept_tokens_only():
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import infer as I
    draft = [(0.0, 0.1, "a"), (0.2, 0.3, "b"), (0.4, 0.5, "a")]
    tok = np.array([0, 0, -1, 2, 2], np.int32)
    wins = [(0, 1), (1, 3), (2, 4)]
    segs = [(0.01, 0.05, "a"), (0.07, 0.1, "a")]
    moves = I.draft_moves(draft, segs, tok, wins, [0, 1, 0])
    assert [(m.index, m.token, m.draft_start_s, m.start_s, m.on_edge) for m in moves] == [(0, "a", 0.0, 0.01, True), (2, "a", 0.4, 0.07, False)]
    full = I.draft_moves(draft, segs + [(0.2, 0.3, "a")], np.array([0, 1, 2]), wins)
    assert [m.index for m in full] == [0, 1, 2] and full == I.draft_moves(draft, segs + [(0.2, 0.3, "a")], np.array([0, 1, 2]), wins, [0, 0, 0])


# ------------------------------------------------------------------------------------------------ 3. the ABI
def test_the_abi_entry_checks_its_arguments(AL):
    import os
    from wfl_asr_amd import _lib
    lib = _lib.load()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wfl_asr.h")).read()
    for name in ("wfl_align_optional", "wfl_align_optional_workspace_bytes"):
        assert name + "(" in src and name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    sig = _lib.SIGNATURES["wfl_align_optional"][1]
    assert len(sig) == len(_lib.SIGNATURES["wfl_align_windowed"][1]) + 3 and sig[13] is ctypes.c_float
    Pv = ctypes.c_void_p
    buf = (ctypes.c_char * 64)()
    d = ctypes.cast(buf, Pv)                       # never dereferenced: every call below fails on the host
    fo, ko = np.zeros(1, np.int64), np.zeros(1, np.int32)
    T, N = np.array([10], np.int32), np.array([3], np.int32)
    h = lambda a: a.ctypes.data_as(Pv)             # noqa: E731
    need = lib.wfl_align_optional_workspace_bytes(h(T), h(N), 1)
    assert need == lib.wfl_align_workspace_bytes(h(T), h(N), 1) > 0

    def align(win=None, opt=d, lam=0.0, skipped=d, ws_bytes=need, C=141, ids=d, n=1):
        return lib.wfl_align_optional(d, 141, C, 0, h(fo), h(T), h(ko), h(N), d, win, d, n, opt, lam, d, ws_bytes, ids, d, d, skipped, d, None)
    for win in (None, d):                          # tok_win is nullable; tok_opt and skipped are not
        assert align(win, opt=None) == -1 and b"wfl_align_optional: null device" in lib.wfl_last_error()
        assert align(win, skipped=None) == -1 and b"wfl_align_optional: null device" in lib.wfl_last_error()
        assert align(win, ids=None) == -1 and b"null device" in lib.wfl_last_error()
        assert align(win, C=0) != 0 and b"wfl_align_optional: C must" in lib.wfl_last_error()
        assert align(win, ws_bytes=need - 1) != 0 and b"workspace" in lib.wfl_last_error()
        for lam in (-0.5, float("nan"), float("inf")):
            assert align(win, lam=lam) == -1 and b"wfl_align_optional: skip_penalty" in lib.wfl_last_error()
    assert align(lam=-1.0, n=0) == -1               # (judged before "nothing to do")
    assert align(n=-1) != 0 and b"n_clips" in lib.wfl_last_error()
    assert lib.wfl_align_optional(d, 141, 141, 0, None, None, None, None, None, None, d, 0, None, 0.0, None, 0, d, d, d, None, d, None) == 0
    # the workspace: wfl_align's own figure wherever T >= N; a clip with fewer frames than tokens may have a path here and has words
    cases = [(1500, 300), (10, 12), (3, 5), (4400, 4096), (4400, 4097), (100, 127), (100, 128), (7, 0), (0, 3), (1000, 2047)]
    words = lambda n: 64 if n <= 127 else 256 if n <= 1023 else 512 if n <= 2047 else 1024       # noqa: E731
    for t, n in cases:
        want = 0 if (n > 4096 or t == 0) else 4 * ((t * words(n) + 63) // 64 * 64)
        assert AL.optional_workspace_bytes([t], [n]) == want, (t, n)
        if t >= n:
            assert AL.optional_workspace_bytes([t], [n]) == AL.workspace_bytes([t], [n])
    assert lib.wfl_align_optional_workspace_bytes(None, None, 0) == 0 and lib.wfl_align_optional_workspace_bytes(None, None, 1) == -1


def test_signatures_that_stay_and_the_new_one(AL):
    assert list(inspect.signature(AL.viterbi_align).parameters) == [
        "logits", "n_frames", "token_classes", "gap_classes", "o_id", "frame_offsets", "stream", "packed", "windows", "min_frames"]
    assert list(inspect.signature(AL.pack_clips).parameters) == [
        "logits", "n_frames", "token_classes", "gap_classes", "frame_offsets", "windows", "min_frames"]
    assert AL.PackedClips._fields[-2:] == ("d_win", "d_min") and len(AL.PackedClips._fields) == 9
    p = inspect.signature(AL.viterbi_align_optional).parameters
    assert list(p) == ["logits", "n_frames", "token_classes", "gap_classes", "o_id", "optional", "skip_penalty", "frame_offsets", "stream",
                       "packed", "windows"]
    assert p["skip_penalty"].default == 0.0 and all(p[k].default is None for k in ("frame_offsets", "stream", "packed", "windows"))
    assert list(inspect.signature(AL.path_segments).parameters)[-1] == "skipped"
    assert inspect.signature(AL.path_segments).parameters["skipped"].default is None
    packed = AL.PackedClips(0, None, None, None, None, None, None, None, d_min=object())
    with pytest.raises(ValueError, match="no minimum durations"):
        AL.viterbi_align_optional(None, [], [], [], 0, [], packed=packed)


# ------------------------------------------------------------------------------------------------ 4. the options
def test_option_rules_19_to_23_and_their_order():
    from wfl_asr_amd.options import OPTIONAL_TOKENS_ERROR, PostOptions, resolve, unknown_optional_tokens
    d = resolve({})
    assert d.optional_tokens is None and d.skip_penalty == 0.0 and resolve({"align": "viterbi", "optional_tokens": []}).optional_tokens is None
    a = resolve({"align": "viterbi", "optional_tokens": ["q", "cl", "q"], "skip_penalty": "1.5"})
    assert a.optional_tokens == ("cl", "q") and a.skip_penalty == 1.5 and type(a.skip_penalty) is float
    assert resolve({"align": "viterbi", "optional_tokens": "*"}).optional_tokens == "*"
    assert resolve({"align": "viterbi", "optional_tokens": ["a", "*"]}).optional_tokens == "*"
    assert resolve({"align": "viterbi", "optional_tokens": ["a"]}, optional_tokens="*", skip_penalty=0).optional_tokens == "*"   # the argument wins
    assert resolve({"align": "viterbi"}, optional_tokens=a.optional_tokens, skip_penalty=1.5) == a          # the normalised form is taken back
    assert resolve({"align": "viterbi", "align_draft": "drafts", "optional_tokens": "*"}).align_draft == "drafts"      # combines with a draft
    assert resolve({"align": "viterbi", "optional_tokens": "*", "decode": "viterbi", "decode_scores": True}).decode_scores
    for bad in ("cl", 3, [1, 2], ["a", ""], {"a": 1}, True):                                                   # rule 19
        with pytest.raises(ValueError, match="optional_tokens must be a list of token names or"):
            resolve({"align": "viterbi"}, optional_tokens=bad)
    with pytest.raises(ValueError, match="optional_tokens needs align='viterbi'"):                              # rule 20
        resolve({}, optional_tokens=["cl"])
    with pytest.raises(ValueError, match="optional_tokens needs align='viterbi'"):
        resolve({"align": "viterbi", "optional_tokens": "*"}, align="greedy")
    for bad in (-0.1, True, "much", float("nan"), float("inf")):                                               # rule 21
        with pytest.raises(ValueError, match="skip_penalty must be a number >= 0"):
            resolve({"align": "viterbi", "optional_tokens": "*"}, skip_penalty=bad)
    with pytest.raises(ValueError, match="skip_penalty needs optional_tokens"):                                 # rule 22
        resolve({"align": "viterbi"}, skip_penalty=1.0)
    for other in ({"min_duration": 0.06}, {"align_scores": True}, {"align_edits": True}, {"align_insertions": True},
                  {"min_duration": 0.06, "duration_scores": True}):                                             # rule 23
        with pytest.raises(ValueError) as e:
            resolve({"align": "viterbi", "optional_tokens": ["cl"], **other})
        assert str(e.value) == OPTIONAL_TOKENS_ERROR
    # the earlier rule is reported: 18 before 19, 19 before 20, 20 before 21, 21 before 22, 22 before 23
    with pytest.raises(ValueError, match="duration_scores needs"):
        resolve({}, duration_scores=True, optional_tokens=3)
    with pytest.raises(ValueError, match="optional_tokens must be"):
        resolve({}, optional_tokens=3)
    with pytest.raises(ValueError, match="optional_tokens needs"):
        resolve({}, optional_tokens="*", skip_penalty=-1)
    with pytest.raises(ValueError, match="skip_penalty must be"):
        resolve({"align": "viterbi"}, skip_penalty=-1)
    with pytest.raises(ValueError, match="skip_penalty needs"):
        resolve({"align": "viterbi", "align_scores": True}, skip_penalty=1)
    # rule 24, for the caller that knows the model
    assert unknown_optional_tokens(("a", "zz", "SP", "q"), ["a", "b", "SP"]) == ["zz", "q"]
    assert unknown_optional_tokens("*", ["a"]) == [] and unknown_optional_tokens(None, ["a"]) == []
    # the record
    plain = resolve({"align": "viterbi"})
    assert isinstance(a, PostOptions) and len(a) == 8 and a[:8] == plain[:8] and len(PostOptions._fields) == 8
    assert a != plain and hash(a) != hash(plain) and a != tuple(a) and plain == tuple(plain) and hash(plain) == hash(tuple(plain))
    assert "optional_tokens=('cl', 'q'), skip_penalty=1.5" in repr(a) and "optional_tokens=None, skip_penalty=0.0" in repr(plain)
    assert a._replace(align_draft="d").optional_tokens == ("cl", "q") and a._replace(optional_tokens=None, skip_penalty=0.0) == plain
    assert a._asdict()["skip_penalty"] == 1.5 and PostOptions._make(tuple(a), optional_tokens="*").optional_tokens == "*"
    with pytest.raises(AttributeError):
        a.optional_tokens = None


def test_the_options_are_refused_before_any_model_is_loaded(monkeypatch, tmp_path):
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import infer as I

    def no_load(*a, **k):
        raise AssertionError("a model was loaded before the options were refused")
    for f in (I.infer_audio, I.infer_folder, I.Labeler.label_files):
        p = inspect.signature(f).parameters
        assert p["optional_tokens"].default is None and p["skip_penalty"].default is None
    monkeypatch.setattr(I, "_labeler", no_load)
    monkeypatch.setattr(I, "Labeler", no_load)
    with pytest.raises(ValueError, match="optional_tokens needs align='viterbi'"):
        I.infer_audio("x.wav", optional_tokens=["cl"])
    with pytest.raises(ValueError, match="cannot be combined with min_duration, align_scores"):
        I.infer_folder("some_folder", align="viterbi", align_edits=True, optional_tokens="*")
    cfg = tmp_path / "config.yaml"
    cfg.write_text("postprocess:\n  align: viterbi\n  skip_penalty: 2\n")
    with pytest.raises(ValueError, match="skip_penalty needs optional_tokens"):                        # from the config file
        I.infer_audio("x.wav", config_path=str(cfg))
    # the CLI: usage errors, exit code 2; and the flags reach the call
    seen = {}

    def record(*a, **k):
        seen.update(k)
        raise SystemExit(0)
    monkeypatch.setattr(I.torch.cuda, "is_available", lambda: True)     # (the CLI turns away a machine without a device first)
    monkeypatch.setattr(I, "infer_audio", record)
    monkeypatch.setattr(I, "infer_folder", record)
    wav, ckpt = tmp_path / "x.wav", tmp_path / "m.pt"
    wav.write_bytes(b"")
    ckpt.write_bytes(b"")
    cfg.write_text("postprocess:\n  align: viterbi\n")
    base = [str(wav), "-ckpt", str(ckpt), "-c", str(cfg)]
    for extra in (["--align", "greedy", "--optional", "cl"], ["--skip-penalty", "1"], ["--optional", "cl", "--skip-penalty", "-1"],
                  ["--optional", "cl", "--align-scores"], ["--optional", "cl", "--align-edits"], ["--optional", "*", "--align-insertions"],
                  ["--optional", "cl", "--min-duration", "0.06"], ["--optional", "cl", "--min-duration", "0.06", "--duration-scores"]):
        with pytest.raises(SystemExit) as e:
            I.main(base + extra)
        assert e.value.code == 2, extra
    with pytest.raises(SystemExit) as e:
        I.main(base + ["--optional", "q", "--optional", "cl", "--skip-penalty", "0.25"])
    assert e.value.code == 0 and seen["optional_tokens"] == ("cl", "q") and seen["skip_penalty"] == 0.25
    with pytest.raises(SystemExit) as e:
        I.main(base + ["--optional", "*"])
    assert e.value.code == 0 and seen["optional_tokens"] == "*" and seen["skip_penalty"] == 0.0
    with pytest.raises(SystemExit) as e:
        I.main(base)
    assert e.value.code == 0 and seen["optional_tokens"] is None and seen["skip_penalty"] is None
    cfg.write_text("postprocess:\n  align: viterbi\n  optional_tokens: [cl]\n  skip_penalty: 2\n")                 # from the config file
    with pytest.raises(SystemExit) as e:
        I.main(base)
    assert e.value.code == 0 and seen["optional_tokens"] == ("cl",) and seen["skip_penalty"] == 2.0
