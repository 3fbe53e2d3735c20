"""CPU (-m "not gpu"): the definition of the forced alignment with filler tokens (tests/viterbi_filler_ref.py against the enumeration
of every legal path), `filler_flags`, `collapse_fillers`, `filler_segments`, the segments of a path with a filler, the .tsv text, the
option rules of `postprocess.filler_token` / `postprocess.filler_penalty`, the refusals before a model is loaded and the ABI entry's
argument checks."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest

import viterbi_filler_ref as R
import viterbi_ref as V
from test_align_cpu import LABELS, _names, table  # noqa: F401  (the label table fixture)

F = "<fill>"


@pytest.fixture(scope="module")
def AL():
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import align
    return align


# ------------------------------------------------------------------------------------------------ 1. the definition
def test_dp_equals_enumeration_with_every_flag_pattern():
    """Every T <= 6, N <= 3, every flag pattern.  phi in {0.5, 2}: the DP's path is the best of all paths.  phi = 0: scores only (a
    filler then ties exactly with a neighbour wherever the neighbour's class is the frame's best); scores only, too, where two fillers
    stand side by side: a frame between them scores the same in either."""
    rng = np.random.default_rng(91)
    C = 9
    lattices = filler_wins = 0
    for T, N in itertools.product(range(1, 7), range(0, 4)):
        alts = [[(1 + 2 * k, 2 + 2 * k)] for k in range(N)]
        paths = R.all_paths(T, N)
        assert all(R.legal(p, N) for p in paths) and len(set(paths)) == len(paths) and bool(paths) == (T >= N)
        for fill in itertools.product((0, 1), repeat=N):
            lattices += 1
            z = rng.standard_normal((T, C))
            for phi in (0.0, 0.5, 2.0):
                path, score = R.viterbi(z, alts, [0, 8], fill, phi)
                if not paths:
                    assert path is None and score == 0.0
                    continue
                scores = {p: R.path_score(p, z, alts, [0, 8], fill, phi) for p in paths}
                best = max(scores.values())
                assert abs(score - best) < 1e-9 and abs(R.path_score(path, z, alts, [0, 8], fill, phi) - best) < 1e-9
                adjacent = any(x and y for x, y in zip(fill, fill[1:]))   # two fillers in a row tie exactly (the host collapses them)
                if phi > 0.0 and not adjacent:
                    assert sorted(scores.values())[-2:].count(best) == 1 or len(paths) == 1, "an exact tie on random logits"
                    assert tuple(int(s) for s in path) == max(scores, key=scores.get)
                    plain = V.path_score(path, z, alts, [0, 8]) if N else score
                    filler_wins += any(fill) and score > plain + 1e-9
    print(lattices, filler_wins)
    assert lattices == 6 * 15 and filler_wins > 20      # (the filler emission decides in a good share of the lattices)


def test_without_flags_it_is_the_plain_dp_exactly_and_the_emission_is_the_frames_best():
    rng = np.random.default_rng(92)
    for T, N in ((1, 0), (1, 1), (9, 3), (40, 12), (40, 40)):
        alts = [[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 9, N)]
        z = rng.standard_normal((T, 20))
        a, sa = V.viterbi(z, alts, [0, 19])
        for phi in (0.0, 3.0):
            b, sb = R.viterbi(z, alts, [0, 19], None, phi)
            assert (a == b).all() and abs(sa - sb) < 1e-9
            assert (R.viterbi(z, alts, [0, 19], [0] * N, phi)[0] == a).all()
    assert R.viterbi(rng.standard_normal((2, 20)), [[(1, 2)]] * 3, [0], [1, 1, 1]) == (None, 0.0)      # a filler needs its frame too
    # one filler alone over four frames: every frame at its best class minus phi, the gap classes included in the maximum
    z = rng.standard_normal((4, 7))
    z[2, 0] = 9.0                                          # the gap class is frame 2's best: the filler still takes max - phi there
    e = V.log_softmax(z)
    EB, EI, EG = R.emissions(z, [[(6, 6)]], [0], [1], 0.25)
    assert np.allclose(EB[:, 0], e.max(1) - 0.25) and np.allclose(EI[:, 0], e.max(1) - 0.25) and np.allclose(EG, e[:, 0])
    ids, tok = R.outputs([1, 2, 2, 2], z, [[(6, 6)]], 6, [1])
    assert tok.tolist() == [0] * 4 and ids.tolist() == z.argmax(1).tolist() and ids[2] == 0
    # windows mask a filler's EB like any token's
    EB, EI, _ = R.emissions(z, [[(6, 6)]], [0], [1], 0.25, windows=[(1, 2)])
    assert np.isneginf(EB[[0, 3], 0]).all() and np.isfinite(EB[1:3, 0]).all() and np.isfinite(EI).all()


def test_plant_gives_the_filler_frames_their_margin():
    rng = np.random.default_rng(93)
    alts = [[(1, 2)], [(11, 11)], [(3, 4)]]
    z, st = R.plant(30, 3, 12, alts, [0, 9], rng, fill=[0, 1, 0], runs=[(1, 5), (2, 9), (0, 6)])
    assert list(st[:6]) == [0, 1, 2, 2, 2, 2] and list(st[6:17]) == [3, 3, 4] + [5] * 8 and st[-1] == 9
    for t in np.nonzero(st // 3 == 1)[0]:
        if st[t] % 3:
            w = int(z[t].argmax())
            assert w not in (0, 9, 1, 2, 3, 4) and z[t, w] - np.delete(z[t], w).max() >= 8.0 - 1e-5
    for phi in (0.5, 1.5, 6.0):
        assert (R.viterbi(z, alts, [0, 9], [0, 1, 0], phi)[0] == st).all()


# ------------------------------------------------------------------------------------------------ 2. the host side
def test_filler_flags_collapse_and_segments(AL):
    tr = ["a", F, "b", F, F, F, "SP", F]
    assert AL.filler_flags(tr, F) == [False, True, False, True, True, True, False, True]
    assert AL.filler_flags(tr, "zz") == [False] * 8 and AL.filler_flags([], F) == []
    assert AL.collapse_fillers(tr, F) == (["a", F, "b", F, "SP", F], 2)
    assert AL.collapse_fillers(["a", "a", "b"], F) == (["a", "a", "b"], 0) and AL.collapse_fillers([], F) == ([], 0)
    assert AL.collapse_fillers([F, F], F) == ([F], 1)
    free = [(0.0, 0.2, "SP"), (0.2, 0.5, "a"), (0.5, 0.6, "AP"), (0.6, 0.9, "b"), (0.9, 1.2, "SP")]
    assert AL.filler_segments((0.3, 0.7, F), free) == [(0.3, 0.5, "a"), (0.5, 0.6, "AP"), (0.6, 0.7, "b")]
    assert AL.filler_segments((0.5, 0.6, F), free) == [(0.5, 0.6, "AP")]             # touching neighbours: no overlap, not held
    assert AL.filler_segments((1.2, 1.5, F), free) == [] and AL.filler_segments((0.5, 0.5, F), free) == []
    assert AL.filler_segments((0.0, 2.0, F), free) == free
    assert AL.filler_segments((0.1, 0.3, F), list(reversed(free))) == [(0.1, 0.2, "SP"), (0.2, 0.3, "a")]      # in time order


def test_the_tsv_texts(AL):
    from wfl_asr_amd import reports as RP
    rows = [AL.FillerSpan(1, 0.3, 0.7, 20, ("a", "AP", "b")), AL.FillerSpan(4, 1.25, 1.5, 12, ())]
    assert AL.FillerSpan._fields == ("index", "start_s", "end_s", "frames", "names")
    assert RP.file_text("fillers", rows) == ("index\tstart_s\tend_s\tframes\tnames\n1\t0.3000000\t0.7000000\t20\ta AP b\n"
                                           "4\t1.2500000\t1.5000000\t12\t\n")
    assert RP.file_text("fillers", []) == "index\tstart_s\tend_s\tframes\tnames\n"
    folder = RP.folder_text("fillers", [("x.wav", rows), ("y.wav", []), ("z.wav", rows[1:])])
    assert folder.splitlines() == ["file\tindex\tstart_s\tend_s\tframes\tnames", "x.wav\t1\t0.3000000\t0.7000000\t20\ta AP b",
                                   "x.wav\t4\t1.2500000\t1.5000000\t12\t", "z.wav\t4\t1.2500000\t1.5000000\t12\t"]


def test_pack_fillers_and_the_batch_record(AL):
    N = np.array([2, 0, 1], np.int32)
    f = AL._pack_fillers([[True, False], None, [1]], N)
    assert f.dtype == np.int32 and f.tolist() == [1, 0, 1]
    assert AL._pack_fillers([None, None, [2]], N).tolist() == [0, 0, 2]              # (not 0 | 1: the kernel's status 4, not the packing's)
    assert AL._pack_fillers([], np.zeros(0, np.int32)).tolist() == [0]
    with pytest.raises(ValueError, match="2 tokens"):
        AL._pack_fillers([[True], None, None], N)
    with pytest.raises(ValueError, match="one entry per clip"):
        AL._pack_fillers([None], N)
    with pytest.raises(ValueError, match="bools"):
        AL._pack_fillers([[0.5, 1], None, None], N)
    b = AL.AlignBatch.of(None, [5, 6], [[1, 2], [3]], [[0], [0]], 0, fills=[None, [True]])
    assert b.fillers == [None, [True]] and b.select([1]).fills == [[True]] and b.select([0]).fillers is None and b.optional is None
    plain = AL.AlignBatch.of(None, [5, 6], [[1, 2], [3]], [[0], [0]], 0)
    assert plain.fillers is None and plain.fills is None and plain.select([1]).fillers is None
    assert AL.AlignBatch.of(None, [5], [[1]], [[0]], 0, fills=[[False]]).fillers is None
    assert len(AL.PackedClips._fields) == 9
    p = inspect.signature(AL.viterbi_align_filler).parameters
    assert list(p) == ["logits", "n_frames", "token_classes", "gap_classes", "o_id", "fillers", "filler_penalty", "frame_offsets", "stream",
                       "packed", "windows"]
    assert p["filler_penalty"].default == 1.0 and all(p[k].default is None for k in ("frame_offsets", "stream", "packed", "windows"))
    assert inspect.signature(AL.path_segments).parameters["fillers"].default is None
    assert inspect.signature(AL.token_alternatives).parameters["filler"].default is None
    packed = AL.PackedClips(0, None, None, None, None, None, None, None, d_min=object())
    with pytest.raises(ValueError, match="no minimum durations"):
        AL.viterbi_align_filler(None, [], [], [], 0, [], packed=packed)
    assert AL._ENTRIES["wfl_align_filler"] == ("wfl_align_filler", True, False)


def _ids_tok(frames):
    """frames: list of (token index or -1, tag or 'O') -> ids, tok."""
    return (np.array([LABELS.index(tag) for _, tag in frames], np.int32), np.array([k for k, _ in frames], np.int32))


def test_segments_of_a_path_with_a_filler(AL, table):  # noqa: F811
    remap, names = _names(table)
    o = LABELS.index("O")
    tr = ["a", F, "b"]
    assert AL.token_alternatives(tr, table, remap, names, LABELS)[0] is None              # without the name: no such phoneme, as ever
    alts, why = AL.token_alternatives(tr, table, remap, names, LABELS, filler=F)
    assert why is None and alts[1] == [(o, o)] and alts[0] == [(2, 6)]
    fd = 0.02
    # in the middle: the filler's frames carry whatever class was the frame's best -- O, a B in the middle, the neighbours' own
    mid = [(-1, "O"), (0, "B-a"), (0, "I-a"), (1, "O"), (1, "B-b"), (1, "I-a"), (1, "B-a"), (-1, "O"), (2, "B-b"), (2, "I-b")]
    ids, tok = _ids_tok(mid)
    segs = AL.path_segments(ids, tok, [10], [None], [0.0], table, alts, tr, fd, fillers=[False, True, False])
    assert [s[2] for s in segs] == tr
    assert segs[0][:2] == pytest.approx((1.5 * fd, 3.5 * fd)) and segs[1][:2] == pytest.approx((3.5 * fd, 7.5 * fd))
    assert segs[2][0] == pytest.approx(8.5 * fd)
    with pytest.raises(ValueError, match="one filler flag per transcript token"):
        AL.path_segments(ids, tok, [10], [None], [0.0], table, alts, tr, fd, fillers=[True])
    # first and last
    first = [(0, "I-b"), (0, "O"), (1, "B-a"), (1, "I-a"), (-1, "O")]
    ids, tok = _ids_tok(first)
    a1, _ = AL.token_alternatives([F, "a"], table, remap, names, LABELS, filler=F)
    segs = AL.path_segments(ids, tok, [5], [None], [0.0], table, a1, [F, "a"], fd, fillers=[True, False])
    assert [s[2] for s in segs] == [F, "a"] and segs[0][:2] == pytest.approx((0.5 * fd, 2.5 * fd)) and segs[1][0] == pytest.approx(2.5 * fd)
    last = [(0, "B-a"), (1, "O"), (1, "O"), (1, "B-b")]
    ids, tok = _ids_tok(last)
    a2, _ = AL.token_alternatives(["a", F], table, remap, names, LABELS, filler=F)
    segs = AL.path_segments(ids, tok, [4], [None], [0.0], table, a2, ["a", F], fd, fillers=[False, True])
    assert [s[2] for s in segs] == ["a", F] and segs[0][:2] == pytest.approx((0.5 * fd, 1.5 * fd)) and segs[1][0] == pytest.approx(1.5 * fd)
    assert segs[1][1] > segs[1][0]
    # across a chunk seam: one span, from chunk 0's clock to chunk 1's
    seam = [(0, "B-a"), (1, "I-b"), (1, "O"),                                            # chunk 0: 3 frames; the filler runs on
            (1, "B-a"), (1, "O"), (2, "B-b"), (-1, "O")]                                 # chunk 1: 4 frames
    ids, tok = _ids_tok(seam)
    offs = [np.full((3, 2), 0.5, np.float32), np.full((4, 2), 0.5, np.float32)]
    segs = AL.path_segments(ids, tok, [3, 4], offs, [0.0, 30.0], table, alts, tr, fd, fillers=[False, True, False])
    assert [s[2] for s in segs] == tr
    assert segs[1][0] == pytest.approx(1.5 * fd) and segs[1][1] == pytest.approx(30.0 + 2.5 * fd)
    assert segs[2][0] == pytest.approx(30.0 + 2.5 * fd)
    # without a filler in the flags every result is what it is without the argument
    plain = [(-1, "O"), (0, "B-a"), (0, "I-a"), (1, "B-a"), (-1, "O"), (2, "B-b"), (2, "I-b")]
    ids, tok = _ids_tok(plain)
    a3, _ = AL.token_alternatives(["a", "a", "b"], table, remap, names, LABELS, filler=F)
    assert a3 == AL.token_alternatives(["a", "a", "b"], table, remap, names, LABELS)[0]
    args = (ids, tok, [7], [None], [0.0], table, a3, ["a", "a", "b"], fd)
    assert AL.path_segments(*args) == AL.path_segments(*args, fillers=[False] * 3) == AL.path_segments(*args, fillers=None)


# ------------------------------------------------------------------------------------------------ 3. the ABI
def test_the_abi_entry_checks_its_arguments(AL):
    import os
    from wfl_asr_amd import _lib
    lib = _lib.load()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wfl_asr.h")).read()
    for name in ("wfl_align_filler", "wfl_align_filler_workspace_bytes"):
        assert name + "(" in src and name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    sig = _lib.SIGNATURES["wfl_align_filler"][1]
    assert len(sig) == len(_lib.SIGNATURES["wfl_align_windowed"][1]) + 2 and sig[13] is ctypes.c_float
    Pv = ctypes.c_void_p
    buf = (ctypes.c_char * 64)()
    d = ctypes.cast(buf, Pv)                       # never dereferenced: every call below fails on the host
    fo, ko = np.zeros(1, np.int64), np.zeros(1, np.int32)
    T, N = np.array([10], np.int32), np.array([3], np.int32)
    h = lambda a: a.ctypes.data_as(Pv)             # noqa: E731
    need = lib.wfl_align_filler_workspace_bytes(h(T), h(N), 1)
    assert need == lib.wfl_align_workspace_bytes(h(T), h(N), 1) > 0

    def align(win=None, fill=d, phi=1.0, ws_bytes=need, C=141, ids=d, n=1):
        return lib.wfl_align_filler(d, 141, C, 0, h(fo), h(T), h(ko), h(N), d, win, d, n, fill, phi, d, ws_bytes, ids, d, d, d, None)
    for win in (None, d):                          # tok_win is nullable; tok_fill is not
        assert align(win, fill=None) == -1 and b"wfl_align_filler: null device" in lib.wfl_last_error()
        assert align(win, ids=None) == -1 and b"null device" in lib.wfl_last_error()
        assert align(win, C=0) != 0 and b"wfl_align_filler: C must" in lib.wfl_last_error()
        assert align(win, ws_bytes=need - 1) != 0 and b"workspace" in lib.wfl_last_error()
        for phi in (-0.5, float("nan"), float("inf")):
            assert align(win, phi=phi) == -1 and b"wfl_align_filler: filler_penalty" in lib.wfl_last_error()
    assert align(phi=-1.0, n=0) == -1               # (judged before "nothing to do")
    assert align(n=-1) != 0 and b"n_clips" in lib.wfl_last_error()
    assert lib.wfl_align_filler(d, 141, 141, 0, None, None, None, None, None, None, d, 0, None, 1.0, None, 0, d, d, d, d, None) == 0
    # the workspace: wfl_align's own figure, clip by clip and on a ragged batch
    Ts, Ns = [1500, 10, 3, 4400, 4400, 100, 100, 7, 0, 1000], [300, 12, 5, 4096, 4097, 127, 128, 0, 3, 2047]
    assert AL.filler_workspace_bytes(Ts, Ns) == AL.workspace_bytes(Ts, Ns) > 0
    for t, n in zip(Ts, Ns):
        assert AL.filler_workspace_bytes([t], [n]) == AL.workspace_bytes([t], [n])
    assert lib.wfl_align_filler_workspace_bytes(None, None, 0) == 0 and lib.wfl_align_filler_workspace_bytes(None, None, 1) == -1


# ------------------------------------------------------------------------------------------------ 4. the options
def test_option_rules_27_to_32_and_their_order():
    from wfl_asr_amd.options import DEFAULT_FILLER_PENALTY, FILLER_TOKEN_ERROR, PostOptions, filler_token_collision, resolve
    import wfl_asr_amd.options as OPT
    d = resolve({})
    assert d.filler_token is None and d.filler_penalty == 1.0 == DEFAULT_FILLER_PENALTY
    a = resolve({"align": "viterbi", "filler_token": F, "filler_penalty": "2.5"})
    assert a.filler_token == F and a.filler_penalty == 2.5 and type(a.filler_penalty) is float
    assert resolve({"align": "viterbi", "filler_token": "spn"}).filler_penalty == 1.0
    assert resolve({"align": "viterbi", "filler_token": "spn"}, filler_token=F, filler_penalty=0).filler_token == F    # the argument wins
    assert resolve({"align": "viterbi"}, filler_token=F, filler_penalty=2.5) == a
    assert resolve({"align": "viterbi", "filler_token": F, "decode": "viterbi", "decode_scores": True}).decode_scores
    for bad in ("", "a b", "a\tb", " x", "x\n", 3, ["a"], True, ("a",)):                                      # rule 27
        with pytest.raises(ValueError, match="filler_token must be a non-empty string without whitespace"):
            resolve({"align": "viterbi"}, filler_token=bad)
    with pytest.raises(ValueError, match="filler_token needs align='viterbi'"):                                 # rule 28
        resolve({}, filler_token=F)
    with pytest.raises(ValueError, match="filler_token needs align='viterbi'"):
        resolve({"align": "viterbi", "filler_token": F}, align="greedy")
    for bad in (-0.1, True, "much", float("nan"), float("inf")):                                               # rule 29
        with pytest.raises(ValueError, match="filler_penalty must be a finite number >= 0"):
            resolve({"align": "viterbi", "filler_token": F}, filler_penalty=bad)
    with pytest.raises(ValueError, match="filler_penalty needs a filler_token"):                                # rule 30
        resolve({"align": "viterbi"}, filler_penalty=1.0)
    for other in ({"align_draft": "drafts"}, {"min_duration": 0.06}, {"optional_tokens": ["cl"]}, {"align_scores": True},
                  {"align_edits": True}, {"align_insertions": True}, {"min_duration": 0.06, "duration_scores": True},
                  {"optional_tokens": "*", "optional_scores": True}):                                          # rule 31
        with pytest.raises(ValueError) as e:
            resolve({"align": "viterbi", "filler_token": F, **other})
        assert str(e.value) == FILLER_TOKEN_ERROR
    for word in ("align_draft", "min_duration", "optional_tokens", "align_scores", "align_edits", "align_insertions", "duration_scores",
                 "optional_scores", "no filler emission"):
        assert word in FILLER_TOKEN_ERROR
    # the earlier rule is reported: 26 before 27, 27 before 28, 28 before 29, 29 before 30, 30 before 31
    with pytest.raises(ValueError, match="optional_scores needs"):
        resolve({}, optional_scores=True, filler_token="")
    with pytest.raises(ValueError, match="optional_scores needs optional_tokens"):
        resolve({"align": "viterbi"}, optional_scores=True, filler_token="")
    with pytest.raises(ValueError, match="filler_token must be"):
        resolve({}, filler_token="a b")
    with pytest.raises(ValueError, match="filler_token needs"):
        resolve({}, filler_token=F, filler_penalty=-1)
    with pytest.raises(ValueError, match="filler_penalty must be"):
        resolve({"align": "viterbi"}, filler_penalty=-1)
    with pytest.raises(ValueError, match="filler_penalty needs"):
        resolve({"align": "viterbi", "align_scores": True}, filler_penalty=1)
    # rule 32, for the caller that knows the model
    assert filler_token_collision("a", ["a", "b", "SP"]) == "a" and filler_token_collision(F, ["a", "b"]) is None
    assert filler_token_collision(None, ["a"]) is None
    # the table at the top of the module says what the default is
    doc = " ".join(OPT.__doc__.split())
    assert "a value to start from, not a measured optimum" in doc and "27." in doc and "(32." in doc
    # the record
    plain = resolve({"align": "viterbi"})
    assert isinstance(a, PostOptions) and len(a) == 8 and a[:8] == plain[:8] and len(PostOptions._fields) == 8
    assert PostOptions._KEYWORD[-2:] == ("filler_token", "filler_penalty") and PostOptions._KEYWORD[-3] == "optional_scores"
    assert a != plain and hash(a) != hash(plain) and a != tuple(a) and plain == tuple(plain) and hash(plain) == hash(tuple(plain))
    assert f"filler_token={F!r}, filler_penalty=2.5" in repr(a) and "filler_token=None, filler_penalty=1.0" in repr(plain)
    assert a._replace(decode="viterbi").filler_token == F and a._replace(filler_token=None, filler_penalty=1.0) == plain
    assert a._asdict()["filler_penalty"] == 2.5 and PostOptions._make(tuple(a), filler_token="x").filler_token == "x"
    assert {a: 1}[resolve({"align": "viterbi"}, filler_token=F, filler_penalty=2.5)] == 1
    with pytest.raises(AttributeError):
        a.filler_token = None


def test_the_options_are_refused_before_any_model_is_loaded(monkeypatch, tmp_path):
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import infer as I

    def no_load(*a, **k):
        raise AssertionError("a model was loaded before the options were refused")
    for f in (I.infer_audio, I.infer_folder, I.Labeler.label_files):
        p = inspect.signature(f).parameters
        assert p["filler_token"].default is None and p["filler_penalty"].default is None
    assert I.ViterbiLabel._fields[-1] == "rows" and I.ViterbiLabel([]).rows.get("fillers") is None
    monkeypatch.setattr(I, "_labeler", no_load)
    monkeypatch.setattr(I, "Labeler", no_load)
    with pytest.raises(ValueError, match="filler_token needs align='viterbi'"):
        I.infer_audio("x.wav", filler_token=F)
    with pytest.raises(ValueError, match="cannot be combined with align_draft, min_duration"):
        I.infer_folder("some_folder", align="viterbi", align_edits=True, filler_token=F)
    cfg = tmp_path / "config.yaml"
    cfg.write_text("postprocess:\n  align: viterbi\n  filler_penalty: 2\n")
    with pytest.raises(ValueError, match="filler_penalty needs a filler_token"):                        # from the config file
        I.infer_audio("x.wav", config_path=str(cfg))
    # the CLI: usage errors, exit code 2; and the flags reach the call
    seen = {}

    def record(*a, **k):
        seen.update(k)
        raise SystemExit(0)
    monkeypatch.setattr(I.torch.cuda, "is_available", lambda: True)     # (the CLI turns away a machine without a device first)
    monkeypatch.setattr(I, "infer_audio", record)
    monkeypatch.setattr(I, "infer_folder", record)
    wav, ckpt, folder = tmp_path / "x.wav", tmp_path / "m.pt", tmp_path / "wavs"
    wav.write_bytes(b"")
    ckpt.write_bytes(b"")
    folder.mkdir()
    cfg.write_text("postprocess:\n  align: viterbi\n")
    base = [str(wav), "-ckpt", str(ckpt), "-c", str(cfg)]
    for extra in (["--align", "greedy", "--filler-token", F], ["--filler-penalty", "1"], ["--filler-token", F, "--filler-penalty", "-1"],
                  ["--filler-token", "a b"], ["--filler-token", F, "--align-scores"], ["--filler-token", F, "--align-edits"],
                  ["--filler-token", F, "--align-insertions"], ["--filler-token", F, "--min-duration", "0.06"],
                  ["--filler-token", F, "--optional", "cl"], ["--filler-token", F, "--align-draft", "drafts"]):
        with pytest.raises(SystemExit) as e:
            I.main(base + extra)
        assert e.value.code == 2, extra
    with pytest.raises(SystemExit) as e:
        I.main([str(folder)] + base[1:] + ["--filler-token", F, "--filler-penalty", "0.25"])              # a folder: infer_folder
    assert e.value.code == 0 and seen["filler_token"] == F and seen["filler_penalty"] == 0.25 and "folder_path" in seen
    seen.clear()
    with pytest.raises(SystemExit) as e:
        I.main(base + ["--filler-token", F])
    assert e.value.code == 0 and seen["filler_token"] == F and seen["filler_penalty"] == 1.0 and "audio_path" in seen
    with pytest.raises(SystemExit) as e:
        I.main(base)
    assert e.value.code == 0 and seen["filler_token"] is None and seen["filler_penalty"] is None
    cfg.write_text("postprocess:\n  align: viterbi\n  filler_token: spn\n  filler_penalty: 2\n")                     # from the config file
    with pytest.raises(SystemExit) as e:
        I.main([str(folder)] + base[1:])
    assert e.value.code == 0 and seen["filler_token"] == "spn" and seen["filler_penalty"] == 2.0
