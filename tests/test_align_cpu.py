"""CPU (-m "not gpu"): the Viterbi forced alignment's definition (tests/viterbi_ref.py against brute force), the path -> segments
assembly, the wfl_align ABI's argument checks and the `align` option of the public surface."""
import ctypes
import inspect

import numpy as np
import pytest

import viterbi_ref as V


# ------------------------------------------------------------------------------------------------ 1. the definition, ties included
@pytest.mark.parametrize("seed", range(6))
def test_dp_equals_brute_force_on_tiny_cases(seed):
    rng = np.random.default_rng(seed)
    C = 9
    for _ in range(40):
        N = int(rng.integers(0, 4))
        T = int(rng.integers(max(N, 1), 8 if N < 3 else 7))
        alts = [[(1 + 2 * int(p), 2 + 2 * int(p)) for p in rng.choice(3, size=int(rng.integers(1, 3)), replace=False)] for _ in range(N)]
        gaps = [0] if rng.random() < 0.5 else [0, 7, 8]
        if rng.random() < 0.5:
            z = rng.standard_normal((T, C))                     # no ties: the paths must be equal
            path, score = V.viterbi(z, alts, gaps)
            bpath, bscore = V.brute_force(z, alts, gaps)
            assert abs(score - bscore) < 1e-9
            assert (path == bpath).all()
        else:
            z = rng.integers(-1, 2, (T, C)).astype(np.float64)  # many exact ties: equal scores, a legal path
            path, score = V.viterbi(z, alts, gaps)
            _, bscore = V.brute_force(z, alts, gaps)
            assert abs(score - bscore) < 1e-9 and V.legal(path, N)
            assert abs(V.path_score(path, z, alts, gaps) - score) < 1e-9


def test_dp_ties_go_to_the_first_listed_predecessor():
    # all-zero logits: every legal path scores the same; the DP must end in G_N, and walk back through G_k (first listed)
    z = np.zeros((5, 5))
    path, _ = V.viterbi(z, [[(1, 2)]], [0])
    assert list(path) == [1, 3, 3, 3, 3]           # B_0 then G_1: G_1's first listed predecessor is G_1 itself
    path, _ = V.viterbi(np.zeros((2, 5)), [[(1, 2)], [(3, 4)]], [0])
    assert list(path) == [1, 4]
    assert V.viterbi(np.zeros((2, 5)), [[(1, 2)]] * 3, [0])[0] is None


# ------------------------------------------------------------------------------------------------ 2. path -> segments
LABELS = ["B-AP", "B-SP", "B-a", "B-b", "I-AP", "I-SP", "I-a", "I-b", "O"]


@pytest.fixture(scope="module")
def table():
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import native_post as npost
    return npost.LabelTable(LABELS)


def _names(table):
    return np.arange(len(table.names), dtype=np.int32), list(table.names)


def _path(table, spec):
    """spec: list of (token index or -1, 'B' | 'I') -> ids, tok."""
    from wfl_asr_amd import align as AL
    pairs = AL.class_pairs(LABELS)
    o = LABELS.index("O")
    ids, tok = [], []
    for k, kind, ph in spec:
        if k < 0:
            ids.append(o)
            tok.append(-1)
        else:
            ids.append(pairs[ph][0 if kind == "B" else 1])
            tok.append(k)
    return np.array(ids, np.int32), np.array(tok, np.int32)


def test_path_segments_one_per_token_equal_neighbours_separate(table):
    from wfl_asr_amd import align as AL
    tr = ["a", "a", "b"]
    remap, names = _names(table)
    alts, why = AL.token_alternatives(tr, table, remap, names, LABELS)
    assert why is None
    ids, tok = _path(table, [(-1, "", ""), (0, "B", "a"), (0, "I", "a"), (1, "B", "a"), (-1, "", ""), (2, "B", "b"), (2, "I", "b")])
    segs = AL.path_segments(ids, tok, [7], [None], [0.0], table, alts, tr, 0.02)
    assert [s[2] for s in segs] == tr
    assert all(a < b for a, b, _ in segs)
    assert all(segs[i][0] < segs[i + 1][0] for i in range(2))
    # the reference decoder's timing without offsets: run start + 0.5, closed at the frame that ends it (+ 0.5)
    assert segs[0][:2] == pytest.approx((0.03, 0.07)) and segs[1][:2] == pytest.approx((0.07, 0.09))


def test_path_segments_join_a_run_across_a_chunk_seam(table):
    from wfl_asr_amd import align as AL
    tr = ["a", "b", "b"]
    remap, names = _names(table)
    alts, _ = AL.token_alternatives(tr, table, remap, names, LABELS)
    spec = [(0, "B", "a"), (0, "I", "a"), (1, "B", "b"), (1, "I", "b"),      # chunk 0: 4 frames; token 1 runs on
            (1, "I", "b"), (2, "B", "b"), (-1, "", "")]                      # chunk 1: 3 frames
    ids, tok = _path(table, spec)
    offs0 = np.full((4, 2), 0.5, np.float32)
    offs1 = np.full((3, 2), 0.5, np.float32)
    segs = AL.path_segments(ids, tok, [4, 3], [offs0, offs1], [0.0, 30.0], table, alts, tr, 0.02)
    assert [s[2] for s in segs] == tr
    assert segs[1][0] == pytest.approx(2.5 * 0.02)          # starts in chunk 0
    assert segs[1][1] == pytest.approx(30.0 + 1.5 * 0.02)   # ends in chunk 1, at the B of the next (equal) token
    assert segs[2][0] == pytest.approx(30.0 + 1.5 * 0.02)


def test_pause_rule_at_the_ends_and_empty_transcript():
    from wfl_asr_amd import align as AL
    free = [(0.0, 0.2, "SP"), (0.2, 0.5, "a"), (0.5, 0.6, "AP"), (0.6, 0.9, "b"), (0.9, 1.2, "SP")]
    aligned = [(0.25, 0.5, "a"), (0.55, 0.85, "b")]
    assert AL.with_end_pauses(free, aligned, ["a", "b"]) == [free[0]] + aligned + [free[4]]
    assert AL.with_end_pauses(free, aligned, ["a", "SP", "b"]) == aligned
    assert AL.with_end_pauses(free, [], []) == []


def test_token_alternatives_and_gap_classes(table):
    from wfl_asr_amd import align as AL
    remap, names = _names(table)
    alts, why = AL.token_alternatives(["a", "x"], table, remap, names, LABELS)
    assert alts is None and "'x'" in why
    # a merge map that sends five phonemes to one output name: more than 4 alternatives
    labels = ["O"] + [f"B-p{i}" for i in range(5)] + [f"I-p{i}" for i in range(5)]
    from wfl_asr_amd import native_post as npost
    t5 = npost.LabelTable(labels)
    alts, why = AL.token_alternatives(["A"], t5, np.zeros(5, np.int32), ["A"], labels)
    assert alts is None and "5 phonemes" in why
    alts, why = AL.token_alternatives(["A"], t5, np.array([0, 0, 1, 1, 1], np.int32), ["A", "B"], labels)
    assert why is None and alts == [[(1, 6), (2, 7)]]
    o = LABELS.index("O")
    assert AL.gap_classes(LABELS, ["a"]) == [o, 1, 5, 0, 4]
    assert AL.gap_classes(LABELS, ["a", "SP"]) == [o, 0, 4]
    assert AL.gap_classes(["O", "B-a", "I-a"], ["a"]) == [0]


# ------------------------------------------------------------------------------------------------ 3. ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import _lib
    return _lib.load()


def test_align_symbols_are_declared_and_exported(lib):
    import os
    from wfl_asr_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wfl_asr.h")).read()
    for name in ("wfl_align", "wfl_align_workspace_bytes"):
        assert name + "(" in src and name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


def _words(N):
    return 64 if N <= 127 else 256 if N <= 1023 else 512 if N <= 2047 else 1024


def test_align_workspace_bytes_formula(lib):
    cases = [(1500, 300), (10, 12), (15000, 300), (4400, 4096), (4400, 4097), (2500, 1000), (100, 127), (100, 128), (7, 0), (3000, 2047)]
    T = np.array([c[0] for c in cases], np.int32)
    N = np.array([c[1] for c in cases], np.int32)
    want = sum(0 if (t < n or n > 4096) else 4 * ((t * _words(n) + 63) // 64 * 64) for t, n in cases)
    got = lib.wfl_align_workspace_bytes(T.ctypes.data_as(ctypes.c_void_p), N.ctypes.data_as(ctypes.c_void_p), len(cases))
    assert got == want
    bad = np.array([-1], np.int32)
    assert lib.wfl_align_workspace_bytes(bad.ctypes.data_as(ctypes.c_void_p), N.ctypes.data_as(ctypes.c_void_p), 1) < 0
    assert lib.wfl_align_workspace_bytes(None, None, 0) == 0


def test_align_validates_its_arguments_without_gpu(lib):
    P = ctypes.c_void_p
    buf = (ctypes.c_char * 64)()
    d = ctypes.cast(buf, P)                        # never dereferenced: every call below fails on the host
    fo = np.zeros(1, np.int64)
    T = np.array([10], np.int32)
    ko = np.zeros(1, np.int32)
    N = np.array([3], np.int32)
    h = lambda a: a.ctypes.data_as(P)              # noqa: E731

    def call(C=141, o_id=0, ldl=141, fo_=fo, T_=T, N_=N, ws=None, ws_bytes=0, logits=d, n=1, ids=d):
        return lib.wfl_align(logits, ldl, C, o_id, h(fo_) if fo_ is not None else None, h(T_), h(ko), h(N_), d, d, n, ws, ws_bytes,
                             ids, d, d, d, None)

    need = lib.wfl_align_workspace_bytes(h(T), h(N), 1)
    assert need > 0
    assert call(C=0) != 0 and b"C must" in lib.wfl_last_error()
    assert call(C=2000, ldl=2000) != 0 and b"C must" in lib.wfl_last_error()
    assert call(o_id=141) != 0 and b"o_id" in lib.wfl_last_error()
    assert call(o_id=-1) != 0 and b"o_id" in lib.wfl_last_error()
    assert call(ldl=100) != 0 and b"ldl" in lib.wfl_last_error()
    assert call(n=-1) != 0 and b"n_clips" in lib.wfl_last_error()
    assert call(fo_=None, ws=d, ws_bytes=need) != 0 and b"null host" in lib.wfl_last_error()
    assert call(T_=np.array([-2], np.int32), ws=d, ws_bytes=need) != 0 and b"negative" in lib.wfl_last_error()
    assert call(fo_=np.array([-1], np.int64), ws=d, ws_bytes=need) != 0 and b"negative offset" in lib.wfl_last_error()
    assert call(logits=None, ws=d, ws_bytes=need) != 0 and b"null device" in lib.wfl_last_error()
    assert call(ids=None, ws=d, ws_bytes=need) != 0 and b"null device" in lib.wfl_last_error()
    assert call(ws=d, ws_bytes=need - 1) != 0 and b"workspace" in lib.wfl_last_error()
    assert call(ws=None, ws_bytes=need) != 0 and b"workspace" in lib.wfl_last_error()
    assert call(n=0) == 0                          # nothing to do


# ------------------------------------------------------------------------------------------------ 4. the public surface
def test_align_option_on_the_public_surface():
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import infer as I
    for f in (I.infer_audio, I.infer_folder, I.Labeler.label_files):
        assert inspect.signature(f).parameters["align"].default is None
    assert I.ALIGN_MODES == ("greedy", "viterbi")
    with pytest.raises(ValueError, match="align"):
        I.infer_audio("x.wav", align="dtw")
    with pytest.raises(ValueError, match="align"):
        I.infer_folder("some_folder", align="dtw")
    # (how the option is resolved against the config: tests/test_options_cpu.py)


def test_cli_takes_align():
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import infer as I
    with pytest.raises(SystemExit) as e:
        I.main(["x.wav", "-ckpt", "m.pt", "-c", "c.yaml", "--align", "dtw"])
    assert e.value.code == 2                       # click: invalid choice, before anything is loaded
    with pytest.raises(SystemExit) as e:
        I.main(["--help"])
    assert e.value.code == 0
