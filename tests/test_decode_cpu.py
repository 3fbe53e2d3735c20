"""CPU (-m "not gpu"): the BIO-grammar Viterbi decode's definition (tests/bio_viterbi_ref.py against exhaustive enumeration), the
class table, the path -> segments assembly, the wfl_decode ABI's argument checks and the `decode` option of the public surface."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import bio_viterbi_ref as R

# an orphan I- (I-z), a B- without I- (B-c) and a name that is not BIO (sil)
LABELS8 = ["O", "B-a", "I-a", "B-b", "I-b", "B-c", "I-z", "sil"]
TABLE8 = (0, [(1, 2), (3, 4), (5, -1)])


# ------------------------------------------------------------------------------------------------ 1. the definition
@pytest.mark.parametrize("lam", [0.0, 0.3, 1.5, 4.0])
@pytest.mark.parametrize("with_forced", [False, True])
def test_reference_equals_exhaustive_enumeration(lam, with_forced):
    """38 seeded cases per (lambda, forced) pair, 304 in all: T <= 5, the 8 classes above, every one of the 8^T class strings."""
    for seed in range(38):
        rng = np.random.default_rng(1000 * seed + int(10 * lam) + (7 if with_forced else 0))
        T = int(rng.integers(1, 6))
        z = rng.standard_normal((T, 8)) * 2.0
        forced = (rng.random(T) < 0.4) if with_forced else None
        ids, obj = R.viterbi(z, TABLE8, lam, forced)
        bids, bobj = R.brute_force(z, TABLE8, lam, forced)
        assert R.legal(ids, TABLE8)
        assert abs(obj - bobj) < 1e-9, (seed, obj, bobj)
        assert abs(R.objective(ids, z, TABLE8, lam, forced) - obj) < 1e-9
        assert (ids == bids).all()                       # Gaussian logits: no ties, one optimum
        if forced is not None:
            assert (ids[forced] == 0).all()


def test_class_table_roles():
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import decode as DC
    t = DC.class_table(LABELS8)
    assert t.o_id == 0 and t.pairs.tolist() == [[1, 2], [3, 4], [5, -1]]
    with pytest.raises(ValueError, match="'O'"):
        DC.class_table(["B-a", "I-a"])


def test_class_table_on_the_synthetic_label_sets():
    import __graft_entry__  # noqa: F401
    import synthetic as synth
    from wfl_asr_amd import decode as DC
    for P in (5, 70):
        labels = synth.make_labels(P)
        t = DC.class_table(labels)
        assert labels[t.o_id] == "O" and t.pairs.shape == (P, 2)
        for b, i in t.pairs:
            assert labels[b].startswith("B-") and labels[i] == "I-" + labels[b][2:]
        assert len(set(t.pairs.reshape(-1).tolist()) | {t.o_id}) == 2 * P + 1


def test_lambda_zero_on_a_legal_argmax_is_the_argmax():
    rng = np.random.default_rng(4)
    table = (0, [(2 * p + 1, 2 * p + 2) for p in range(6)])
    for _ in range(20):
        z, ids = R.plant(int(rng.integers(1, 120)), 13, table, rng, margin=9.0, min_run=1, max_run=9)
        assert (z.argmax(1) == ids).all() and R.legal(ids, table)          # (test setup)
        got, obj = R.viterbi(z, table, 0.0)
        assert (got == ids).all()
        assert abs(obj - float(z.astype(np.float64)[np.arange(len(ids)), ids].sum())) < 1e-9


def test_a_planted_flicker_is_absorbed():
    """One frame of B-b inside a long run of a: keeping it opens two runs (the flicker and the resumed a), so a margin below
    2 lambda is absorbed when the resumed frame's B-a logit is not above its I-a logit; with lambda = 0 the flicker is kept."""
    table = (0, [(1, 2), (3, 4)])
    z = np.full((12, 5), -10.0)
    z[0, 1] = 5.0
    z[1:, 2] = 5.0
    z[6, 3] = 5.0 + 3.0                                  # the flicker: B-b beats I-a by 3 on frame 6
    z[7, 1] = 5.0                                        # the resumed frame: B-a ties I-a
    clean = np.array([1] + [2] * 11, np.int32)
    kept = clean.copy()
    kept[6], kept[7] = 3, 1
    assert (R.viterbi(z, table, 0.0)[0] == kept).all()
    assert (R.viterbi(z, table, 1.4)[0] == kept).all()   # 2 lambda = 2.8 < 3: still worth two runs
    assert (R.viterbi(z, table, 1.6)[0] == clean).all()  # 2 lambda = 3.2 > 3: absorbed
    assert (R.viterbi(z, table, 4.0)[0] == clean).all()


def test_float32_restatement_follows_the_float64_one():
    rng = np.random.default_rng(8)
    table = (0, [(2 * p + 1, 2 * p + 2) for p in range(6)])
    z, ids = R.plant(400, 13, table, rng)
    a, oa = R.viterbi(z, table, 2.0)
    b, ob = R.viterbi(z, table, 2.0, dtype=np.float32)
    assert (a == ids).all() and (b == ids).all() and abs(oa - ob) < 1e-3 * 400


# ------------------------------------------------------------------------------------------------ 2. path -> segments
LABELS = ["B-a", "B-b", "I-a", "I-b", "O"]
Ba, Bb, Ia, Ib, O = range(5)


@pytest.fixture(scope="module")
def table():
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import native_post as npost
    return npost.LabelTable(LABELS)


def test_segments_seam_joining_and_end_capping(table):
    from wfl_asr_amd import decode as DC
    fd = 0.02
    # chunk 0: O a a a | chunk 1 begins with I-a: the run crosses the seam; then b; chunk 2 begins with I-b after O: not a seam run
    ids = [O, Ba, Ia, Ia] + [Ia, Ia, Bb, Ib] + [O, O]
    s, e, ph = DC.path_segments_free(ids, [4, 4, 2], [None, None, None], [0.0, 30.0, 60.0], table, fd)
    assert [table.names[p] for p in ph] == ["a", "b"]
    assert s[0] == pytest.approx(1.5 * fd) and e[0] == pytest.approx(30.0 + 2.5 * fd)     # joined: ends where b starts
    assert s[1] == pytest.approx(30.0 + 2.5 * fd) and e[1] == pytest.approx(30.0 + 3.5 * fd)
    # the same phoneme on both sides of a seam, but the next chunk opens with B-a: two segments
    s, e, ph = DC.path_segments_free([Ba, Ia, Ba, Ia], [2, 2], [None, None], [0.0, 30.0], table, fd)
    assert len(s) == 2 and s[1] == pytest.approx(30.0 + 0.5 * fd)
    # I-a at a chunk's start after a chunk that ended in O cannot come from a legal path's seam; it is a segment of its own
    s, e, ph = DC.path_segments_free([Ba, O, Ia, Ia], [2, 2], [None, None], [0.0, 30.0], table, fd)
    assert len(s) == 2
    # B-a directly after B-a, and after I-a, of the same phoneme: new segments
    s, e, ph = DC.path_segments_free([Ba, Ba, Ia, Ba, O], [5], [None], [0.0], table, fd)
    assert [table.names[p] for p in ph] == ["a", "a", "a"]
    assert list(s) == pytest.approx([0.5 * fd, 1.5 * fd, 3.5 * fd]) and list(e) == pytest.approx([1.5 * fd, 3.5 * fd, 4.5 * fd])
    # offsets: an end offset that runs past the next start is capped at it, and no end is before its start
    offs = np.zeros((4, 2), np.float32)
    offs[:, 0] = 0.2
    offs[:, 1] = 0.9
    s, e, ph = DC.path_segments_free([Ba, Ia, Bb, O], [4], [offs], [0.0], table, fd)
    assert e[0] == pytest.approx(min(2.9 * fd, 2.2 * fd)) and s[1] == pytest.approx(2.2 * fd) and (e >= s).all()
    # an empty file and an empty chunk
    s, e, ph = DC.path_segments_free([], [0], [None], [0.0], table, fd)
    assert len(s) == len(e) == len(ph) == 0


# ------------------------------------------------------------------------------------------------ 3. the ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import _lib
    return _lib.load()


def test_header_declares_decode(lib):
    from wfl_asr_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wfl_asr.h")).read()
    for name in ("wfl_decode", "wfl_decode_workspace_bytes"):
        assert name + "(" in src and name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert "infer.py:86-96, 164-174, 293-302" in src
    assert lib.wfl_abi_version() == 2                  # additive: the ABI version is unchanged


def _slots(n_pairs):
    return 2 if n_pairs <= 128 else 4 if n_pairs <= 256 else 8 if n_pairs <= 512 else 16


def test_decode_workspace_bytes_rule(lib):
    """Per clip with T > 0: round_up_64(T (2 S + 1)) + 2 round_up_64(T) words; S by the pair count; 0 above 1024 pairs."""
    r64 = lambda v: (v + 63) // 64 * 64                # noqa: E731
    Ts = [1500, 1, 0, 15000, 63, 64, 65]
    T = np.array(Ts, np.int32)
    for n_pairs in (0, 70, 128, 129, 256, 511, 512, 513, 1023, 1024):
        S = _slots(n_pairs)
        want = sum(4 * (r64(t * (2 * S + 1)) + 2 * r64(t)) for t in Ts if t > 0)
        assert lib.wfl_decode_workspace_bytes(T.ctypes.data_as(ctypes.c_void_p), len(Ts), n_pairs) == want
    assert lib.wfl_decode_workspace_bytes(T.ctypes.data_as(ctypes.c_void_p), len(Ts), 1025) == 0
    assert lib.wfl_decode_workspace_bytes(T.ctypes.data_as(ctypes.c_void_p), 1, 70) == 4 * (r64(1500 * 5) + 2 * r64(1500))
    bad = np.array([-1], np.int32)
    assert lib.wfl_decode_workspace_bytes(bad.ctypes.data_as(ctypes.c_void_p), 1, 70) < 0
    assert lib.wfl_decode_workspace_bytes(T.ctypes.data_as(ctypes.c_void_p), -1, 70) < 0
    assert lib.wfl_decode_workspace_bytes(T.ctypes.data_as(ctypes.c_void_p), 1, -1) < 0
    assert lib.wfl_decode_workspace_bytes(None, 1, 70) < 0
    assert lib.wfl_decode_workspace_bytes(None, 0, 70) == 0


def test_decode_validates_its_arguments_without_gpu(lib):
    P = ctypes.c_void_p
    buf = (ctypes.c_char * 64)()
    d = ctypes.cast(buf, P)                        # never dereferenced: every call below fails on the host
    fo = np.zeros(1, np.int64)
    T = np.array([10], np.int32)
    h = lambda a: a.ctypes.data_as(P)              # noqa: E731

    def call(C=141, o_id=0, ldl=141, fo_=fo, T_=T, ws=None, ws_bytes=0, logits=d, n=1, ids=d, pairs=d, n_pairs=70, lam=1.0, thr=0.0,
             score=d):
        return lib.wfl_decode(logits, ldl, C, o_id, h(fo_) if fo_ is not None else None, h(T_), n, pairs, n_pairs, lam, thr, ws, ws_bytes,
                              ids, score, d, None)

    need = lib.wfl_decode_workspace_bytes(h(T), 1, 70)
    assert need > 0
    assert call(C=0) != 0 and b"C < 1" in lib.wfl_last_error()
    assert call(o_id=141) != 0 and b"o_id" in lib.wfl_last_error()
    assert call(o_id=-1) != 0 and b"o_id" in lib.wfl_last_error()
    assert call(ldl=100) != 0 and b"ldl" in lib.wfl_last_error()
    assert call(n=-1) != 0 and b"negative count" in lib.wfl_last_error()
    assert call(n_pairs=-1) != 0 and b"negative count" in lib.wfl_last_error()
    assert call(lam=-0.5) != 0 and b"lambda" in lib.wfl_last_error()
    assert call(lam=float("nan")) != 0 and b"lambda" in lib.wfl_last_error()
    assert call(thr=-0.1) != 0 and b"threshold" in lib.wfl_last_error()
    assert call(fo_=None, ws=d, ws_bytes=need) != 0 and b"null host" in lib.wfl_last_error()
    assert call(T_=np.array([-2], np.int32), ws=d, ws_bytes=need) != 0 and b"negative" in lib.wfl_last_error()
    assert call(fo_=np.array([-1], np.int64), ws=d, ws_bytes=need) != 0 and b"negative offset" in lib.wfl_last_error()
    assert call(logits=None, ws=d, ws_bytes=need) != 0 and b"null device" in lib.wfl_last_error()
    assert call(ids=None, ws=d, ws_bytes=need) != 0 and b"null device" in lib.wfl_last_error()
    assert call(score=None, ws=d, ws_bytes=need) != 0 and b"null device" in lib.wfl_last_error()
    assert call(pairs=None, ws=d, ws_bytes=need) != 0 and b"null device" in lib.wfl_last_error()
    assert call(ws=d, ws_bytes=need - 1) != 0 and b"workspace" in lib.wfl_last_error()
    assert call(ws=None, ws_bytes=need) != 0 and b"workspace" in lib.wfl_last_error()
    assert call(n=0) == 0                          # nothing to do


# ------------------------------------------------------------------------------------------------ 4. the public surface
def test_decode_option_on_the_public_surface():
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import infer as I
    for f in (I.infer_audio, I.infer_folder, I.Labeler.label_files):
        assert inspect.signature(f).parameters["decode"].default is None
        assert inspect.signature(f).parameters["switch_penalty"].default is None
    assert I.DECODE_MODES == ("argmax", "viterbi")
    with pytest.raises(ValueError, match="decode"):
        I.infer_audio("x.wav", decode="beam")
    with pytest.raises(ValueError, match="decode"):
        I.infer_folder("some_folder", decode="beam")
    with pytest.raises(ValueError, match="switch_penalty"):
        I.infer_audio("x.wav", decode="viterbi", switch_penalty=-1.0)
    with pytest.raises(ValueError, match="switch_penalty"):
        I.infer_folder("some_folder", switch_penalty="much")
    # (how the options are resolved against the config: tests/test_options_cpu.py)


def test_cli_takes_decode():
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import infer as I
    with pytest.raises(SystemExit) as e:
        I.main(["x.wav", "-ckpt", "m.pt", "-c", "c.yaml", "--decode", "beam"])
    assert e.value.code == 2                       # click: invalid choice, before anything is loaded
    with pytest.raises(SystemExit) as e:
        I.main(["x.wav", "-ckpt", "m.pt", "-c", "c.yaml", "-dec", "viterbi", "--switch-penalty", "-2"])
    assert e.value.code == 2                       # click.UsageError
