"""Single-insertion scores of a transcript (wfl_align_insertions, `postprocess.align_insertions`), without a GPU:

  1. the closed form of tests/align_insertions_ref.py against the DEFINITION, logZ of every transcript with one token inserted by
     posterior_ref.forward_backward (windows through viterbi_window_ref), to 1e-9 in float64, the -inf patterns identical
  2. the identity that ties the insertions to the edits: inserting a deleted token again is minus its deletion
  3. host logic: the option and its rule 13, the parameter's place, PlaceInsertion rows through a merge map, the TSV writers, the ABI's
     declarations and argument checks, the workspace rule
"""
import ctypes
import inspect

import numpy as np
import pytest

import align_edits_ref as E
import align_insertions_ref as R
import test_align_edits_cpu as CPU

C, PH, GAPS = CPU.C, CPU.PH, CPU.GAPS
_tiny = CPU._tiny


# ------------------------------------------------------------------------------------------------ 1. closed form == definition
def _against_definition(z, alts, wins, gaps=GAPS):
    """-> (finite entries, -inf entries)"""
    got = R.insertion_scores(z, alts, gaps, PH, wins)
    want = R.by_definition(z, alts, gaps, PH, wins)
    assert got is not None and want is not None
    assert got["ins"].shape == (len(alts) + 1, len(PH))
    fin = np.isfinite(want["ins"])
    assert (np.isfinite(got["ins"]) == fin).all()
    assert (got["ins"][~fin] == -np.inf).all()
    assert abs(got["logz"] - want["logz"]) <= 1e-9
    err = float(np.abs(got["ins"][fin] - want["ins"][fin]).max()) if fin.any() else 0.0
    assert err <= 1e-9, err
    # the float32 restatement follows (it is the GPU test's yardstick, not a reference)
    r32 = R.insertion_scores(z, alts, gaps, PH, wins, dtype=np.float32)
    assert (np.isfinite(r32["ins"]) == fin).all()
    if fin.any():
        assert np.abs(r32["ins"][fin] - want["ins"][fin]).max() < 1e-3
    return int(fin.sum()), int((~fin).sum())


@pytest.mark.parametrize("T", [1, 3])
def test_no_token_has_one_place(T):
    n_fin, n_inf = _against_definition(*_tiny(T, 0, T))
    assert (n_fin, n_inf) == (len(PH), 0)


@pytest.mark.parametrize("N", [1, 2, 3, 5])
def test_as_many_tokens_as_frames_leaves_no_frame_to_insert_into(N):
    n_fin, n_inf = _against_definition(*_tiny(10 + N, N, N))
    assert (n_fin, n_inf) == (0, (N + 1) * len(PH))


@pytest.mark.parametrize("N", [1, 2, 4, 6])
def test_one_frame_to_spare_and_more(N):
    """T = N + 1 (every place has exactly one frame), then longer clips; N = 1 among them.  Unwindowed with T >= N + 1: no -inf."""
    for seed, T in enumerate([N + 1, N + 3, 13, 17]):
        n_fin, n_inf = _against_definition(*_tiny(20 * N + seed, N, T))
        assert n_inf == 0 and n_fin == (N + 1) * len(PH)


def test_tokens_with_two_to_four_alternatives_a_repeated_token_and_two_gap_classes():
    for seed in range(4):
        assert _against_definition(*_tiny(100 + seed, 4, 10, n_alt=(2, 4)))[1] == 0
        assert _against_definition(*_tiny(200 + seed, 4, 9, equal_neighbours=True))[1] == 0
        assert _against_definition(*_tiny(300 + seed, 3, 8, n_alt=(1, 2)), gaps=[0, 9])[1] == 0     # (9: a class no phoneme of PH[:4] uses as I)


def _windowed(seed, N, T, half_width):
    """Windows of one half-width around centres drawn WITH replacement: around increasing distinct starts (_tiny's windows) a half-width
    >= 1 always leaves the new token a frame (shift the tokens up to the nearest gap frame by one), so no entry would be -inf."""
    z, alts, _ = _tiny(seed, N, T, n_alt=(1, 2))
    centres = np.sort(np.random.default_rng(1000 + seed).integers(0, T, N))
    return z, alts, [(int(c) - half_width, int(c) + half_width) for c in centres]


# (seed, N, T) at which the transcript has a path and the reference holds both finite and -inf entries: found once by running the
# reference over seeds 400 .. 439, not by looking at any kernel
@pytest.mark.parametrize("half_width,seed,N,T", [(2, 430, 5, 8), (2, 431, 5, 8), (2, 400, 6, 9), (2, 417, 6, 9),
                                                 (0, 400, 3, 9), (0, 409, 3, 9), (0, 419, 3, 9), (0, 400, 4, 12), (0, 405, 4, 12)])
def test_windows_of_half_width_two_and_zero(half_width, seed, N, T):
    n_fin, n_inf = _against_definition(*_windowed(seed, N, T, half_width))
    assert n_fin > 0 and n_inf > 0


def test_open_windows_are_no_windows_and_transcripts_without_a_path():
    z, alts, wins = _tiny(7, 3, 9, windows="open")
    assert np.array_equal(R.insertion_scores(z, alts, GAPS, PH, wins)["ins"], R.insertion_scores(z, alts, GAPS, PH)["ins"])
    z, alts, _ = _tiny(1, 3, 2)
    assert R.insertion_scores(z, alts, GAPS, PH) is None and R.by_definition(z, alts, GAPS, PH) is None        # T < N
    z, alts, _ = _tiny(2, 2, 6)
    assert R.insertion_scores(z, alts, GAPS, PH, [(3, 3), (3, 3)]) is None                                     # two starts on one frame
    assert R.insertion_scores(z, alts, GAPS, [])["ins"].shape == (3, 0)                                         # an empty table


# ------------------------------------------------------------------------------------------------ 2. the identity
@pytest.mark.parametrize("seed", range(4))
def test_inserting_a_deleted_token_again_is_minus_its_deletion(seed):
    """Token k has the single alternative PH[p]: the transcript without k, with PH[p] inserted at place k, is the transcript."""
    rng = np.random.default_rng(seed)
    N, T = 5, 14
    alts = [[PH[int(p)]] for p in rng.integers(0, 5, N)]
    z = (rng.standard_normal((T, C)) * 3).astype(np.float32)
    edits = E.edit_scores(z, alts, GAPS, PH)["edits"]
    for k in range(N):
        ins = R.insertion_scores(z, alts[:k] + alts[k + 1:], GAPS, PH)["ins"]
        assert abs(ins[k, PH.index(alts[k][0])] + edits[k, len(PH)]) <= 1e-9


# ------------------------------------------------------------------------------------------------ 3. host logic
def test_option_rule_13():
    from wfl_asr_amd.options import PostOptions, resolve
    assert resolve({}).align_insertions is False
    assert resolve({}) == ("greedy", False, "argmax", 0.0, False, None, 1.0, False)       # defaults equal the plain eight-tuple
    assert hash(resolve({})) == hash(("greedy", False, "argmax", 0.0, False, None, 1.0, False))
    a = resolve({"align": "viterbi", "align_insertions": True})                           # the config key
    assert a.align_insertions is True and a != resolve({"align": "viterbi"}) and "align_insertions=True" in repr(a)
    assert a != tuple(a) and a.align_edits is False
    assert resolve({"align": "viterbi", "align_insertions": True}, align_insertions=False).align_insertions is False
    assert resolve({"align": "viterbi"}, align_insertions=True).align_insertions is True
    assert a._asdict()["align_insertions"] is True and a._replace(align_scores=True).align_insertions is True
    assert a._replace(align_insertions=False) == resolve({"align": "viterbi"})
    assert PostOptions._make(tuple(a), align_insertions=True) == a
    assert isinstance(a, PostOptions) and hash(a) != hash(resolve({"align": "viterbi"}))
    assert a != resolve({"align": "viterbi", "align_edits": True})
    with pytest.raises(AttributeError):
        a.align_insertions = False
    with pytest.raises(ValueError, match="align_insertions needs align='viterbi'"):
        resolve({}, align_insertions=True)
    with pytest.raises(ValueError, match="align_insertions needs align='viterbi'"):
        resolve({"align_insertions": True, "align": "greedy"})
    with pytest.raises(ValueError, match="align_edits needs align='viterbi'"):            # the earlier rule is reported
        resolve({"align": "greedy"}, align_edits=True, align_insertions=True)


def test_the_parameter_follows_align_edits_and_the_cli_flag_reaches_the_record(monkeypatch, tmp_path):
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import infer as I

    def no_load(*a, **k):
        raise AssertionError("a model was loaded before the options were refused")
    for f in (I.infer_audio, I.infer_folder, I.Labeler.label_files):
        names = list(inspect.signature(f).parameters)
        assert inspect.signature(f).parameters["align_insertions"].default is None
        assert names.index("align_insertions") == names.index("align_edits") + 1 and names[-1] == "bigram_scores"
    monkeypatch.setattr(I, "_labeler", no_load)
    monkeypatch.setattr(I, "Labeler", no_load)
    with pytest.raises(ValueError, match="align_insertions needs align='viterbi'"):
        I.infer_audio("x.wav", align_insertions=True)
    cfg = tmp_path / "config.yaml"
    cfg.write_text("postprocess:\n  align: greedy\n  align_insertions: true\n")
    with pytest.raises(ValueError, match="align_insertions needs align='viterbi'"):
        I.infer_folder("some_folder", config_path=str(cfg))
    seen = {}

    def record(*a, **k):
        seen.update(k)
        raise SystemExit(0)
    monkeypatch.setattr(I.torch.cuda, "is_available", lambda: True)     # (the CLI turns away a machine without a device first)
    monkeypatch.setattr(I, "infer_audio", record)
    monkeypatch.setattr(I, "infer_folder", record)
    wav = tmp_path / "x.wav"
    wav.write_bytes(b"")
    ckpt = tmp_path / "m.pt"
    ckpt.write_bytes(b"")
    cfg.write_text("postprocess:\n  align: viterbi\n")
    with pytest.raises(SystemExit):
        I.main([str(wav), "-ckpt", str(ckpt), "-c", str(cfg), "--align-insertions"])
    assert seen.get("align_insertions") is True and seen.get("align_edits") is False


def test_place_insertions_through_a_merge_map():
    from wfl_asr_amd import align as AL
    table, labels = CPU._table(["a", "b", "c", "d"])
    sub_names, _ = AL.substitute_table(labels)
    names = ["a", "bc", "d"]                               # b and c are merged into one output name "bc"
    remap = np.array([{"a": 0, "b": 1, "c": 1, "d": 2}[n] for n in table.names])
    out = AL.substitute_output_names(sub_names, table, remap, names)
    assert out == ["a", "bc", "bc", "d"]
    segs = [(0.25, 0.5, "a"), (0.5, 0.75, "bc")]
    ins = np.array([[9.0, -1.0, 2.0, -3.0],                # a neighbour's own name is a hypothesis like any other: "a" in front of "a"
                    [1.0, 7.0, 8.0, 8.0],                  # bc stands with its better member (8.0), and wins the tie with d: table order
                    [-np.inf, -np.inf, -np.inf, -np.inf]], np.float32)
    rows = AL.place_insertions(ins, segs, out)
    assert [(r.index, r.after, r.before, r.at_s) for r in rows] == [(0, "", "a", 0.25), (1, "a", "bc", 0.5), (2, "bc", "", 0.75)]
    assert [(r.best, r.best_ratio, r.second, r.second_ratio) for r in rows] == [("a", 9.0, "bc", 2.0), ("bc", 8.0, "d", 8.0),
                                                                                ("a", -np.inf, "bc", -np.inf)]
    assert [r.flag for r in rows] == [1, 1, 0]
    with pytest.raises(ValueError):
        AL.place_insertions(ins[:, :3], segs, out)
    with pytest.raises(ValueError):
        AL.place_insertions(ins[:2], segs, out)            # N + 1 rows
    only = AL.place_insertions(np.array([[0.5]]), [], ["a"])[0]                            # no token: one place, no neighbours
    assert (only.index, only.after, only.before, only.at_s, only.best, only.second, only.second_ratio, only.flag) == \
        (0, "", "", 0.0, "a", "", -np.inf, 1)
    none = AL.place_insertions(np.zeros((2, 0)), segs[:1], [])                              # an empty table
    assert [(r.best, r.best_ratio, r.flag) for r in none] == [("", -np.inf, 0)] * 2


def test_the_tsv_writers_and_the_folder_files_order(tmp_path):
    from wfl_asr_amd import align as AL
    from wfl_asr_amd import reports as RP
    mk = lambda i, best: AL.PlaceInsertion(i, "p", "q", 0.1 * i, "x", best, "y", best - 1, int(best > 0))      # noqa: E731
    a = [mk(0, -1.0), mk(1, 3.0), mk(2, 0.5)]
    b = [mk(0, 3.0), mk(1, -np.inf), mk(2, 7.0)]
    (tmp_path / "a.insertions.tsv").write_text(RP.file_text("insertions", a))
    lines = (tmp_path / "a.insertions.tsv").read_text().split("\n")
    assert lines[0] == RP.REPORTS["insertions"].header and lines[0].split("\t") == ["index", "after", "before", "at_s", "best", "best_log_ratio",
                                                                         "second", "second_log_ratio", "flag"]
    assert len(lines) == 5 and lines[4] == ""
    assert lines[2].split("\t") == ["1", "p", "q", "0.1000000", "x", "3", "y", "2", "1"]
    rows = RP.folder_rows("insertions", [("a.wav", a), ("b.wav", b)])
    # the flagged places, largest ratio first; the tie at 3.0 in file order
    assert [(n, r.index) for n, r in rows] == [("b.wav", 2), ("a.wav", 1), ("b.wav", 0), ("a.wav", 2)]
    assert [(n, r.index) for n, r in RP.folder_rows("insertions", [("a.wav", [mk(0, 2.0), mk(1, 2.0)])])] == [("a.wav", 0), ("a.wav", 1)]
    (tmp_path / "transcript_insertions.tsv").write_text(RP.folder_text("insertions", [("a.wav", a), ("b.wav", b)]))
    lines = (tmp_path / "transcript_insertions.tsv").read_text().split("\n")
    assert lines[0] == "file\t" + RP.REPORTS["insertions"].header and [ln.split("\t")[0] for ln in lines[1:5]] == ["b.wav", "a.wav", "b.wav", "a.wav"]
    assert lines[1].split("\t")[-4:] == ["7", "y", "6", "1"] and len(lines) == 6
    (tmp_path / "e.insertions.tsv").write_text(RP.file_text("insertions", [b[1]]))
    assert (tmp_path / "e.insertions.tsv").read_text().split("\n")[1].split("\t")[4:] == ["x", "-inf", "y", "-inf", "0"]
    assert f"{float('-inf'):.6g}" == str(float("-inf"))    # (-inf as written by Python)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import _lib
    return _lib.load()


def test_symbols_are_declared_and_exported(lib):
    import os
    from wfl_asr_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wfl_asr.h")).read()
    for name in ("wfl_align_insertions", "wfl_align_insertions_workspace_bytes"):
        assert name + "(" in src and name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.SIGNATURES["wfl_align_insertions"] == _lib.SIGNATURES["wfl_align_edits"]            # the edits entry's arguments
    assert "tok_off_host[b] + b + j" in src and "clip order" in src                                  # the row rule and what it rests on


def test_workspace_rule_and_groups(lib):
    from wfl_asr_amd import align as AL
    r64 = lambda x: (x + 63) // 64 * 64                   # noqa: E731

    def words(T, N):
        W = r64(min(N, 4096) + 1)
        return 0 if T == 0 else 64 + r64(T) + r64(2 * (T + 1)) + r64(2 * T) + r64((T + 1) * W) + r64(T * W)
    assert [AL.insertions_workspace_bytes([T], [N]) for T, N in ((0, 0), (5, 0), (70, 63), (70, 64))] == [0, 3840, 38400, 74496]
    for T, N in ((0, 0), (5, 0), (70, 63), (70, 64), (1500, 300), (15000, 4096), (20, 5000)):
        assert AL.insertions_workspace_bytes([T], [N]) == 4 * words(T, N), (T, N)
    assert AL.insertions_workspace_bytes([1500, 60], [300, 7]) == 4 * (words(1500, 300) + words(60, 7))
    assert AL.insertions_workspace_bytes([15000], [4096]) < AL.EDITS_WORKSPACE_LIMIT
    assert lib.wfl_align_insertions_workspace_bytes(None, None, 0) == 0 and lib.wfl_align_insertions_workspace_bytes(None, None, 1) == -1
    with pytest.raises(Exception, match="negative"):
        AL.insertions_workspace_bytes([-1], [0])
    # the groups go by the call's own rule; the default is edit_scores'
    one = AL.insertions_workspace_bytes([70], [63])
    assert one < AL.edits_workspace_bytes([70], [63])      # (no D plane)
    assert AL.edit_groups([70] * 3, [63] * 3, limit=2 * one) == [[0], [1], [2]]
    assert AL.edit_groups([70] * 5, [63] * 5, limit=2 * one, workspace_bytes=AL.insertions_workspace_bytes) == [[0, 1], [2, 3], [4]]
    assert AL.edit_groups([70] * 3, [64] * 3, limit=2 * one, workspace_bytes=AL.insertions_workspace_bytes) == [[0], [1], [2]]
    assert AL.edit_groups([70] * 3, [63] * 3, limit=2 * AL.edits_workspace_bytes([70], [63])) == [[0, 1], [2]]


def test_arguments_are_checked_on_the_host(lib):
    Pv = ctypes.c_void_p
    buf = (ctypes.c_char * 64)()
    d = ctypes.cast(buf, Pv)                               # never dereferenced: every call below fails on the host
    fo, ko = np.zeros(1, np.int64), np.zeros(1, np.int32)
    T, N = np.array([10], np.int32), np.array([3], np.int32)
    h = lambda a: a.ctypes.data_as(Pv)                     # noqa: E731
    need = lib.wfl_align_insertions_workspace_bytes(h(T), h(N), 1)

    def call(C=141, n_sub=5, sub=d, ws_bytes=need, ins=d, n_clips=1, Tn=T, Nn=N, fo_=fo):
        return lib.wfl_align_insertions(d, 141, C, 0, h(fo_), h(Tn), h(ko), h(Nn), d, None, d, n_clips, sub, n_sub, d, ws_bytes, d, ins, d,
                                        None)
    assert call(n_sub=513) == -1 and b"wfl_align_insertions: n_sub" in lib.wfl_last_error()
    assert call(n_sub=-1) == -1
    assert call(sub=None) == -1 and b"wfl_align_insertions: null device" in lib.wfl_last_error()
    assert call(ins=None) == -1
    assert call(C=0) != 0 and b"wfl_align_insertions: C must" in lib.wfl_last_error()
    assert call(ws_bytes=need - 1) != 0 and b"workspace" in lib.wfl_last_error()
    assert call(n_clips=-1) != 0 and b"n_clips" in lib.wfl_last_error()
    assert call(Tn=np.array([-1], np.int32)) != 0 and b"negative" in lib.wfl_last_error()
    assert call(Nn=np.array([-3], np.int32)) != 0 and b"negative" in lib.wfl_last_error()
    assert lib.wfl_align_insertions(d, 141, 141, 0, None, None, None, None, None, None, d, 1, d, 1, d, need, d, d, d, None) == -1
    assert b"null host array" in lib.wfl_last_error()
    assert lib.wfl_align_insertions(d, 141, 141, 0, None, None, None, None, None, None, d, 0, None, 0, None, 0, d, d, d, None) == 0   # no clip
