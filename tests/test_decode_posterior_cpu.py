"""CPU (-m "not gpu"): the numpy forward-backward over the BIO grammar (tests/bio_posterior_ref.py) against brute force and its
identities, the wfl_decode_posterior ABI's declarations, workspace rule and argument checks, the run scores of a path and the
`decode_scores` option, files and texts of the public surface."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import bio_posterior_ref as P
import bio_viterbi_ref as R

# C = 6: O, B-a, I-a, B-b without I-b, an orphan I-c (no B-c: never chosen) and a junk class
LABELS = ["O", "B-a", "I-a", "B-b", "I-c", "junk"]
O, Ba, Ia, Bb, Ic, JUNK = range(6)
TABLE = (O, [(Ba, Ia), (Bb, -1)])


# ------------------------------------------------------------------------------------------------ 1. the reference itself
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("lam", [0.0, 0.7])
@pytest.mark.parametrize("force", [False, True])
def test_float64_recurrence_equals_brute_force(T, lam, force):
    rng = np.random.default_rng(100 * T + int(10 * lam) + force)
    for _ in range(4):
        z = rng.standard_normal((T, 6)) * 2
        forced = np.zeros(T, bool)
        if force:
            forced[int(rng.integers(T))] = True
        ids, _ = R.viterbi(z, TABLE, lam, forced)
        assert P.path_is_legal(ids, TABLE, forced)
        bz, bp, bc = P.brute_force(z, TABLE, lam, forced, ids)
        logz, post, cls = P.forward_backward(z, TABLE, lam, forced, ids)
        assert abs(logz - bz) <= 1e-10
        assert np.abs(post - bp).max() <= 1e-10 and np.abs(cls - bc).max() <= 1e-10
        # the float32 restatement is the same recurrence
        l32, p32, c32 = P.forward_backward(z, TABLE, lam, forced, ids, dtype=np.float32)
        assert abs(l32 - bz) <= 1e-4 and np.abs(p32 - bp).max() <= 1e-4 and np.abs(c32 - bc).max() <= 1e-4


def test_path_is_legal_checks_the_grammar_and_the_forced_frames():
    assert P.path_is_legal([O, Ba, Ia, Ia, Bb, O], TABLE)
    assert not P.path_is_legal([O, Ia], TABLE)                  # I-a after O
    assert not P.path_is_legal([Ia], TABLE)                     # ... after the virtual O frame
    assert not P.path_is_legal([Bb, Ia], TABLE)                 # I-a after another phoneme
    assert not P.path_is_legal([Ba, Ic], TABLE) and not P.path_is_legal([JUNK], TABLE)
    assert P.path_is_legal([Ba, Ia], TABLE, [False, False]) and not P.path_is_legal([Ba, Ia], TABLE, [False, True])
    assert P.path_is_legal([Ba, O], TABLE, [False, True])


def _big_table(C=41, n_both=15, n_b_only=4):
    pairs = [(2 * p + 1, 2 * p + 2) for p in range(n_both)] + [(2 * n_both + 1 + q, -1) for q in range(n_b_only)]
    return C, (0, pairs)


@pytest.mark.parametrize("seed", range(4))
def test_invariants_on_random_and_planted_inputs(seed):
    C, table = _big_table()
    rng = np.random.default_rng(seed)
    lam = [0.0, 1.5, 2.0, 4.0][seed]
    thr = 0.5 if seed % 2 else 0.0
    for planted in (False, True):
        T = int(rng.integers(40, 120))
        z = R.plant(T, C, table, rng, margin=4.0)[0] if planted else (rng.standard_normal((T, C)) * 3).astype(np.float32)
        lse, forced, _ = R.prepass(z, thr)
        ids, obj = R.viterbi(z, table, lam, forced)
        logz, post, cls = P.forward_backward(z, table, lam, forced, ids)
        assert (cls >= 0).all() and (cls <= post + 1e-12).all() and (post <= 1 + 1e-12).all()
        assert logz >= R.objective(ids, z, table, lam, forced) - 1e-9        # logZ sums over every legal path, Viterbi's among them
        assert logz <= float(lse.sum()) + 1e-9                               # ... and over no more than every class string
        assert (post[forced] > 1 - 1e-12).all()                              # a forced frame is O on every path
        gO, gB, gI = P.forward_backward(z, table, lam, forced, ids, want_gamma=True)[3:]
        assert np.abs(gO + gB.sum(1) + gI.sum(1) - 1).max() <= 1e-9          # the posteriors of a frame's states sum to 1


def test_a_near_tie_is_kept_by_the_search_and_shown_by_the_posterior():
    """A planted run of phoneme 3 (B-3 = 7, I-3 = 8) at lambda = 2 with one frame whose two top classes are tied within 0.1.  Which
    frame: inside a run a tie cannot make the frame doubtful at this penalty, because leaving the run for one frame opens two runs
    (4 nats; the second case below shows the posterior saying just that); the frame a tie does make doubtful is the run's LAST one, tied
    between I-3 and the O that follows -- both readings open the same runs.  The Viterbi path keeps the frame in the run, its post is
    near 1/2, the run's other frames are sure."""
    C, table = _big_table()
    T, lam = 30, 2.0
    z = np.full((T, C), -6.0)
    ids = np.zeros(T, np.int32)
    ids[5], ids[6:25] = 7, 8
    z[np.arange(T), ids] = 6.0
    z[24, 0] = 5.95                                        # O on the run's last frame, 0.05 under I-3
    got, _ = R.viterbi(z, table, lam)
    assert (got == ids).all()
    logz, post, cls = P.forward_backward(z, table, lam, None, got)
    assert 0.3 < post[24] < 0.7, post[24]
    assert (post[5:24] > 0.99).all(), post[5:24].min()
    # the tie in the middle of the run, against another phoneme's B class: absorbed, and the posterior agrees with the search
    z[24, 0] = -6.0
    z[14, 11] = 5.95                                       # B-5
    got, _ = R.viterbi(z, table, lam)
    assert (got == ids).all()
    logz, post, cls = P.forward_backward(z, table, lam, None, got)
    assert (post[5:25] > 0.99).all(), post[5:25].min()


# ------------------------------------------------------------------------------------------------ 2. the ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import _lib
    return _lib.load()


def test_abi_declares_the_entries_and_the_workspace_rule(lib):
    from wfl_asr_amd import _lib
    for name in ("wfl_decode_posterior", "wfl_decode_posterior_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["wfl_decode_posterior"][1]) == 19
    r64 = lambda x: (x + 63) // 64 * 64    # noqa: E731
    h = lambda a: a.ctypes.data_as(ctypes.c_void_p)    # noqa: E731
    Ts = np.array([1500, 0, 1, 65], np.int32)
    want = 4 * sum(r64(3 * t) + 3 * r64(t) for t in Ts if t > 0)
    for n_pairs in (0, 3, 128, 129, 1024):
        assert lib.wfl_decode_posterior_workspace_bytes(h(Ts), len(Ts), n_pairs) == want
    assert lib.wfl_decode_posterior_workspace_bytes(h(Ts), len(Ts), 1025) == 0
    assert lib.wfl_decode_posterior_workspace_bytes(h(np.array([-1], np.int32)), 1, 70) < 0
    assert lib.wfl_decode_posterior_workspace_bytes(h(Ts), -1, 70) < 0 and lib.wfl_decode_posterior_workspace_bytes(h(Ts), 1, -1) < 0
    assert lib.wfl_decode_posterior_workspace_bytes(None, 1, 70) < 0 and lib.wfl_decode_posterior_workspace_bytes(None, 0, 70) == 0


def test_abi_argument_checks_touch_no_gpu(lib):
    buf = (ctypes.c_char * 64)()
    d = ctypes.cast(buf, ctypes.c_void_p)            # stands for a device pointer: every call below must fail before using it
    h = lambda a: a.ctypes.data_as(ctypes.c_void_p)    # noqa: E731
    T, fo = np.array([1500], np.int32), np.array([0], np.int64)

    def call(logits=d, ldl=141, C=141, o_id=0, fo_=fo, T_=T, n=1, pairs=d, n_pairs=70, lam=1.0, thr=0.0, ids=d, ws=d, ws_bytes=1 << 30,
             logz=d, post=d, cls=d, status=d):
        return lib.wfl_decode_posterior(logits, ldl, C, o_id, h(fo_) if fo_ is not None else None, h(T_) if T_ is not None else None, n,
                                        pairs, n_pairs, lam, thr, ids, ws, ws_bytes, logz, post, cls, status, None)
    need = lib.wfl_decode_posterior_workspace_bytes(h(T), 1, 70)
    for kw, word in ((dict(C=0), b"C < 1"), (dict(o_id=141), b"o_id"), (dict(o_id=-1), b"o_id"), (dict(ldl=100), b"ldl"),
                     (dict(n=-1), b"negative"), (dict(n_pairs=-1), b"negative"), (dict(lam=-1.0), b"lambda"),
                     (dict(lam=float("nan")), b"lambda"), (dict(thr=-0.1), b"threshold"), (dict(fo_=None), b"null host"),
                     (dict(T_=np.array([-5], np.int32)), b"negative"), (dict(fo_=np.array([-1], np.int64)), b"negative"),
                     (dict(ids=None), b"null device"), (dict(post=None), b"null device"), (dict(cls=None), b"null device"),
                     (dict(logz=None), b"null device"), (dict(status=None), b"null device"), (dict(pairs=None), b"null device"),
                     (dict(logits=None), b"null device"), (dict(ws_bytes=need - 1), b"workspace"), (dict(ws=None), b"workspace")):
        assert call(**kw) < 0, kw
        err = lib.wfl_last_error()
        assert b"wfl_decode_posterior" in err and word in err, (kw, err)
    assert call(n=0) == 0                            # an empty batch is fine and launches nothing


# ------------------------------------------------------------------------------------------------ 3. run scores and the public surface
@pytest.fixture(scope="module")
def table():
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import native_post as npost
    return npost.LabelTable(LABELS)


def test_run_scores_follow_the_segments_across_a_seam(table):
    from wfl_asr_amd import decode as DC
    fd = 0.02
    # chunk 0: O a a a | chunk 1 begins with I-a: ONE run over both chunks' frames; then b, one frame
    ids = [O, Ba, Ia, Ia] + [Ia, Ia, Bb, O]
    post = np.array([0.9, 0.8, 0.6, 1.0, 0.5, 0.7, 0.25, 0.95])
    cls = np.array([0.9, 0.4, 0.5, 0.9, 0.45, 0.6, 0.2, 0.95])
    plan = ([4, 4], [None, None], [0.0, 30.0])
    fs = DC.free_score(-10.0, -98.0, -90.0, post, cls, ids, *plan, table, fd)
    s, e, ph = DC.path_segments_free(ids, *plan, table, fd)
    assert len(fs.runs) == len(s) == 2
    assert [(r.start_s, r.end_s, r.phoneme) for r in fs.runs] == [(s[j], e[j], table.names[ph[j]]) for j in range(2)]
    a, b = fs.runs
    assert a.phoneme == "a" and a.posterior == pytest.approx(np.mean([0.8, 0.6, 1.0, 0.5, 0.7]))          # both chunks' frames
    assert a.start_posterior == 0.4 and a.min_frame_posterior == 0.5
    assert b.phoneme == "b" and b.posterior == 0.25 and b.start_posterior == 0.2 and b.min_frame_posterior == 0.25
    assert fs.min_posterior == 0.25
    assert fs.path_log_posterior == pytest.approx(-10.0 + -90.0 - -98.0) and fs.mean_frame_logprob == -10.0 / 8
    assert fs.legal_log_mass_per_frame == pytest.approx((-98.0 - -90.0) / 8)
    # the merge-map names, B-a right after I-a (a new run), a path without runs, a wrong length
    fs2 = DC.free_score(0, 0, 0, post[:4], cls[:4], [Ba, Ia, Ba, O], [4], [None], [0.0], table, fd, names=["x", "y", "z"])
    assert [r.phoneme for r in fs2.runs] == ["x", "x"] and fs2.runs[0].posterior == pytest.approx(0.85) and fs2.runs[1].posterior == 0.6
    assert DC.free_score(0, 0, 0, [1.0], [1.0], [O], [1], [None], [0.0], table, fd).min_posterior == 1.0
    with pytest.raises(ValueError):
        DC.free_score(0, 0, 0, post[:3], cls[:3], ids, *plan, table, fd)


def test_decode_scores_option_on_the_public_surface():
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import decode as DC
    from wfl_asr_amd import infer as I
    for f in (I.infer_audio, I.infer_folder, I.Labeler.label_files):
        assert inspect.signature(f).parameters["decode_scores"].default is None
    assert list(inspect.signature(DC.decode_posteriors).parameters) == ["logits", "n_frames", "table", "switch_penalty", "threshold", "ids",
                                                                       "frame_offsets", "stream"]
    assert DC.RunScore._fields == ("start_s", "end_s", "phoneme", "posterior", "start_posterior", "min_frame_posterior")
    assert DC.FreeScore._fields == ("path_log_posterior", "mean_frame_logprob", "legal_log_mass_per_frame", "min_posterior", "runs")
    with pytest.raises(ValueError, match="decode_scores"):
        I.infer_audio("x.wav", decode="argmax", decode_scores=True)
    with pytest.raises(ValueError, match="decode_scores"):
        I.infer_folder("some_folder", decode="argmax", decode_scores=True)
    # (how the option is resolved against the config: tests/test_options_cpu.py)


def test_the_texts_of_both_files():
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import decode as DC
    from wfl_asr_amd import infer as I
    runs = [DC.RunScore(0.03, 0.25, "a", 0.75, 0.5, 0.125), DC.RunScore(0.25, 1.0, "sh", 1.0, 0.999999, 0.9999996)]
    fs = DC.FreeScore(-2.25, -0.5, -0.125, 0.75, runs)
    note = "runs are the path's runs before merge_segments and any transcript match"
    assert I.format_decode_scores_tsv(fs, 1) == (
        "# path_log_posterior=-2.2500\tmean_frame_logprob=-0.500000\tlegal_log_mass_per_frame=-0.125000\tmin_posterior=0.750000\t"
        "runs=2 lab_lines=1\t" + note + "\n"
        "300000\t2500000\ta\t0.750000\t0.500000\t0.125000\n"
        "2500000\t10000000\tsh\t1.000000\t0.999999\t1.000000\n")
    assert I.format_decode_scores_tsv(DC.FreeScore(0.0, 0.0, 0.0, 1.0, []), 0) == (
        "# path_log_posterior=0.0000\tmean_frame_logprob=0.000000\tlegal_log_mass_per_frame=0.000000\tmin_posterior=1.000000\t"
        "runs=0 lab_lines=0\t" + note + "\n")
    weak, sure = fs._replace(min_posterior=0.01), fs._replace(min_posterior=0.9, runs=runs[:1])
    assert I.format_decode_review_tsv([("m.wav", fs), ("z.wav", weak), ("a.wav", sure), ("b.wav", weak)]) == (
        "# file\tmin_posterior\tpath_log_posterior\tmean_frame_logprob\tlegal_log_mass_per_frame\truns\n"
        "b.wav\t0.010000\t-2.2500\t-0.500000\t-0.125000\t2\n"
        "z.wav\t0.010000\t-2.2500\t-0.500000\t-0.125000\t2\n"
        "m.wav\t0.750000\t-2.2500\t-0.500000\t-0.125000\t2\n"
        "a.wav\t0.900000\t-2.2500\t-0.500000\t-0.125000\t1\n")
    assert I.decode_scores_path("out/x.lab") == os.path.join("out", "x.decode_scores.tsv")
