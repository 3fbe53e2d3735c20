"""CPU (-m "not gpu"): the definition of the alignment posteriors (tests/posterior_ref.py against brute-force enumeration of every
accepted path), identities of the reference, the wfl_align_posterior ABI's declarations, workspace rule and argument checks, the
`align_scores` option of the public surface and its writers, and the inputs of the GPU discrimination check."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import posterior_ref as P
import viterbi_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tok(z, alts, gaps):
    states, score = V.viterbi(z, alts, gaps)
    return V.outputs(states, z, alts, 0)[1], score


# ------------------------------------------------------------------------------------------------ 1. the definition
@pytest.mark.parametrize("seed", range(6))
def test_forward_backward_equals_brute_force_on_tiny_cases(seed):
    rng = np.random.default_rng(seed)
    C = 9
    for _ in range(25):
        N = int(rng.integers(0, 4))
        T = int(rng.integers(max(N, 1), 8 if N < 3 else 7))
        alts = [[(1 + 2 * int(p), 2 + 2 * int(p)) for p in rng.choice(3, size=int(rng.integers(1, 3)), replace=False)] for _ in range(N)]
        gaps = [0] if rng.random() < 0.5 else [0, 7, 8]
        z = rng.standard_normal((T, C)) * 2
        tok, _ = _tok(z, alts, gaps)
        a = P.forward_backward(z, alts, gaps, tok=tok, want_gamma=True)
        b = P.brute_force(z, alts, gaps, tok=tok)
        assert abs(a["logz"] - b["logz"]) < 1e-10
        for k in ("gG", "gB", "gI", "tok_post", "start_mean", "start_sd"):
            assert np.abs(np.asarray(a[k]) - np.asarray(b[k])).max(initial=0) < 1e-7, k        # (sd: a square root of ~1e-15 is 3e-8)


def test_identities_of_the_reference():
    rng = np.random.default_rng(1)
    C, gaps = 141, [0, 137, 138]
    for T, N, boost in ((60, 10, 4.0), (300, 80, 0.0), (500, 120, 4.0)):
        alts = [[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 68, N)]
        z = P.planted_logits(T, N, C, alts, gaps, rng, boost)
        tok, score = _tok(z, alts, gaps)
        r = P.forward_backward(z, alts, gaps, tok=tok, want_gamma=True)
        assert np.abs(r["gB"].sum(0) - 1).max() < 1e-9                      # a path visits B_k in exactly one frame
        assert np.abs(r["gG"].sum(1) + r["gB"].sum(1) + r["gI"].sum(1) - 1).max() < 1e-9
        assert r["logz"] >= score - 1e-9
        assert (r["tok_post"] >= 0).all() and (r["tok_post"] <= 1 + 1e-12).all()
        r32 = P.forward_backward(z, alts, gaps, tok=tok, dtype=np.float32)
        assert abs(r32["logz"] - r["logz"]) < 1e-3 and np.abs(r32["tok_post"] - r["tok_post"]).max() < 1e-3
    for N in (1, 7, 40):                                                      # as many tokens as frames: one path
        alts = [[(int(2 * p - 1), int(2 * p))] for p in rng.integers(1, 68, N)]
        z = P.planted_logits(N, N, C, alts, gaps, rng, 0.0)
        tok, score = _tok(z, alts, gaps)
        r = P.forward_backward(z, alts, gaps, tok=tok)
        assert np.abs(r["tok_post"] - 1).max() < 1e-9 and r["start_sd"].max() < 1e-6 and np.abs(r["start_mean"]).max() < 1e-9
        assert abs(r["logz"] - score) < 1e-9
    assert P.forward_backward(np.zeros((2, 5)), [[(1, 2)]] * 3, [0]) is None


def test_discrimination_inputs_on_the_float64_reference():
    """The GPU test asserts logz(planted transcript) > logz(two neighbours swapped) on these inputs; here the float64 reference
    shows the gap is there (tens of nats), so the choice of inputs does not rest on the kernel."""
    from test_gpu_align_posterior import discrimination_case
    for seed in range(4):
        z, alts, sw = discrimination_case(seed)
        a = P.forward_backward(z, alts, [0])["logz"]
        b = P.forward_backward(z, sw, [0])["logz"]
        assert a - b > 5.0, (seed, a, b)


# ------------------------------------------------------------------------------------------------ 2. ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import _lib
    return _lib.load()


def test_posterior_symbols_are_declared_bound_and_exported(lib):
    from wfl_asr_amd import _lib
    src = open(os.path.join(ROOT, "include", "wfl_asr.h")).read()
    for name in ("wfl_align_posterior", "wfl_align_posterior_workspace_bytes"):
        assert name + "(" in src and name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert len(_lib.SIGNATURES["wfl_align_posterior"][1]) == 20


def _ws(lib, T, N):
    t, n = np.array([T], np.int32), np.array([N], np.int32)
    return lib.wfl_align_posterior_workspace_bytes(t.ctypes.data_as(ctypes.c_void_p), n.ctypes.data_as(ctypes.c_void_p), 1)


def test_posterior_workspace_rules_out_the_lattice_and_is_monotone(lib):
    cap = _ws(lib, 15000, 4096)
    assert 0 < cap <= 64 * 2 ** 20                        # the lattice itself would be 15000 x 12289 x 4 = 737 MB
    assert cap >= 4 * 3 * 4097 * (128 + 15000 // 128)     # one block of alpha and the checkpoints do not fit in less
    Ts = [1, 2, 100, 128, 129, 1500, 6000, 15000, 40000]
    Ns = [0, 1, 127, 128, 300, 511, 512, 1023, 1024, 2047, 2048, 4096, 5000]
    grid = np.array([[_ws(lib, T, N) for N in Ns] for T in Ts])
    assert (grid > 0).all() and (np.diff(grid, axis=0) >= 0).all() and (np.diff(grid, axis=1) >= 0).all()
    assert _ws(lib, 0, 5) == 0 and _ws(lib, -1, 5) < 0 and _ws(lib, 5, -1) < 0
    both = lib.wfl_align_posterior_workspace_bytes(np.array([1500, 60], np.int32).ctypes.data_as(ctypes.c_void_p),
                                                   np.array([300, 10], np.int32).ctypes.data_as(ctypes.c_void_p), 2)
    assert both == _ws(lib, 1500, 300) + _ws(lib, 60, 10)
    assert lib.wfl_align_posterior_workspace_bytes(None, None, 0) == 0


def test_posterior_validates_its_arguments_without_gpu(lib):
    P_ = ctypes.c_void_p
    buf = (ctypes.c_char * 64)()
    d = ctypes.cast(buf, P_)                       # never dereferenced: every call below fails on the host
    fo = np.zeros(1, np.int64)
    T = np.array([10], np.int32)
    ko = np.zeros(1, np.int32)
    N = np.array([3], np.int32)
    h = lambda a: a.ctypes.data_as(P_)             # noqa: E731

    def call(C=141, o_id=0, ldl=141, fo_=fo, T_=T, N_=N, ws=None, ws_bytes=0, logits=d, n=1, tok=d, tok_post=d):
        return lib.wfl_align_posterior(logits, ldl, C, o_id, h(fo_) if fo_ is not None else None, h(T_), h(ko), h(N_), d, d, n, tok, ws,
                                       ws_bytes, d, tok_post, d, d, d, None)

    need = lib.wfl_align_posterior_workspace_bytes(h(T), h(N), 1)
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
    assert call(tok=None, ws=d, ws_bytes=need) != 0 and b"null device" in lib.wfl_last_error()
    assert call(tok_post=None, ws=d, ws_bytes=need) != 0 and b"null device" in lib.wfl_last_error()
    assert call(ws=d, ws_bytes=need - 1) != 0 and b"workspace" in lib.wfl_last_error()
    assert call(ws=None, ws_bytes=need) != 0 and b"workspace" in lib.wfl_last_error()
    assert b"wfl_align_posterior" in lib.wfl_last_error()
    assert call(n=0) == 0                          # nothing to do


# ------------------------------------------------------------------------------------------------ 3. the public surface
def test_align_scores_option_on_the_public_surface():
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import align as AL
    from wfl_asr_amd import infer as I
    for f in (I.infer_audio, I.infer_folder, I.Labeler.label_files):
        assert inspect.signature(f).parameters["align_scores"].default is None
    sig = inspect.signature(AL.alignment_posteriors)
    assert list(sig.parameters) == ["logits", "n_frames", "token_classes", "gap_classes", "o_id", "tok", "frame_offsets", "stream", "packed"]
    with pytest.raises(ValueError, match="align_scores"):
        I.infer_audio("x.wav", align="greedy", align_scores=True)
    with pytest.raises(ValueError, match="align_scores"):
        I.infer_folder("some_folder", align="greedy", align_scores=True)
    # (how the option is resolved against the config: tests/test_options_cpu.py)


def test_cli_takes_align_scores(capsys):
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import infer as I
    with pytest.raises(SystemExit) as e:
        I.main(["--help"])
    assert e.value.code == 0 and "--align-scores" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        I.main(["x.wav", "-ckpt", "m.pt", "-c", "c.yaml", "--align-scores", "--align", "dtw"])
    assert e.value.code == 2


def test_file_score_and_the_tsv_writers():
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import align as AL
    from wfl_asr_amd import infer as I
    from wfl_asr_amd import native_post as npost
    from wfl_asr_amd import postprocess as pp
    segs = [(0.1234567891, 0.5, "a"), (0.5, 1.7000000049, "b"), (2.02, 2.04, "a")]
    fs = AL.file_score(-120.5, -118.25, 150, [0.75, 0.999, 0.125], [0.5, 0.0, -2.0], [1.5, 0.0, 3.0], segs, pp.FRAME_DURATION)
    assert isinstance(fs, AL.FileScore) and fs._fields == ("path_log_posterior", "mean_frame_logprob", "mean_frame_logz",
                                                            "min_posterior", "tokens")
    assert AL.TokenScore._fields == ("token", "start_s", "end_s", "posterior", "start_sd_s", "start_shift_s")
    assert fs.path_log_posterior == -2.25 and fs.mean_frame_logprob == -120.5 / 150 and fs.mean_frame_logz == -118.25 / 150
    assert fs.min_posterior == 0.125 and [t.token for t in fs.tokens] == ["a", "b", "a"]
    assert fs.tokens[0].start_sd_s == pytest.approx(1.5 * 0.02) and fs.tokens[2].start_shift_s == pytest.approx(-2.0 * 0.02)
    assert [(t.start_s, t.end_s) for t in fs.tokens] == [(s, e) for s, e, _ in segs]
    with pytest.raises(ValueError):
        AL.file_score(-1, -1, 10, [0.5], [0.0], [0.0], segs, 0.02)
    text = I.format_scores_tsv(fs)
    lines = text.split("\n")
    assert text.endswith("\n") and len(lines) == 5 and lines[0].startswith("# ")
    head = dict(kv.split("=") for kv in lines[0][2:].split("\t"))
    assert list(head) == ["path_log_posterior", "mean_frame_logprob", "mean_frame_logz", "min_posterior"]
    assert float(head["path_log_posterior"]) == -2.25 and float(head["min_posterior"]) == 0.125
    lab = npost.format_lab_tuples(segs).decode().split("\n")
    for ln, lab_ln, t in zip(lines[1:4], lab, fs.tokens):
        f = ln.split("\t")
        assert len(f) == 6 and f[:2] == lab_ln.split()[:2] and f[2] == lab_ln.split()[2] == t.token      # the .lab line's integers
        assert float(f[3]) == pytest.approx(t.posterior, abs=1e-6) and float(f[4]) == pytest.approx(t.start_sd_s, abs=1e-4)
        assert float(f[5]) == pytest.approx(t.start_shift_s, abs=1e-4)
    weak = fs._replace(min_posterior=0.01)
    sure = fs._replace(min_posterior=0.9)
    review = I.format_review_tsv([("m.wav", fs), ("z.wav", weak), ("a.wav", sure), ("b.wav", weak)]).split("\n")
    assert review[0].startswith("#")
    assert [r.split("\t")[0] for r in review[1:5]] == ["b.wav", "z.wav", "m.wav", "a.wav"]                  # the weakest first
    assert [float(r.split("\t")[1]) for r in review[1:5]] == [0.01, 0.01, 0.125, 0.9]
    assert I.scores_path("out/x.lab") == os.path.join("out", "x.scores.tsv")
