"""CPU (-m "not gpu"): the definition of the posteriors over the minimum-duration lattice (tests/duration_posterior_ref.py against the
enumeration of every accepted path, against posterior_ref for D = 1, and the identity gamma(H^j) = shifted gamma(B)), the option rules
of `postprocess.duration_scores`, the signatures, the ABI entry's checks and duration_posteriors' refusal."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest

import duration_posterior_ref as DP
import posterior_ref as P
import viterbi_min_ref as M
import viterbi_window_ref as W


@pytest.fixture(scope="module")
def AL():
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import align
    return align


def _window_sets(T, N, rng):
    yield None
    for width in (4, 2):                           # wide windows (mostly feasible), then narrow ones
        wins = []
        for k in range(N):
            lo = int(rng.integers(-1, max(T // 2, 1))) + k
            wins.append((lo, lo + int(rng.integers(0, width))))
        yield wins


# ------------------------------------------------------------------------------------------------ 1. the definition
def test_reference_equals_enumeration():
    """T <= 7, N <= 3, D mixes of 1, 2 and 3, with and without windows: logz, every gamma, the three per-token outputs."""
    rng = np.random.default_rng(83)
    C = 11
    checked = none = chained = 0
    for T, N in itertools.product(range(1, 8), range(0, 4)):
        alts = [[(1 + 2 * k, 2 + 2 * k)] for k in range(N)]
        mixes = list(itertools.product((1, 2, 3), repeat=N))
        for D in mixes:
            z = rng.standard_normal((T, C)) * 2.0
            for wins in _window_sets(T, N, rng):
                open_w = wins if wins is not None else [W.OPEN] * N
                path, _ = M.viterbi(z, alts, [0, 9], D, windows=wins)
                bf_any = DP.brute_force(z, alts, [0, 9], open_w, D)
                if path is None:
                    assert bf_any is None and DP.forward_backward(z, alts, [0, 9], D, windows=wins) is None, (T, N, D, wins)
                    none += 1
                    continue
                tok = np.array([s // 3 if s % 3 else -1 for s in path])
                bf = DP.brute_force(z, alts, [0, 9], open_w, D, tok=tok)
                fb = DP.forward_backward(z, alts, [0, 9], D, tok=tok, windows=wins, want_gamma=True)
                assert abs(fb["logz"] - bf["logz"]) < 1e-10, (T, N, D, wins)
                for key in ("gG", "gB", "gI", "gH", "tok_post", "start_mean", "start_sd"):
                    assert np.allclose(fb[key], bf[key], rtol=0, atol=1e-10), (key, T, N, D, wins)
                if N:
                    assert np.allclose(fb["sum_gamma_b"], 1.0, atol=1e-10)
                    assert np.allclose((fb["gG"].sum(1) + fb["gB"].sum(1) + fb["gI"].sum(1) + fb["gH"].sum((1, 2))), 1.0, atol=1e-10)
                checked += 1
                chained += bool(N) and max(D) == 3 and fb["gH"].max() > 0.01
    print(checked, none, chained)
    assert checked > 150 and none > 50 and chained > 40


def test_all_ones_is_posterior_ref():
    rng = np.random.default_rng(5)
    for T, N in ((1, 1), (9, 3), (40, 11), (64, 0)):
        alts = [[(1 + 2 * k, 2 + 2 * k)] for k in range(N)]
        z = rng.standard_normal((T, 2 * N + 3)) * 3.0
        path, _ = M.viterbi(z, alts, [0], [1] * N)
        tok = np.array([s // 3 if s % 3 else -1 for s in path])
        a = DP.forward_backward(z, alts, [0], [1] * N, tok=tok, want_gamma=True)
        b = P.forward_backward(z, alts, [0], tok=tok, want_gamma=True)
        for key in ("logz", "gG", "gB", "gI", "tok_post", "start_mean", "start_sd"):
            assert np.allclose(a[key], b[key], rtol=0, atol=1e-12), key
        assert not a["gH"].any()
        a32 = DP.forward_backward(z, alts, [0], [1] * N, tok=tok, dtype=np.float32)
        b32 = P.forward_backward(z, alts, [0], tok=tok, dtype=np.float32)
        assert a32["logz"] == b32["logz"] and np.array_equal(a32["tok_post"], b32["tok_post"])      # the restatement mode, too


def test_chain_gamma_is_shifted_start_gamma():
    """gamma_t(H_k^j) = gamma_{t-j+1}(B_k): every path in B_k at t is in H_k^j exactly j - 1 frames later."""
    rng = np.random.default_rng(17)
    T, N = 60, 6
    alts = [[(1 + 2 * k, 2 + 2 * k)] for k in range(N)]
    D = [8, 1, 5, 3, 2, 6]
    z = rng.standard_normal((T, 2 * N + 2)) * 2.0
    fb = DP.forward_backward(z, alts, [0, 2 * N + 1], D, want_gamma=True)
    for k in range(N):
        for j in range(2, D[k]):
            assert np.allclose(fb["gH"][j - 1:, k, j - 2], fb["gB"][:T - j + 1, k], rtol=0, atol=1e-12), (k, j)
            assert not fb["gH"][:j - 1, k, j - 2].any()
        assert not fb["gH"][:, k, max(D[k] - 2, 0):].any()
    assert fb["gH"].max() > 0.05
    f32 = DP.forward_backward(z, alts, [0, 2 * N + 1], D, dtype=np.float32)
    assert abs(f32["logz"] - fb["logz"]) < 1e-3 * abs(fb["logz"])


# ------------------------------------------------------------------------------------------------ 2. the options
def test_option_rules_17_and_18_and_their_order():
    from wfl_asr_amd.options import MIN_DURATION_SCORES_ERROR, resolve
    assert resolve({}).duration_scores is False and resolve({"align": "viterbi", "min_duration": 0.06}).duration_scores is False
    a = resolve({"align": "viterbi", "min_duration": 0.06, "duration_scores": True})
    assert a.duration_scores is True and a.scored and not a.align_scores and not a.free_scores
    assert resolve({"align": "viterbi", "min_duration": 0.06, "duration_scores": True}, duration_scores=False).duration_scores is False
    assert resolve({"align": "viterbi", "min_duration": 0.06, "align_draft": "d"}, duration_scores=True).align_draft == "d"
    with pytest.raises(ValueError, match="duration_scores needs align='viterbi'"):                                   # rule 17
        resolve({}, duration_scores=True)
    with pytest.raises(ValueError, match="duration_scores needs a min_duration.*align_scores is the option"):        # rule 18
        resolve({"align": "viterbi"}, duration_scores=True)
    with pytest.raises(ValueError, match="duration_scores needs a min_duration"):
        resolve({"align": "viterbi", "min_duration": {}}, duration_scores=True)
    # the earlier rule is reported: 15 before 17, 16 before 17 / 18; rule 16 and its message stay
    with pytest.raises(ValueError, match="min_duration needs align='viterbi'"):
        resolve({}, min_duration=0.06, duration_scores=True)
    with pytest.raises(ValueError) as e:
        resolve({"align": "viterbi", "min_duration": 0.06, "align_scores": True, "duration_scores": True})
    assert str(e.value) == MIN_DURATION_SCORES_ERROR and "duration_scores" not in MIN_DURATION_SCORES_ERROR


def test_post_options_carry_the_field():
    from wfl_asr_amd.options import PostOptions, resolve
    plain = resolve({"align": "viterbi", "min_duration": 0.06})
    a = resolve({"align": "viterbi", "min_duration": 0.06, "duration_scores": True})
    assert isinstance(a, PostOptions) and len(a) == 8 and a[:8] == plain[:8] and len(PostOptions._fields) == 8
    assert a != plain and plain != a and hash(a) != hash(plain) and a != tuple(a) and len({a, plain, a}) == 2
    assert a == resolve({"align": "viterbi", "duration_scores": True}, min_duration=0.06)
    assert "duration_scores=True" in repr(a) and "duration_scores=False" in repr(plain)
    assert a._replace(align_draft="d").duration_scores is True and a._replace(duration_scores=False) == plain
    assert a._asdict()["duration_scores"] is True and PostOptions._make(tuple(a), duration_scores=True).duration_scores is True
    assert PostOptions._make(tuple(a)).duration_scores is False and resolve({}) == tuple(resolve({}))
    with pytest.raises(AttributeError):
        a.duration_scores = False


def test_signatures_and_the_refusal_before_any_model_is_loaded(AL, monkeypatch):
    from wfl_asr_amd import infer as I
    assert list(inspect.signature(AL.duration_posteriors).parameters) == [
        "logits", "n_frames", "token_classes", "gap_classes", "o_id", "tok", "frame_offsets", "stream", "packed", "windows", "min_frames"]
    for name in ("frame_offsets", "stream", "packed", "windows", "min_frames"):
        assert inspect.signature(AL.duration_posteriors).parameters[name].default is None
    assert list(inspect.signature(AL.duration_posterior_workspace_bytes).parameters) == ["n_frames", "n_tokens"]
    assert "min_frames" not in inspect.signature(AL.alignment_posteriors).parameters

    def no_load(*a, **k):
        raise AssertionError("a model was loaded before the options were refused")
    for f in (I.infer_audio, I.infer_folder, I.Labeler.label_files):
        names = list(inspect.signature(f).parameters)
        assert inspect.signature(f).parameters["duration_scores"].default is None
        assert names.index("duration_scores") == names.index("min_duration") + 1 and names[-1] == "bigram_scores"
    monkeypatch.setattr(I, "_labeler", no_load)
    monkeypatch.setattr(I, "Labeler", no_load)
    with pytest.raises(ValueError, match="duration_scores needs a min_duration"):
        I.infer_audio("x.wav", align="viterbi", duration_scores=True)
    with pytest.raises(ValueError, match="duration_scores needs align='viterbi'"):
        I.infer_folder("some_folder", duration_scores=True)


def test_the_cli_flag_reaches_the_record(monkeypatch, tmp_path):
    import __graft_entry__  # noqa: F401
    from wfl_asr_amd import infer as I
    seen = {}

    def record(*a, **k):
        seen.update(k)
        raise SystemExit(0)
    monkeypatch.setattr(I.torch.cuda, "is_available", lambda: True)     # (the CLI turns away a machine without a device first)
    monkeypatch.setattr(I, "infer_audio", record)
    monkeypatch.setattr(I, "infer_folder", record)
    wav, ckpt, cfg = tmp_path / "x.wav", tmp_path / "m.pt", tmp_path / "config.yaml"
    wav.write_bytes(b"")
    ckpt.write_bytes(b"")
    cfg.write_text("postprocess:\n  align: viterbi\n")
    base = [str(wav), "-ckpt", str(ckpt), "-c", str(cfg)]
    with pytest.raises(SystemExit) as e:
        I.main(base + ["--min-duration", "0.06", "--duration-scores"])
    assert e.value.code == 0 and seen.get("duration_scores") is True and seen.get("min_duration") == 0.06 and seen["align_scores"] is False
    with pytest.raises(SystemExit) as e:
        I.main(base + ["--min-duration", "0.06"])
    assert e.value.code == 0 and seen.get("duration_scores") is False
    cfg.write_text("postprocess:\n  align: viterbi\n  min_duration: 0.04\n  duration_scores: true\n")    # from the config file
    with pytest.raises(SystemExit) as e:
        I.main(base)
    assert e.value.code == 0 and seen.get("duration_scores") is True and seen.get("min_duration") == 0.04
    for extra in (["--duration-scores"], ["--align", "greedy", "--duration-scores"]):                         # rules 18 and 17: usage errors
        cfg.write_text("postprocess:\n  align: viterbi\n")
        with pytest.raises(SystemExit) as e:
            I.main(base + extra)
        assert e.value.code == 2


# ------------------------------------------------------------------------------------------------ 3. the ABI and the packing
def test_the_abi_entry_checks_its_arguments(AL):
    import os
    from wfl_asr_amd import _lib
    lib = _lib.load()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wfl_asr.h")).read()
    for name in ("wfl_align_min_duration_posterior", "wfl_align_min_duration_posterior_workspace_bytes"):
        assert name + "(" in src and hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["wfl_align_min_duration_posterior"][1]) == len(_lib.SIGNATURES["wfl_align_posterior_windowed"][1]) + 1
    Pv = ctypes.c_void_p
    buf = (ctypes.c_char * 64)()
    d = ctypes.cast(buf, Pv)                       # never dereferenced: every call below fails on the host
    fo, ko = np.zeros(1, np.int64), np.zeros(1, np.int32)
    T, N = np.array([300], np.int32), np.array([3], np.int32)
    h = lambda a: a.ctypes.data_as(Pv)             # noqa: E731
    need = lib.wfl_align_min_duration_posterior_workspace_bytes(h(T), h(N), 1)
    plain = lib.wfl_align_posterior_workspace_bytes(h(T), h(N), 1)
    # three checkpoints of 128 slots, 6 chain floats more per slot than wfl_align_posterior's
    assert need == plain + 3 * 128 * 6 * 4 and AL.duration_posterior_workspace_bytes(T, N) == need
    assert lib.wfl_align_min_duration_posterior_workspace_bytes(None, None, 1) == -1
    assert lib.wfl_align_min_duration_posterior_workspace_bytes(h(np.array([-1], np.int32)), h(N), 1) == -1
    assert lib.wfl_align_min_duration_posterior_workspace_bytes(None, None, 0) == 0

    def post(win, dmin, ws_bytes=need, C=141, tok=d):
        return lib.wfl_align_min_duration_posterior(d, 141, C, 0, h(fo), h(T), h(ko), h(N), d, win, dmin, d, 1, tok, d, ws_bytes,
                                                    d, d, d, d, d, None)
    for win in (None, d):                          # tok_win is nullable, tok_min is not
        assert post(win, None) == -1 and b"wfl_align_min_duration_posterior: null device" in lib.wfl_last_error()
        assert post(win, d, tok=None) == -1 and b"wfl_align_min_duration_posterior: null device" in lib.wfl_last_error()
        assert post(win, d, C=0) != 0 and b"wfl_align_min_duration_posterior: C must" in lib.wfl_last_error()
        assert post(win, d, ws_bytes=need - 1) != 0 and b"wfl_align_min_duration_posterior_workspace_bytes" in lib.wfl_last_error()
    assert post(d, d, ws_bytes=plain) != 0         # wfl_align_posterior's size is not enough
    assert lib.wfl_align_min_duration_posterior(d, 141, 141, 0, None, None, None, None, None, None, None, d, 0, None, None, 0,
                                                d, d, d, d, d, None) == 0


def test_duration_posteriors_refuses_a_batch_packed_without_durations(AL):
    packed = AL.PackedClips(0, None, None, None, None, None, None, d_win=object())
    with pytest.raises(ValueError, match="duration_posteriors scores the lattice with minimum durations: this batch was packed without"):
        AL._with_min_frames(packed, "duration_posteriors")
    with pytest.raises(ValueError, match="packed without min_frames"):     # (refused before the logits are looked at)
        AL.duration_posteriors(None, [], [], [], 0, None, packed=packed)
    with_min = AL.PackedClips(0, 1, 2, 3, 4, 5, 6, None, d_min=object())
    assert AL._with_min_frames(with_min, "x") is with_min and len(with_min) == 9
