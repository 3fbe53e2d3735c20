"""CPU (-m "not gpu"): the host side of the duration-prior decode's posteriors -- the float64 semi-Markov forward-backward of
tests/bio_duration_posterior_ref.py against the enumeration of every class string and, without a prior, against the bigram reference;
the rules of `postprocess.decode_duration_scores` (options.py); the ABI entries, the workspace formula and the host-side argument
checks (no GPU is touched: every bad call returns before a launch); the score file of a FreeScore built from the reference's arrays."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import bio_bigram_posterior_ref as BP
import bio_duration_posterior_ref as DP
import bio_duration_ref as R
from test_decode_duration_cpu import C, TABLE, _tiny_case
from wfl_asr_amd import decode as DC
from wfl_asr_amd import native_post as npost
from wfl_asr_amd import options as OPT
from wfl_asr_amd.options import PostOptions, resolve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_reference_equals_the_enumeration_of_every_class_string():
    """T = 1 .. 5, D = 1, 2, 3, -inf entries of both tables, rows of -1 and forced frames; the path is the reference search's own."""
    seen, seen_forced, seen_inf, seen_none, seen_tail = set(), 0, 0, 0, 0
    worst = 0.0
    for seed in range(300):
        z, W, dur, sd, forced = _tiny_case(seed)
        if len(z) > 5:
            continue
        ids, obj = R.viterbi(z, TABLE, W, dur, sd, forced)
        assert np.isfinite(obj)
        got = DP.forward_backward(z, TABLE, W, dur, sd, forced, ids)
        want = DP.brute_force(z, TABLE, W, dur, sd, forced, ids)
        d = max(abs(got[0] - want[0]), float(np.abs(got[1] - want[1]).max()), float(np.abs(got[2] - want[2]).max()))
        worst = max(worst, d)
        assert d <= 1e-12, (seed, d)
        assert got[0] >= obj - 1e-12                     # logZ sums over the search's path too
        assert (got[2] <= got[1] + 1e-12).all() and (got[1] <= 1 + 1e-12).all() and (got[2] >= 0).all()
        g32 = DP.forward_backward(z, TABLE, W, dur, sd, forced, ids, dtype=np.float32)
        assert abs(g32[0] - got[0]) <= 1e-4 and np.abs(g32[1] - got[1]).max() <= 1e-4 and np.abs(g32[2] - got[2]).max() <= 1e-4
        D = dur.shape[1] - 1
        seen.add((len(z), D))
        seen_forced += bool(forced.any())
        seen_inf += bool(np.isneginf(dur).any() and np.isneginf(W).any())
        seen_none += bool((np.asarray(sd) < 0).any())
        seen_tail += any(k > D for _, _, k in R.run_lengths(ids, TABLE))
    print(f"float64 reference against the enumeration: largest deviation {worst:.3e}")
    assert seen == {(T, D) for T in range(1, 6) for D in (1, 2, 3)}
    assert seen_forced >= 50 and seen_inf >= 50 and seen_none >= 50 and seen_tail >= 10


def test_the_enumeration_weighs_a_string_as_the_objective_does():
    """bio_duration_posterior_ref.path_weights is vectorised over the strings; on every string of short clips it is
    bio_duration_ref.objective's weight (a string that is no path: -inf)."""
    n = 0
    for seed in range(40):
        z, W, dur, sd, forced = _tiny_case(seed)
        z, forced = z[:3], forced[:3]
        paths, tot = DP.path_weights(z, TABLE, W, dur, sd, forced)
        for ids, w in zip(paths, tot):
            want = R.objective(ids, z, TABLE, W, dur, sd, forced) if R.legal(ids, TABLE) else -np.inf
            assert (w == want) or abs(w - want) <= 1e-12, (seed, ids, w, want)
            n += np.isfinite(want)
    assert n > 500


@pytest.mark.parametrize("prior", ["none", "zero"])
def test_without_a_prior_it_is_the_bigram_posterior(prior):
    for seed in range(20):
        rng = np.random.default_rng(900 + seed)
        T, D = int(rng.integers(1, 60)), int(rng.integers(1, 9))
        z = rng.standard_normal((T, C)) * 2
        W = -3.0 * rng.random((4, 4))
        if seed % 2:
            W[1, 2] = W[0, 3] = -np.inf
        forced = rng.random(T) < 0.1
        dur = np.zeros((2, D + 1))
        sd = [-1, -1, -1] if prior == "none" else [0, 1, 0]
        ids, _ = R.viterbi(z, TABLE, W, dur, sd, forced)
        got = DP.forward_backward(z, TABLE, W, dur, sd, forced, ids)
        want = BP.forward_backward(z, TABLE, W, forced, ids)
        assert abs(got[0] - want[0]) <= 1e-10
        assert np.abs(got[1] - want[1]).max() <= 1e-10 and np.abs(got[2] - want[2]).max() <= 1e-10


def test_the_option_rules():
    on = {"decode": "viterbi", "decode_duration_prior": "d.json", "decode_duration_scores": True}
    a = resolve(on)
    assert isinstance(a, PostOptions) and a.decode_duration_scores is True and a.free_scores and a.scored
    assert not a.decode_scores and not a.bigram_scores and len(a) == 8
    assert "decode_duration_scores" in PostOptions._KEYWORD and len(PostOptions._KEYWORD) == len(PostOptions._KEYWORD_DEFAULTS)
    assert "decode_duration_scores=True" in repr(a) and a._asdict()["decode_duration_scores"] is True
    assert a != resolve({"decode": "viterbi", "decode_duration_prior": "d.json"}) and hash(a) != hash(a._replace(decode_duration_scores=False))
    assert a._replace(decode_duration_scores=False) == resolve({"decode": "viterbi", "decode_duration_prior": "d.json"})
    plain = resolve({})
    assert plain.decode_duration_scores is False and not plain.free_scores and not plain.scored
    # the argument wins over the config; beside a bigram and a switch penalty it stands
    assert resolve(on, decode_duration_scores=False).decode_duration_scores is False
    b = resolve({"decode": "viterbi", "phoneme_bigram": "b.json", "switch_penalty": 1.5, "decode_duration_prior": "d.json"},
                decode_duration_scores=True)
    assert b.decode_duration_scores and b.phoneme_bigram == "b.json" and b.free_scores
    for post, message in (
            ({"decode_duration_scores": True}, "decode_duration_scores needs decode='viterbi'"),
            ({"decode": "argmax", "decode_duration_scores": True}, "decode_duration_scores needs decode='viterbi'"),
            ({"decode": "viterbi", "decode_duration_scores": True}, OPT.DECODE_DURATION_SCORES_ERROR),
            ({"decode": "viterbi", "phoneme_bigram": "b.json", "decode_duration_scores": True}, OPT.DECODE_DURATION_SCORES_ERROR),
            ({"decode": "viterbi", "decode_duration_prior": "d.json", "decode_duration_scores": 1}, "must be true or false"),
            ({"decode": "viterbi", "decode_duration_prior": "d.json", "decode_duration_scores": "yes"}, "must be true or false"),
            ({"decode": "viterbi", "decode_duration_prior": "d.json", "decode_scores": True}, OPT.DECODE_DURATION_PRIOR_ERROR),
            ({"decode": "viterbi", "decode_duration_prior": "d.json", "decode_scores": True, "decode_duration_scores": True},
             OPT.DECODE_DURATION_PRIOR_ERROR),
            ({"decode": "viterbi", "decode_duration_prior": "d.json", "phoneme_bigram": "b.json", "bigram_scores": True},
             OPT.DECODE_DURATION_PRIOR_ERROR)):
        with pytest.raises(ValueError) as err:
            resolve(post)
        assert message in str(err.value), (post, str(err.value))
    # without a prior the message names the option to ask for; beside a prior the refusal of the other two names this one
    assert "decode_scores" in OPT.DECODE_DURATION_SCORES_ERROR and "bigram_scores" in OPT.DECODE_DURATION_SCORES_ERROR
    assert "decode_duration_scores" in OPT.DECODE_DURATION_PRIOR_ERROR and "--decode-duration-scores" in OPT.DECODE_DURATION_PRIOR_ERROR
    assert OPT.DECODE_DURATION_PRIOR_ERROR.startswith("decode_duration_prior cannot be combined with decode_scores or bigram_scores: their "
                                                      "forward-backward sweeps carry no duration term, and a posterior must score the "
                                                      "grammar the search ran on")
    assert "for the scoring run" not in OPT.DECODE_DURATION_PRIOR_ERROR


def test_the_keyword_is_threaded_and_refused_before_any_model_is_loaded(tmp_path):
    from wfl_asr_amd import infer
    from wfl_asr_amd.infer import Labeler, infer_audio, infer_folder
    for f in (Labeler.label_files, infer_audio, infer_folder):
        assert inspect.signature(f).parameters["decode_duration_scores"].default is None, f
    assert "decode_duration_scores" in inspect.signature(resolve).parameters

    class Stub:
        config = {"postprocess": {"decode": "viterbi", "decode_duration_prior": "d.json", "decode_duration_scores": True}}
    assert Labeler.options(Stub()) == PostOptions(decode="viterbi", decode_duration_prior="d.json", decode_duration_scores=True)

    def no_model(*a, **k):
        raise AssertionError("a model was asked for")
    saved = infer._labeler
    infer._labeler = no_model
    try:
        with pytest.raises(ValueError, match="decode_duration_scores needs decode='viterbi'"):
            infer_audio("x.wav", decode_duration_scores=True)
        with pytest.raises(ValueError, match="decode_duration_scores needs a decode_duration_prior"):
            infer_folder(str(tmp_path), decode="viterbi", decode_duration_scores=True, config_path=str(tmp_path / "none.yaml"))
        cfg = tmp_path / "config.yaml"
        cfg.write_text("postprocess:\n  decode: viterbi\n  decode_duration_prior: d.json\n")
        with pytest.raises(AssertionError, match="a model was asked for"):
            infer_audio("x.wav", config_path=str(cfg), decode_duration_scores=True)
    finally:
        infer._labeler = saved


def test_parameter_lists_of_the_python_entries():
    assert list(inspect.signature(DC.decode_posteriors_duration).parameters) == [
        "logits", "n_frames", "table", "trans", "dur", "sym_dur", "threshold", "ids", "frame_offsets", "stream"]
    assert list(inspect.signature(DC.duration_posterior_workspace_bytes).parameters) == ["n_frames", "n_pairs", "D"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import _lib
    return _lib.load()


def test_abi_entries_and_the_workspace_formula(lib):
    from wfl_asr_amd import _lib
    src = open(os.path.join(ROOT, "include", "wfl_asr.h")).read()
    for name in ("wfl_decode_duration_posterior_workspace_bytes", "wfl_decode_duration_posterior"):
        assert re.search(rf"\b{name}\s*\(", src) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["wfl_decode_duration_posterior"][1]) == 23
    assert len(_lib.SIGNATURES["wfl_decode_duration_posterior_workspace_bytes"][1]) == 4
    assert lib.wfl_decode_duration_posterior is not None
    h = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    size = lib.wfl_decode_duration_posterior_workspace_bytes
    r64 = lambda x: (x + 63) // 64 * 64                   # noqa: E731
    T = np.array([300, 0, 17], np.int32)

    def want(P, D):                                       # the header's formula
        N = P + 1
        HS = r64(N)
        table = (4 * N * (N | 1) + 15) // 16 * 16
        H = 0 if table + 6912 + 4 * (2 * D + 1) * HS <= 163840 - 4608 else r64((2 * D + 1) * HS)
        return 4 * sum(r64(int(t) * (D + 2)) + r64(int(t)) + H + 2 * r64(int(t)) for t in T if t > 0)
    for P, D in ((1, 1), (70, 32), (140, 32), (158, 32), (159, 32), (170, 8), (191, 1), (191, 2), (191, 3), (191, 32)):
        assert size(h(T), 3, P, D) == want(P, D) == DC.duration_posterior_workspace_bytes(T, P, D), (P, D)
    # the history is in LDS at 159 symbols for every D, at the cap for D <= 2 alone
    per_frame = lambda D: 4 * sum(r64(int(t) * (D + 2)) + 3 * r64(int(t)) for t in T if t > 0)   # noqa: E731
    assert size(h(T), 3, 158, 32) == per_frame(32) < size(h(T), 3, 159, 32)
    assert size(h(T), 3, 191, 2) == per_frame(2) and size(h(T), 3, 191, 3) > per_frame(3)
    assert size(h(T), 3, 192, 8) == 0                    # over the symbol cap: nothing is scored
    for bad_D in (0, 33, -1):
        assert size(h(T), 3, 70, bad_D) == -1
    assert size(None, 3, 70, 8) == -1 and size(h(T), -1, 70, 8) == -1 and size(h(np.array([-1], np.int32)), 1, 70, 8) == -1
    with pytest.raises(Exception, match="wfl_decode_duration_posterior_workspace_bytes"):
        DC.duration_posterior_workspace_bytes(T, 70, 33)


def test_host_side_argument_checks(lib):
    """Every bad call returns a negative code and names the entry before anything is launched (the pointers are never read)."""
    P, Cn, D = 70, 141, 8
    T = np.array([100], np.int32)
    fo = np.array([0], np.int64)
    h = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    buf = (ctypes.c_char * 64)()
    dev = ctypes.cast(buf, ctypes.c_void_p)              # stands for a device pointer
    need = lib.wfl_decode_duration_posterior_workspace_bytes(h(T), 1, P, D)
    assert need > 0

    def call(**kw):
        a = dict(logits=dev, ldl=Cn, C=Cn, o_id=0, fo=fo, T=T, n=1, pairs=dev, n_pairs=P, trans=dev, sym_dur=dev, dur=dev, n_rows=4, D=D,
                 thr=0.5, ids=dev, ws=dev, ws_n=need, logz=dev, post=dev, cls=dev, status=dev)
        a.update(kw)
        return lib.wfl_decode_duration_posterior(a["logits"], a["ldl"], a["C"], a["o_id"], h(a["fo"]) if a["fo"] is not None else None,
                                                 h(a["T"]) if a["T"] is not None else None, a["n"], a["pairs"], a["n_pairs"], a["trans"],
                                                 a["sym_dur"], a["dur"], a["n_rows"], a["D"], a["thr"], a["ids"], a["ws"], a["ws_n"],
                                                 a["logz"], a["post"], a["cls"], a["status"], None)
    for kw, word in ((dict(D=0), b"D must be 1 .. 32"), (dict(D=33), b"D must be 1 .. 32"), (dict(n_rows=-1), b"n_rows < 0"),
                     (dict(dur=None), b"null dur"), (dict(sym_dur=None), b"null sym_dur"), (dict(trans=None), b"null device pointer"),
                     (dict(ws_n=need - 1), b"workspace too small"), (dict(ws=None), b"workspace too small"),
                     (dict(C=0), b"C < 1"), (dict(o_id=Cn), b"o_id"), (dict(ldl=Cn - 1), b"ldl"), (dict(n=-1), b"negative count"),
                     (dict(n_pairs=-1), b"negative count"), (dict(thr=-0.5), b"threshold"), (dict(fo=None), b"null host array"),
                     (dict(T=np.array([-1], np.int32)), b"negative offset or frame count"), (dict(logits=None), b"null device pointer"),
                     (dict(ids=None), b"null device pointer"), (dict(logz=None), b"null device pointer"),
                     (dict(post=None), b"null device pointer"), (dict(cls=None), b"null device pointer"),
                     (dict(status=None), b"null device pointer"), (dict(pairs=None), b"null device pointer")):
        rc = call(**kw)
        err = lib.wfl_last_error()
        assert rc < 0, kw
        assert b"wfl_decode_duration_posterior" in err and word in err, (kw, err)
    # an empty batch is fine and launches nothing; so is a null dur without rows and a null sym_dur without phonemes or frames
    assert call(n=0) == 0
    assert call(n=0, dur=None, n_rows=0, sym_dur=None, trans=None) == 0


def test_the_score_file_of_a_freescore_built_from_the_reference(lib):
    """decode.free_score and the two writers downstream are unchanged: a FreeScore from the float64 reference's arrays formats as
    decode_scores' does (one `#` header with the file's four figures, one row per run of the path)."""
    from wfl_asr_amd.infer import format_decode_review_tsv, format_decode_scores_tsv
    labels = ["O", "B-a", "I-a", "B-k", "I-k", "B-t"]
    table = DC.class_table(labels)
    rng = np.random.default_rng(12)
    T = 40
    z = rng.standard_normal((T, len(labels))) * 2.5
    W = -2.0 * rng.random((4, 4))
    dur = -2.0 * rng.random((3, 5))
    dur[:, 0] = -np.inf                               # no run of one frame for a and k; t has no I class and no prior
    sd = np.array([0, 1, -1], np.int32)
    ids, obj = R.viterbi(z, table, W, dur, sd)
    runs = R.run_lengths(ids, table)
    assert runs and all(k >= 2 for s, _, k in runs if s != 3)
    logz, post, cls = DP.forward_backward(z, table, W, dur, sd, None, ids)
    lse = float(R.prepass(z, 0.0)[0].sum())
    lt = npost.LabelTable(labels)
    fs = DC.free_score(obj - lse, logz, lse, post, cls, ids, [T], [None], [0.0], lt, 0.02)
    assert isinstance(fs, DC.FreeScore) and len(fs.runs) == len(runs)
    assert fs.path_log_posterior <= 1e-9 and abs(fs.path_log_posterior - (obj - logz)) <= 1e-9
    for r, (s, t0, k) in zip(fs.runs, runs):
        assert abs(r.posterior - post[t0:t0 + k].mean()) <= 1e-12 and r.start_posterior == cls[t0]
        assert r.min_frame_posterior == post[t0:t0 + k].min() and 0 <= r.start_posterior <= post[t0] + 1e-12 <= 1 + 2e-12
    text = format_decode_scores_tsv(fs, len(runs))
    lines = text.strip().split("\n")
    assert lines[0].startswith("# path_log_posterior=") and f"runs={len(runs)} lab_lines={len(runs)}" in lines[0]
    assert len(lines) == 1 + len(runs) and all(len(ln.split("\t")) == 6 for ln in lines[1:])
    assert [ln.split("\t")[2] for ln in lines[1:]] == [r.phoneme for r in fs.runs]
    review = format_decode_review_tsv([("x.wav", fs)]).strip().split("\n")
    assert len(review) == 2 and review[1].split("\t")[0] == "x.wav" and review[1].split("\t")[-1] == str(len(runs))
