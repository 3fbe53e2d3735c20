"""CPU (-m "not gpu"): the host side of the bigram decode's posteriors -- the float64 forward-backward of tests/bio_bigram_posterior_ref.py
against its brute force and against the flat-penalty reference, the ABI entries, the Python entry's parameter list and the validation
of `bigram_scores`."""
import inspect
import os
import re

import numpy as np
import pytest

import bio_bigram_posterior_ref as BP
import bio_bigram_ref as R
import bio_posterior_ref as P
from wfl_asr_amd import decode as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE5 = (1, [(2, 3), (4, -1)])          # C = 5: class 0 is never chosen, O = 1, a (B, I) pair, a B alone
TABLE6 = (0, [(1, 2), (3, 4)])           # C = 6: class 5 is never chosen, two (B, I) pairs


def _random_table(n, rng, forbid):
    W = -6.0 * rng.random((n + 1, n + 1))
    mask = rng.random(W.shape) < forbid
    mask[:, 0] = False
    W[mask] = -np.inf
    return W


@pytest.mark.parametrize("T,C,table", [(1, 5, TABLE5), (2, 5, TABLE5), (3, 5, TABLE5), (4, 5, TABLE5), (5, 5, TABLE5), (3, 6, TABLE6),
                                       (4, 6, TABLE6)])
def test_reference_equals_brute_force(T, C, table):
    rng = np.random.default_rng(20 + 7 * T + C)
    seen_forced = seen_forbidden = 0
    for trial in range(12 if T < 5 else 4):
        z = rng.standard_normal((T, C)) * 2
        W = _random_table(2, rng, 0.3 if trial % 2 else 0.0)
        forced = rng.random(T) < 0.25 if trial % 3 == 0 else None
        ids, _ = R.viterbi(z, table, W, forced)
        got = BP.forward_backward(z, table, W, forced, ids)
        want = BP.brute_force(z, table, W, forced, ids)
        assert abs(got[0] - want[0]) <= 1e-10, (trial, got[0], want[0])
        assert np.abs(got[1] - want[1]).max() <= 1e-10 and np.abs(got[2] - want[2]).max() <= 1e-10, trial
        assert (got[2] <= got[1] + 1e-12).all() and (got[1] <= 1 + 1e-12).all()
        # the float32 restatement is the same recurrence: close to float64 on inputs this small
        g32 = BP.forward_backward(z, table, W, forced, ids, dtype=np.float32)
        assert abs(g32[0] - got[0]) <= 1e-4 and np.abs(g32[1] - got[1]).max() <= 1e-4
        if forced is not None:
            seen_forced += int(forced.sum())
        seen_forbidden += int(np.isneginf(W).sum())
    assert seen_forbidden and (T < 2 or seen_forced)


@pytest.mark.parametrize("lam", [0.0, 1.5, 4.0])
def test_a_flat_table_is_the_flat_posterior(lam):
    rng = np.random.default_rng(4)
    table = (0, [(1, 2), (3, 4), (5, -1)])
    for T in (1, 7, 60):
        z = rng.standard_normal((T, 8)) * 3
        forced = rng.random(T) < 0.2
        W = np.full((4, 4), -lam)
        ids, _ = R.viterbi(z, table, W, forced)
        got = BP.forward_backward(z, table, W, forced, ids, want_gamma=True)
        want = P.forward_backward(z, table, lam, forced, ids, want_gamma=True)
        assert abs(got[0] - want[0]) <= 1e-12 * max(1.0, abs(want[0]))
        for a, b in zip(got[1:], want[1:]):
            assert np.abs(a - b).max() <= 1e-12


def test_abi_entries():
    from wfl_asr_amd import _lib
    src = open(os.path.join(ROOT, "include", "wfl_asr.h")).read()
    for name in ("wfl_decode_bigram_posterior_workspace_bytes", "wfl_decode_bigram_posterior"):
        assert re.search(rf"\b{name}\s*\(", src) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["wfl_decode_bigram_posterior"][1]) == 19
    assert len(_lib.SIGNATURES["wfl_decode_bigram_posterior_workspace_bytes"][1]) == 3
    assert int(re.search(r"#define\s+WFL_ABI_VERSION\s+(\d+)", src).group(1)) == 2
    import __graft_entry__ as g
    g.build()
    lib = _lib.load()                                                  # (binds every signature: both symbols are exported)
    assert lib.wfl_decode_bigram_posterior is not None
    T = np.array([10, 0, 7], np.int32)
    # per clip with T > 0: round_up_64(3 T) + 3 round_up_64(T) words, whatever n_pairs under the cap
    for n_pairs in (0, 70, 191):
        assert DC.bigram_posterior_workspace_bytes(T, n_pairs) == 4 * 2 * (64 + 3 * 64)
        assert DC.bigram_posterior_workspace_bytes(T, n_pairs) == DC.posterior_workspace_bytes(T, n_pairs)
    assert DC.bigram_posterior_workspace_bytes(np.array([1500], np.int32), 70) == 4 * (4544 + 3 * 1536)
    assert DC.bigram_posterior_workspace_bytes(T, 192) == 0             # over the cap: nothing is scored


def test_the_entry_validates_its_arguments_without_gpu():
    import ctypes
    import __graft_entry__ as g
    g.build()
    from wfl_asr_amd import _lib
    lib = _lib.load()
    V = ctypes.c_void_p
    buf = (ctypes.c_char * 64)()
    d = ctypes.cast(buf, V)                        # never dereferenced: every call below fails on the host
    fo = np.zeros(1, np.int64)
    T = np.array([10], np.int32)
    h = lambda a: a.ctypes.data_as(V)              # noqa: E731

    def call(C=141, o_id=0, ldl=141, fo_=fo, T_=T, ws=None, ws_bytes=0, logits=d, n=1, ids=d, pairs=d, n_pairs=70, trans=d, thr=0.0,
             logz=d, post=d, cls=d, status=d):
        return lib.wfl_decode_bigram_posterior(logits, ldl, C, o_id, h(fo_) if fo_ is not None else None, h(T_), n, pairs, n_pairs, trans,
                                               thr, ids, ws, ws_bytes, logz, post, cls, status, None)

    need = lib.wfl_decode_bigram_posterior_workspace_bytes(h(T), 1, 70)
    assert need == 4 * (64 + 3 * 64)
    for kw, word in ((dict(C=0), b"C < 1"), (dict(o_id=141), b"o_id"), (dict(ldl=100), b"ldl"), (dict(n=-1), b"negative count"),
                     (dict(n_pairs=-1), b"negative count"), (dict(thr=-0.1), b"threshold"),
                     (dict(fo_=None, ws=d, ws_bytes=need), b"null host"),
                     (dict(T_=np.array([-2], np.int32), ws=d, ws_bytes=need), b"negative"),
                     (dict(logits=None, ws=d, ws_bytes=need), b"null device"), (dict(ids=None, ws=d, ws_bytes=need), b"null device"),
                     (dict(logz=None, ws=d, ws_bytes=need), b"null device"), (dict(post=None, ws=d, ws_bytes=need), b"null device"),
                     (dict(cls=None, ws=d, ws_bytes=need), b"null device"), (dict(status=None, ws=d, ws_bytes=need), b"null device"),
                     (dict(pairs=None, ws=d, ws_bytes=need), b"null device"), (dict(trans=None, ws=d, ws_bytes=need), b"null device"),
                     (dict(ws=d, ws_bytes=need - 1), b"workspace"), (dict(ws=None, ws_bytes=need), b"workspace")):
        assert call(**kw) != 0, kw
        err = lib.wfl_last_error()
        assert b"wfl_decode_bigram_posterior" in err and word in err, (kw, err)
    assert call(n=0) == 0                          # nothing to do
    assert call(n=0, trans=None) == 0
    size = lib.wfl_decode_bigram_posterior_workspace_bytes
    assert size(h(T), -1, 70) < 0 and size(h(T), 1, -1) < 0 and size(None, 1, 70) < 0 and size(None, 0, 70) == 0


def test_parameter_list_of_the_python_entry():
    assert list(inspect.signature(DC.decode_posteriors_bigram).parameters) == ["logits", "n_frames", "table", "trans", "threshold", "ids",
                                                                               "frame_offsets", "stream"]
    assert list(inspect.signature(DC.bigram_posterior_workspace_bytes).parameters) == ["n_frames", "n_pairs"]
    from wfl_asr_amd.infer import Labeler, infer_audio, infer_folder
    for f in (Labeler.label_files, infer_audio, infer_folder):
        params = inspect.signature(f).parameters
        assert list(params)[-1] == "bigram_scores" and params["bigram_scores"].default is None, f


def test_option_validation():
    """The rules and how the options are resolved against a config: tests/test_options_cpu.py.  Here: the Labeler resolves a request
    against its own config (a bare one: no model, no GPU)."""
    from wfl_asr_amd.infer import Labeler
    from wfl_asr_amd.options import PostOptions

    class Stub:
        config = {"postprocess": {"decode": "viterbi", "phoneme_bigram": "bg.json", "bigram_scores": True}}
    assert Labeler.options(Stub()) == PostOptions(decode="viterbi", phoneme_bigram="bg.json", bigram_scores=True)
    assert Labeler.options(Stub(), bigram_scores=False, switch_penalty=2).bigram_scores is False
    with pytest.raises(ValueError, match="decode_scores cannot be combined with a phoneme bigram.*bigram_scores"):
        Labeler.options(Stub(), decode_scores=True)
    Stub.config = {}                                  # no postprocess section: the defaults
    assert Labeler.options(Stub()) == PostOptions()
    with pytest.raises(ValueError, match="bigram_scores needs a phoneme_bigram"):
        Labeler.options(Stub(), decode="viterbi", bigram_scores=True)


def test_refused_before_any_model_is_loaded(tmp_path):
    from wfl_asr_amd import infer
    from wfl_asr_amd.infer import infer_audio, infer_folder

    def no_model(*a, **k):
        raise AssertionError("a model was asked for")
    saved = infer._labeler
    infer._labeler = no_model
    try:
        with pytest.raises(ValueError, match="bigram_scores needs"):
            infer_audio("x.wav", bigram_scores=True)
        with pytest.raises(ValueError, match="bigram_scores needs"):
            infer_audio("x.wav", config_path=str(tmp_path / "none.yaml"), bigram_scores=True)
        with pytest.raises(ValueError, match="bigram_scores needs decode='viterbi'"):
            infer_audio("x.wav", decode="argmax", bigram_scores=True)
        with pytest.raises(ValueError, match="bigram_scores needs a phoneme_bigram"):
            infer_folder(str(tmp_path), decode="viterbi", bigram_scores=True, config_path=str(tmp_path / "none.yaml"))
        # what the arguments leave open is taken from the config file: a bigram there is enough to get past the check
        cfg = tmp_path / "config.yaml"
        cfg.write_text("postprocess:\n  decode: viterbi\n  phoneme_bigram: bg.json\n")
        with pytest.raises(AssertionError, match="a model was asked for"):
            infer_audio("x.wav", config_path=str(cfg), bigram_scores=True)
        cfg.write_text("postprocess:\n  decode: viterbi\n")
        with pytest.raises(ValueError, match="bigram_scores needs a phoneme_bigram"):
            infer_audio("x.wav", config_path=str(cfg), bigram_scores=True)
    finally:
        infer._labeler = saved
