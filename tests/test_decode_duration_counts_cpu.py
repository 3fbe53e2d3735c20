"""CPU (-m "not gpu"): the host side of the free decode's duration EM -- the float64 expected run lengths and successions of
tests/bio_duration_counts_ref.py against the enumeration of every class string, the identities of include/wfl_asr.h on the reference,
its agreement with the bigram counts reference (no prior) and the duration posterior reference (logz), the EM bound over three rounds in
float64 (durations alone, and with the bigram re-estimated jointly), the ABI entries, the workspace formula, and the argument errors
of the Python entry and of `python -m wfl_asr_amd.adapt_decode_durations` that need no GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import bio_bigram_counts_ref as BC
import bio_bigram_ref as RB
import bio_duration_counts_ref as CR
import bio_duration_posterior_ref as DP
import bio_duration_ref as R
from wfl_asr_amd import decode as DC
from wfl_asr_amd import durations as DU
from wfl_asr_amd import phonotactics as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = (1, [(0, 2), (3, 4), (5, -1)])          # tests/test_gpu_decode_duration.py's: O, two phonemes with I, one without
TINY_C = 6


def _tables(D, rng, forbid):
    W = -3.0 * rng.random((4, 4))
    mask = rng.random((4, 4)) < forbid
    mask[:, 0] = False
    W[mask] = -np.inf
    dur = -6.0 * rng.random((3, D + 1))
    dur[rng.random(dur.shape) < forbid] = -np.inf
    sd = rng.integers(-1, 3, size=3).astype(np.int32)
    return W, dur.astype(np.float32), sd


def _forbidden(dur, sd):
    D = dur.shape[1] - 1
    out = np.zeros((len(sd), D + 1), bool)
    for p, r in enumerate(sd):
        if r >= 0:
            out[p] = np.isneginf(dur[r])
            out[p, D] |= np.isneginf(dur[r, D - 1])
    return out


@pytest.mark.parametrize("D", [1, 2, 3, 4, 8])
def test_reference_equals_the_enumeration_and_keeps_the_identities(D):
    """Clips of 1 .. 6 frames, with and without forced frames, forbidden entries and sym_dur = -1.  At D <= 3 the tail and column D
    are reached (asserted); at D = 8 the ring never fills."""
    rng = np.random.default_rng(900 + D)
    seen = dict(forced=0, forbidden=0, no_row=0, excess=0.0)
    for trial in range(30):
        T = 1 + trial % 6
        z = rng.standard_normal((T, TINY_C)) * 2
        W, dur, sd = _tables(D, rng, 0.25 if trial % 2 else 0.0)
        forced = rng.random(T) < 0.3 if trial % 3 == 0 else None
        logz, succ, dc = CR.expected_counts(z, TINY, W, dur, sd, forced)
        want = CR.brute_force(z, TINY, W, dur, sd, forced)
        assert abs(logz - want[0]) <= 1e-10 and np.abs(succ - want[1]).max() <= 1e-10 and np.abs(dc - want[2]).max() <= 1e-10, trial
        forb = _forbidden(dur, sd)
        assert (succ >= 0).all() and succ[0, 0] == 0 and (succ[np.isneginf(W)] == 0).all()
        assert (dc >= 0).all() and (dc[forb] == 0).all()
        # every run is opened once; the frames of the phonemes are at most T
        assert np.abs(dc[:, :D].sum(1) - succ[:, 1:].sum(0)).max() <= 1e-12
        lens = np.concatenate([np.arange(1, D + 1), [1]])
        assert (dc * lens).sum() <= T + 1e-12
        if D == 8:
            assert not dc[:, T:].any()             # no run is longer than the clip
        r32 = CR.expected_counts(z, TINY, W, dur, sd, forced, dtype=np.float32)
        assert abs(r32[0] - logz) <= 1e-4 and np.abs(r32[1] - succ).max() <= 1e-4 and np.abs(r32[2] - dc).max() <= 1e-4
        seen["forced"] += 0 if forced is None else int(forced.sum())
        seen["forbidden"] += int(forb.sum())
        seen["no_row"] += int((sd < 0).sum())
        seen["excess"] += float(dc[:, D].sum())
    assert seen["forced"] and seen["forbidden"] and seen["no_row"]
    assert (seen["excess"] > 0) == (D <= 4), seen


def test_frames_of_a_phoneme_are_its_posterior_frames():
    """sum_j (j + 1) dc[p][j] + D dc[p][D - 1] + dc[p][D] is the posterior number of frames of p: against the enumeration's per-frame
    class posteriors."""
    rng = np.random.default_rng(17)
    for D in (1, 2, 3):
        z = rng.standard_normal((6, TINY_C)) * 2
        W, dur, sd = _tables(D, rng, 0.0)
        _, _, dc = CR.expected_counts(z, TINY, W, dur, sd, None)
        paths, tot = DP.path_weights(z, TINY, W, dur, sd, None)
        good = np.isfinite(tot)
        pw = np.exp(tot[good] - np.logaddexp.reduce(tot[good]))
        lens = np.concatenate([np.arange(1, D + 1), [1]])
        for p, (b, i) in enumerate(TINY[1]):
            frames = float((pw[:, None] * np.isin(paths[good], [b] + ([i] if i >= 0 else []))).sum())
            assert abs(float((dc[p] * lens).sum()) - frames) <= 1e-10, (D, p)


@pytest.mark.parametrize("prior", ["none", "zero"])
def test_without_a_prior_succ_and_logz_are_the_bigram_counts(prior):
    rng = np.random.default_rng(23)
    table = (0, [(1, 2), (3, 4), (5, -1)])
    for T, D in ((1, 1), (7, 3), (60, 8)):
        z = rng.standard_normal((T, 8)) * 3
        forced = rng.random(T) < 0.2
        W = -6.0 * rng.random((4, 4))
        dur = np.zeros((2, D + 1), np.float32)
        sd = np.full(3, -1, np.int32) if prior == "none" else np.array([0, 1, 0], np.int32)
        logz, succ, dc = CR.expected_counts(z, table, W, dur, sd, forced)
        blz, bcn = BC.expected_counts(z, table, W, forced)
        assert abs(logz - blz) <= 1e-11 * max(1.0, abs(blz)) and np.abs(succ - bcn).max() <= 1e-11


def test_logz_is_the_posterior_reference_s():
    rng = np.random.default_rng(29)
    table = (0, [(1, 2), (3, 4), (5, -1)])
    for T, D in ((1, 2), (9, 3), (50, 4)):
        z = rng.standard_normal((T, 8)) * 3
        forced = rng.random(T) < 0.2
        W = -6.0 * rng.random((4, 4))
        dur = (-3.0 * rng.random((3, D + 1))).astype(np.float32)
        sd = np.array([2, -1, 0], np.int32)
        ids = np.full(T, 0, np.int32)              # all-O is a path of every table
        logz = CR.expected_counts(z, table, W, dur, sd, forced)[0]
        want = DP.forward_backward(z, table, W, dur, sd, forced, ids)[0]
        assert abs(logz - want) <= 1e-12 * max(1.0, abs(want))


def _em(joint):
    """Three float64 EM rounds on eight seeded clips from the flat prior (and, joint, the uniform bigram), smoothing 0, weights 1,
    penalty 0 -> sum logZ per round and the number of terms a round's sum is made of."""
    from wfl_asr_amd import adapt_bigram as AB
    P, C, D = 4, 10, 4
    table = (0, [(1, 2), (3, 4), (5, 6), (7, -1)])
    labels = ["O", "B-a", "I-a", "B-b", "I-b", "B-c", "I-c", "B-d", "x", "y"]
    ct = DC.class_table(labels)
    assert ct.o_id == table[0] and [tuple(p) for p in ct.pairs.tolist()] == table[1]
    syms = AB.symbols_of(labels)
    rng = np.random.default_rng(5)
    clips = [rng.standard_normal((int(rng.integers(20, 60)), C)) * 2 for _ in range(4)]
    clips += [RB.plant(int(rng.integers(30, 60)), C, table, rng, margin=2.0, scale=1.5)[0].astype(np.float64) for _ in range(4)]
    prior = DU.flat(syms[1:], D)
    bg = AB.uniform_bigram(syms)
    totals = []
    for k in range(4):
        W = np.where(np.isfinite(bg.log_prob), bg.log_prob, -np.inf)
        W[0, 0] = 0.0
        dur = np.zeros((P, D + 1))
        sd = np.full(P, -1, np.int32)
        for i, r in enumerate(prior.log_prob):
            if r is not None:
                dur[i], sd[i] = np.concatenate([r, [prior.log_tail[i]]]), i      # (no float32 rounding of the table)
        tot, succ, dc = 0.0, np.zeros((P + 1, P + 1)), np.zeros((P, D + 1))
        for z in clips:
            lz, s, d = CR.expected_counts(z, table, W, dur, sd, None)
            tot, succ, dc = tot + lz, succ + s, dc + d
        totals.append(tot)
        prior = DU.reestimate(dc, syms[1:], D)
        if joint:
            bg = PH.reestimate(succ, syms)
    frames = sum(len(z) for z in clips)
    return totals, frames * (P + 1) * (D + 2)


@pytest.mark.parametrize("joint", [False, True])
def test_em_rounds_never_lower_the_sum_of_logz(joint):
    """The EM bound.  A round's sum logZ is a log-sum over at most frames x symbols x (D + 2) terms per clip, each rounded once in
    float64: it is reproduced to within that many ulps of its magnitude, and a decrease beyond that would break the bound."""
    totals, terms = _em(joint)
    bound = terms * np.spacing(max(abs(t) for t in totals))
    print(f"joint {joint}: sum logZ per round:", " ".join(f"{t:.9f}" for t in totals), f"; rounding bound {bound:.3e}")
    assert all(b >= a - bound for a, b in zip(totals, totals[1:])), totals
    assert totals[-1] > totals[0] + 1e-3, "the rounds did not move the tables (test setup)"


# ------------------------------------------------------------------------------------------------------- ABI and Python entry
def _formula(T, N, D):
    """include/wfl_asr.h: the workspace of one clip, in bytes."""
    r64 = lambda x: (x + 63) // 64 * 64                         # noqa: E731
    HS = r64(N)
    in_lds = 16 * ((4 * N * (N | 1) + 15) // 16) + 6912 + 4 * (4 * D + 3) * HS <= 163840 - 4608
    return 4 * (r64(T * (4 * N + 2)) + (0 if in_lds else r64((4 * D + 3) * HS)) + 2 * r64(T)) if T > 0 else 0, in_lds


def test_abi_entries_and_the_workspace_formula():
    from wfl_asr_amd import _lib
    src = open(os.path.join(ROOT, "include", "wfl_asr.h")).read()
    for name in ("wfl_decode_duration_counts_workspace_bytes", "wfl_decode_duration_counts"):
        assert re.search(rf"\b{name}\s*\(", src) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["wfl_decode_duration_counts"][1]) == 22
    assert len(_lib.SIGNATURES["wfl_decode_duration_counts_workspace_bytes"][1]) == 4
    assert int(re.search(r"#define\s+WFL_ABI_VERSION\s+(\d+)", src).group(1)) == 2
    import __graft_entry__ as g
    g.build()
    lib = _lib.load()
    assert lib.wfl_decode_duration_counts is not None and lib.wfl_abi_version() == 2
    T = np.array([10, 0, 7], np.int32)
    sides = set()
    for P, D in ((0, 1), (70, 8), (70, 32), (127, 32), (128, 32), (140, 22), (140, 23), (191, 1), (191, 32)):
        want = 0
        for t in T:
            b, in_lds = _formula(int(t), P + 1, D)
            want += b
        sides.add(in_lds)
        assert DC.duration_counts_workspace_bytes(T, P, D) == want, (P, D)
    assert sides == {True, False}
    assert _formula(10, 128, 32)[1] and not _formula(10, 129, 32)[1] and _formula(10, 141, 22)[1] and not _formula(10, 141, 23)[1]
    assert DC.duration_counts_workspace_bytes(T, 192, 8) == 0                # over the cap: nothing is counted
    h = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)           # noqa: E731
    size = lib.wfl_decode_duration_counts_workspace_bytes
    assert size(h(T), 3, 70, 0) == -1 and size(h(T), 3, 70, 33) == -1 and size(h(T), 3, 192, 33) == -1
    assert size(h(T), -1, 70, 8) < 0 and size(h(T), 3, -1, 8) < 0 and size(None, 1, 70, 8) < 0 and size(None, 0, 70, 8) == 0
    with pytest.raises(_lib.WflError):
        DC.duration_counts_workspace_bytes(T, 70, 0)


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

    def call(C=141, o_id=0, ldl=141, fo_=fo, T_=T, ws=None, ws_bytes=0, logits=d, n=1, pairs=d, n_pairs=70, trans=d, sym_dur=d, dur=d,
             n_rows=3, D=8, thr=0.0, logz=d, succ=d, dc=d, status=d):
        return lib.wfl_decode_duration_counts(logits, ldl, C, o_id, h(fo_) if fo_ is not None else None, h(T_), n, pairs, n_pairs, trans,
                                              sym_dur, dur, n_rows, D, thr, ws, ws_bytes, logz, succ, dc, status, None)

    need = lib.wfl_decode_duration_counts_workspace_bytes(h(T), 1, 70, 8)
    assert need == _formula(10, 71, 8)[0]
    for kw, word in ((dict(C=0), b"C < 1"), (dict(o_id=141), b"o_id"), (dict(ldl=100), b"ldl"), (dict(n=-1), b"negative count"),
                     (dict(n_pairs=-1), b"negative count"), (dict(thr=-0.1), b"threshold"), (dict(D=0), b"D must be"),
                     (dict(D=33), b"D must be"), (dict(n_rows=-1), b"n_rows"), (dict(dur=None), b"null dur"),
                     (dict(fo_=None, ws=d, ws_bytes=need), b"null host"),
                     (dict(T_=np.array([-2], np.int32), ws=d, ws_bytes=need), b"negative"),
                     (dict(logits=None, ws=d, ws_bytes=need), b"null device"), (dict(logz=None, ws=d, ws_bytes=need), b"null device"),
                     (dict(succ=None, ws=d, ws_bytes=need), b"null device"), (dict(dc=None, ws=d, ws_bytes=need), b"null device"),
                     (dict(status=None, ws=d, ws_bytes=need), b"null device"), (dict(pairs=None, ws=d, ws_bytes=need), b"null device"),
                     (dict(trans=None, ws=d, ws_bytes=need), b"null device"), (dict(sym_dur=None, ws=d, ws_bytes=need), b"null sym_dur"),
                     (dict(ws=d, ws_bytes=need - 1), b"workspace"), (dict(ws=None, ws_bytes=need), b"workspace")):
        assert call(**kw) != 0, kw
        err = lib.wfl_last_error()
        assert b"wfl_decode_duration_counts" in err and word in err, (kw, err)
    assert call(n=0) == 0                          # nothing to do
    assert call(n=0, trans=None, succ=None, dc=None) == 0


def test_parameter_lists_and_the_python_entry_s_checks():
    assert list(inspect.signature(DC.duration_expected_counts).parameters) == ["logits", "n_frames", "table", "trans", "dur", "sym_dur",
                                                                               "threshold", "frame_offsets", "stream"]
    assert list(inspect.signature(DC.duration_counts_workspace_bytes).parameters) == ["n_frames", "n_pairs", "D"]
    from wfl_asr_amd.infer import Labeler
    assert list(inspect.signature(Labeler.expected_free_durations).parameters) == [
        "self", "audio_paths", "trans", "prior", "weight", "lang_id", "confidence_threshold", "verbose"]
    import torch
    with pytest.raises(ValueError, match="float32 CUDA"):          # (the first check: needs no device)
        DC.duration_expected_counts(torch.zeros((10, 8)), [10], TINY, np.zeros((4, 4), np.float32), np.zeros((1, 3), np.float32),
                                    np.zeros(3, np.int32), 0.0)


# ----------------------------------------------------------------------------------------------------------------- the tool
def _model_dir(tmp_path, labels):
    save = tmp_path / "model"
    save.mkdir()
    (save / "phonemes.txt").write_text("\n".join(labels) + "\n")
    cfg = tmp_path / "config.yaml"
    cfg.write_text(f"output:\n  save_dir: {save}\npostprocess:\n  decode: viterbi\n")
    return str(cfg)


def test_the_tool_refuses_bad_requests_before_any_model_is_loaded(tmp_path, capsys):
    from wfl_asr_amd import adapt_decode_durations as AD
    from wfl_asr_amd import infer

    class NoModel:
        def __init__(self, *a, **k):
            raise AssertionError("a model was asked for")
    saved = infer.Labeler
    infer.Labeler = NoModel
    try:
        labels = ["O", "B-a", "I-a", "B-b"]
        cfg = _model_dir(tmp_path, labels)
        wav = tmp_path / "x.wav"
        wav.write_bytes(b"RIFF")
        out = str(tmp_path / "out.json")
        base = ["-ckpt", "none.pt", "-c", cfg, "-o", out]

        def refused(args, word):
            with pytest.raises(SystemExit) as e:
                AD.main(args)
            assert e.value.code == 2
            assert word in capsys.readouterr().err, word
        empty = tmp_path / "empty"
        empty.mkdir()
        refused([str(empty), str(tmp_path / "nothing.wav")] + base, "no audio file found")
        refused([str(wav)] + base + ["--iterations", "0"], "--iterations")
        refused([str(wav)] + base + ["--smoothing", "-1"], ">= 0")
        refused([str(wav)] + base + ["--prior-count", "2"], "--prior-count needs --init")
        refused([str(wav)] + base + ["--max-frames", "33"], "--max-frames must be 1 .. 32")
        refused([str(wav)] + base + ["--switch-penalty", "-1"], "must be >= 0")
        # an --init counted on another clock, and one whose D is not the one asked for
        DU.save(DU.flat(["a", "b"], 8, 0.01), tmp_path / "clock.json")
        refused([str(wav)] + base + ["--init", str(tmp_path / "clock.json")], "frames of 0.01 s")
        DU.save(DU.flat(["a", "b"], 8), tmp_path / "d8.json")
        refused([str(wav)] + base + ["--init", str(tmp_path / "d8.json"), "--max-frames", "16"], "fixes D")
        # a bigram the label set refuses
        PH.save(PH.Bigram(["O", "a", "z"], np.log(np.full((3, 3), 0.5))), tmp_path / "other.json")
        refused([str(wav)] + base + ["--phoneme-bigram", str(tmp_path / "other.json")], "lacks phonemes of the label set")
        # a label set above 191 phonemes
        big = tmp_path / "big"
        big.mkdir()
        cfg_big = _model_dir(big, ["O"] + [f"B-p{i}" for i in range(192)])
        refused([str(wav), "-ckpt", "none.pt", "-c", cfg_big, "-o", out], "at most 191")
        # a good request gets as far as the model
        with pytest.raises(AssertionError, match="a model was asked for"):
            AD.main([str(wav)] + base + ["--init", str(tmp_path / "d8.json"), "--bigram-output", str(tmp_path / "bg.json")])
        assert not os.path.exists(out)
        with pytest.raises(SystemExit):
            AD.main(["--help"])
        text = capsys.readouterr().out
        assert "cannot decrease" in " ".join(text.split()) and "informative only" in " ".join(text.split())
    finally:
        infer.Labeler = saved
