"""The cases of tests/test_gpu_bigram_sumproduct_identity.py and of tests/golden/make_bigram_sumproduct_parent.py, which recorded their
expected outputs (tests/golden/bigram_sumproduct_parent.npz) once, on the GPU, from the commit BEFORE the sum-product chain of
bigram_post_chain_kernel and bigram_counts_chain_kernel was written once in csrc/bigram_sumproduct.h and the path-posterior pieces of
decode_post_chain_kernel moved to csrc/path_posterior.h.  The kernels built from the shared pieces must reproduce those outputs bit
for bit.  Inputs come from seeds; `ids` come from wfl_decode / wfl_decode_bigram.  The flat search's object is the one it was, so its
ids are inputs only; wfl_decode_bigram's entry was edited on the host side, so its ids, score and status are recorded too.

Every call is one ragged batch.  Shapes are the smallest at which a sweep can go wrong:
  bigram   P in test_gpu_decode_bigram.PHONEMES (empty wave slices, the J = 1 / 2 / 3 boundaries, N not divisible by 4, the cap), its
           tables and clips at BIGRAM_T (7 .. 17: the group boundaries at D = 8; 0: the empty clip; 300: many rescales), each with
           (forbid, threshold) in BIGRAM_CASES (-inf entries as exact zeros, forced frames, phonemes without an I class), through
           wfl_decode_bigram_posterior and wfl_decode_bigram_counts
  flat     the tables FLAT_TABLES of test_gpu_decode_posterior (the four slot configurations and their full cases) at FLAT_T
           (D = 16, 8, 4, 2), lambda in FLAT_LAMBDA, threshold in FLAT_THRESHOLD, through wfl_decode_posterior
  status   per entry: a class used twice (4), ids with an I frame after O (8), for the bigram posterior also ids that open a run
           through a forbidden succession (8), N = 193 symbols (2, no workspace), C = 1025 (2); the status is asserted here

The golden file stays under 256 KB: an output of more than FULL_BYTES bytes is kept as the SHA-256 of its bytes (pack, the rule of
tests/sumproduct_cases.py)."""
import numpy as np
import torch

import bio_viterbi_ref as R
import test_gpu_decode_bigram as SB
import test_gpu_decode_posterior as TP
from sumproduct_cases import pack
from wfl_asr_amd import decode as DC

BIGRAM_T = [1, 2, 7, 8, 9, 15, 16, 17, 0, 33, 300]
BIGRAM_CASES = ((0.0, 0.0), (0.3, 0.5))
FLAT_TABLES = ("p3", "p128", "p129", "p511", "p599")
FLAT_T = [1, 2, 15, 16, 17, 31, 32, 33, 65, 300]
FLAT_LAMBDA = (0.0, 2.5)
FLAT_THRESHOLD = (0.0, 0.5)


def _upload(clips, C):
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(clips) if clips else np.zeros((0, C), np.float32))).cuda(), [len(c) for c in clips]


def _host(**tensors):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in tensors.items()}


def run_bigram(lg, T, table, W, thr, ids_edit=None):
    """The search, the path's posteriors and the expected successions of one ragged call -> {entry.output: array}."""
    ids, score, vst = DC.bio_viterbi_bigram(lg, T, table, W, thr)
    out = _host(**{"search.ids": ids, "search.score": score, "search.status": vst})
    if ids_edit is not None:
        ids = torch.from_numpy(ids_edit(out["search.ids"].copy())).cuda()
    logz, post, cls, st = DC.decode_posteriors_bigram(lg, T, table, W, thr, ids)
    clz, counts, cst = DC.bigram_expected_counts(lg, T, table, W, thr)
    out.update(_host(**{"posterior.logz": logz, "posterior.post": post, "posterior.cls_post": cls, "posterior.status": st,
                        "counts.logz": clz, "counts.counts": counts, "counts.status": cst}))
    return out


def run_flat(lg, T, table, lam, thr, ids_edit=None):
    ids = DC.bio_viterbi(lg, T, table, lam, thr)[0]
    if ids_edit is not None:
        ids = torch.from_numpy(ids_edit(ids.cpu().numpy())).cuda()
    logz, post, cls, st = DC.decode_posteriors(lg, T, table, lam, thr, ids)
    return _host(logz=logz, post=post, cls_post=cls, status=st)


def flat_clips(name):
    """test_gpu_decode_posterior.make_clips at FLAT_T: random logits, every other clip with a planted path."""
    C, table, seed = TP.TABLES[name]
    rng = np.random.default_rng(1000 + seed)
    return [(rng.standard_normal((T, C)) * 3).astype(np.float32) if j % 2 == 0 else R.plant(T, C, table, rng, margin=2.0 if j % 4 == 1 else 12.0)[0]
            for j, T in enumerate(FLAT_T)]


def _first_frames(T, first):
    """ids edit for clips of T frames each, first[b] = (class, O's class): clip b becomes that class on frame 0 and O after it; a
    clip whose class is None keeps the search's path."""
    def edit(ids):
        for b, (c, o) in enumerate(first):
            if c is not None:
                ids[b * T:(b + 1) * T] = o
                ids[b * T] = c
        return ids
    return edit


def bigram_status_cases():
    """-> {name.entry.output: array}; every status is asserted."""
    res = {}
    P, T = 5, 20
    C, table = SB.make_table(P)                              # O = 1, B-p = 2 + 2p, I-p = 3 + 2p (p = 1 has none)
    rng = np.random.default_rng(7001)
    W = SB.make_trans(P, rng)
    W[0, 3] = -np.inf                                        # no run of phoneme 2 straight after O
    lg, Ts = _upload([R.plant(T, C, table, rng, margin=12.0)[0] for _ in range(3)], C)
    # clip 0 keeps the search's path; clip 1: I-0 on frame 0, after the virtual O frame; clip 2: B-2 on frame 0, through W[O][2] = -inf
    out = run_bigram(lg, Ts, table, W, 0.0, _first_frames(T, [(None, 1), (3, 1), (6, 1)]))
    assert out["posterior.status"].tolist() == [0, 8, 8] and out["counts.status"].tolist() == [0, 0, 0], out
    res.update({f"status.not_a_path.{k}": v for k, v in out.items()})
    out = run_bigram(lg, Ts, (1, [(2, 3), (4, -1), (6, 3), (8, 9), (10, 11)]), W, 0.0)        # class 3 twice
    assert all(out[k].tolist() == [4] * 3 for k in ("search.status", "posterior.status", "counts.status")), out
    res.update({f"status.class_twice.{k}": v for k, v in out.items()})
    P = 192                                                  # N = 193 symbols: over the cap, and no workspace
    C, table = SB.make_table(P)
    lg, Ts = _upload([rng.standard_normal((9, C)).astype(np.float32), rng.standard_normal((4, C)).astype(np.float32)], C)
    assert DC.bigram_posterior_workspace_bytes(Ts, P) == 0 and DC.bigram_counts_workspace_bytes(Ts, P) == 0
    out = run_bigram(lg, Ts, table, SB.make_trans(P, rng), 0.0)
    assert all(out[k].tolist() == [2] * 2 for k in ("search.status", "posterior.status", "counts.status")), out
    res.update({f"status.n193.{k}": v for k, v in out.items() if not k.startswith("counts.counts")})
    assert not out["counts.counts"].any()
    lg, Ts = _upload([rng.standard_normal((9, 1025)).astype(np.float32), rng.standard_normal((4, 1025)).astype(np.float32)], 1025)
    out = run_bigram(lg, Ts, (0, [(2 * p + 1, 2 * p + 2) for p in range(5)]), W, 0.0)
    assert all(out[k].tolist() == [2] * 2 for k in ("search.status", "posterior.status", "counts.status")), out
    res.update({f"status.c1025.{k}": v for k, v in out.items()})
    return res


def flat_status_cases():
    res = {}
    C, table, _ = TP.TABLES["p3"]                            # O = 0, (1, 2), (3, 4), (5, -1)
    T = 20
    rng = np.random.default_rng(7002)
    lg, Ts = _upload([R.plant(T, C, table, rng, margin=12.0)[0] for _ in range(2)], C)
    out = run_flat(lg, Ts, table, 1.5, 0.0, _first_frames(T, [(None, 0), (2, 0)]))           # clip 1: I-0 on frame 0
    assert out["status"].tolist() == [0, 8], out
    res.update({f"status.not_a_path.flat.{k}": v for k, v in out.items()})
    out = run_flat(lg, Ts, (0, [(1, 2), (3, 2), (5, -1)]), 1.5, 0.0)                          # class 2 twice
    assert out["status"].tolist() == [4, 4], out
    res.update({f"status.class_twice.flat.{k}": v for k, v in out.items()})
    lg, Ts = _upload([rng.standard_normal((9, 1025)).astype(np.float32), rng.standard_normal((4, 1025)).astype(np.float32)], 1025)
    out = run_flat(lg, Ts, table, 1.5, 0.0)
    assert out["status"].tolist() == [2, 2], out
    res.update({f"status.c1025.flat.{k}": v for k, v in out.items()})
    return res


def run_all():
    """-> {call.entry.output: array}, packed.  Every call of every case, in a fixed order."""
    res = {}
    for P in SB.PHONEMES:
        C, table, clips = SB.make_clips(P, SB.SEEDS[P], BIGRAM_T)
        lg, T = _upload(clips, C)
        for forbid, thr in BIGRAM_CASES:
            W = SB.make_trans(P, np.random.default_rng(2000 + P), forbid)
            out = run_bigram(lg, T, table, W, thr)
            assert all(not out[k].any() for k in ("search.status", "posterior.status", "counts.status")), (P, forbid, out)
            res.update({f"bigram.P{P}.forbid{forbid}.{k}": v for k, v in out.items()})
    for name in FLAT_TABLES:
        C, table, _ = TP.TABLES[name]
        lg, T = _upload(flat_clips(name), C)
        for lam in FLAT_LAMBDA:
            for thr in FLAT_THRESHOLD:
                out = run_flat(lg, T, table, lam, thr)
                assert not out["status"].any(), (name, lam, thr, out["status"])
                res.update({f"flat.{name}.lam{lam}.thr{thr}.{k}": v for k, v in out.items()})
    res.update(bigram_status_cases())
    res.update(flat_status_cases())
    return pack(res)
