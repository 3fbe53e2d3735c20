"""-m gpu: wfl_align (csrc/align.hip) against the float64 numpy DP of tests/viterbi_ref.py on seeded random logits, ragged batches."""
import numpy as np
import pytest
import torch

import viterbi_ref as V
from wfl_asr_amd import align as AL

pytestmark = pytest.mark.gpu
C = 141
O_ID = 0
GAPS = [O_ID, 137, 138]


def _alts(N, rng, n_alt=1, repeat=False):
    out = []
    for k in range(N):
        if repeat and k % 3 == 1:
            out.append(out[-1])                       # the same token twice in a row
            continue
        ph = rng.choice(np.arange(1, 68), size=n_alt, replace=False)
        out.append([(int(2 * p - 1), int(2 * p)) for p in ph])
    return out


def _run(clips):
    """clips: list of (z [T, C] float32, alternatives) -> numpy (ids, tok, score, status) per clip."""
    z = np.concatenate([c[0] for c in clips]) if clips else np.zeros((0, C), np.float32)
    lg = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    T = [len(c[0]) for c in clips]
    ids, tok, score, status = AL.viterbi_align(lg, T, [c[1] for c in clips], [GAPS] * len(clips), O_ID)
    torch.cuda.synchronize()
    ids, tok, score, status = ids.cpu().numpy(), tok.cpu().numpy(), score.cpu().numpy(), status.cpu().numpy()
    out, pos = [], 0
    for b, t in enumerate(T):
        out.append((ids[pos:pos + t], tok[pos:pos + t], float(score[b]), int(status[b])))
        pos += t
    return out


def _path_states(ids, tok, alts):
    """(ids, tok) -> the state sequence the kernel walked (B classes are the odd ones here)."""
    s = np.zeros(len(ids), np.int64)
    done = 0                                           # tokens finished: a gap frame is in G_done
    for t in range(len(ids)):
        k = int(tok[t])
        if k < 0:
            s[t] = 3 * done
        else:
            is_b = any(int(ids[t]) == b for b, _ in alts[k])
            s[t] = 3 * k + (1 if is_b else 2)
            done = k + 1
    return s


def _check(z, alts, got, planted=None):
    ids, tok, score, status = got
    T, N = len(z), len(alts)
    ref, ref_score = V.viterbi(z, alts, GAPS)
    if T < N:
        assert status == 1
        assert (ids == O_ID).all() and (tok == -1).all()
        return
    assert status == 0
    states = _path_states(ids, tok, alts)
    assert V.legal(states, N), "the kernel's path is not a legal path"
    rid, rtok = V.outputs(ref, z, alts, O_ID)
    mine = V.path_score(states, z, alts, GAPS)
    assert mine >= ref_score - 1e-3, (mine, ref_score)
    assert abs(score - ref_score) <= 1e-3 * T, (score, ref_score)
    if planted is not None:
        assert (ref == planted).all(), "the planted path is not the reference's optimum (test setup)"
        assert (states == ref).all()
        assert (ids == rid).all() and (tok == rtok).all()


def test_ragged_batch_against_float64_dp():
    rng = np.random.default_rng(11)
    cases = []
    # (T, N, alternatives per token, equal neighbours, planted)
    for T, N, na, rep, pl in [(40, 1, 1, False, False), (40, 1, 1, False, True), (25, 25, 1, False, True), (60, 20, 1, True, True),
                              (90, 30, 4, False, True), (90, 30, 4, False, False), (300, 40, 2, True, False), (10, 12, 1, False, False),
                              (200, 90, 1, False, True), (700, 300, 1, False, False), (1500, 300, 1, False, True)]:
        alts = _alts(N, rng, na, rep)
        if pl:
            z, st = V.plant(T, N, C, alts, GAPS, rng)
        else:
            z, st = rng.standard_normal((T, C)).astype(np.float32) * 3, None
        cases.append((z, alts, st))
    got = _run([(z, a) for z, a, _ in cases])
    for (z, alts, st), g in zip(cases, got):
        _check(z, alts, g, st)


@pytest.mark.parametrize("T,N", [(2500, 1000), (4400, 4096)])
def test_multi_wave_transcripts(T, N):
    rng = np.random.default_rng(N)
    alts = _alts(N, rng, 1, True)
    z, st = V.plant(T, N, C, alts, GAPS, rng)
    z2 = rng.standard_normal((T, C)).astype(np.float32) * 2
    got = _run([(z, alts), (z2, alts)])
    _check(z, alts, got[0], st)
    _check(z2, alts, got[1])


def test_long_clip_and_over_cap_beside_feasible():
    rng = np.random.default_rng(5)
    alts = _alts(300, rng, 2)
    z, st = V.plant(15000, 300, C, alts, GAPS, rng)
    zr = rng.standard_normal((15000, C)).astype(np.float32) * 3
    big = _alts(4097, rng, 1)
    zb = rng.standard_normal((4200, C)).astype(np.float32)
    short = _alts(50, rng, 1)
    zs = rng.standard_normal((30, C)).astype(np.float32)
    got = _run([(z, alts), (zs, short), (zr, alts), (zb, big)])
    _check(z, alts, got[0], st)
    _check(zs, short, got[1])
    _check(zr, alts, got[2])
    assert got[3][3] == 2 and (got[3][0] == O_ID).all() and (got[3][1] == -1).all()


def test_a_clip_alone_equals_the_clip_in_a_batch_of_16():
    rng = np.random.default_rng(3)
    clips = []
    for b in range(16):
        N = int(rng.integers(1, 600))
        T = int(rng.integers(N, 2 * N + 200))
        clips.append((rng.standard_normal((T, C)).astype(np.float32) * 3, _alts(N, rng, int(rng.integers(1, 5)))))
    batch = _run(clips)
    for b in (0, 5, 15):
        alone = _run([clips[b]])[0]
        assert (alone[0] == batch[b][0]).all() and (alone[1] == batch[b][1]).all()
        assert np.float32(alone[2]).tobytes() == np.float32(batch[b][2]).tobytes() and alone[3] == batch[b][3]


def test_a_bad_class_id_is_reported_per_clip():
    rng = np.random.default_rng(9)
    alts = _alts(5, rng)
    z = rng.standard_normal((20, C)).astype(np.float32)
    lg = torch.from_numpy(np.concatenate([z, z])).cuda()
    bad = [list(a) for a in alts]
    bad[2] = [(C + 3, 4)]
    ids, tok, score, status = AL.viterbi_align(lg, [20, 20], [alts, bad], [GAPS, GAPS], O_ID)
    st = status.cpu().numpy()
    assert list(st) == [0, 4]
    assert (tok.cpu().numpy()[20:] == -1).all()
