"""-m gpu: wfl_align_graph (csrc/align_graph.hip) against the float64 numpy DP of tests/viterbi_graph_ref.py and against wfl_align, with
the checks and tolerances of tests/test_gpu_align.py::_check: the path is legal in the graph, its float64 score is within 1e-3 of the
reference optimum, `score` within 1e-3 T, and on planted logits states, ids, tok and taken equal the reference's.

Logits are random normal x 3.  Phonemes are drawn so that no slot shares one with any of the ten slots in front of it: that covers
the slots within two places on any path and the sibling variants' slots at the same place (tests/test_gpu_align_optional.py's rule
for _alts), so exact ties do not occur."""
import itertools

import numpy as np
import pytest
import torch

import viterbi_graph_ref as G
from wfl_asr_amd import align as AL

pytestmark = pytest.mark.gpu
C = 141
O_ID = 0
GAPS = [O_ID, 137, 138]


def _alts(N, rng):
    ph = []
    for k in range(N):
        while True:
            p = int(rng.integers(1, 68))
            if p not in ph[-10:]:
                break
        ph.append(p)
    return [[(2 * p - 1, 2 * p)] for p in ph]


def _run(clips):
    """clips: list of (z [T, C] float32, alternatives, preds, final) -> numpy (ids, tok, score, status, taken) per clip."""
    z = np.concatenate([c[0] for c in clips]) if clips else np.zeros((0, C), np.float32)
    lg = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    T = [len(c[0]) for c in clips]
    out = AL.viterbi_align_graph(lg, T, [c[1] for c in clips], [c[2] for c in clips], [c[3] for c in clips], [GAPS] * len(clips), O_ID)
    torch.cuda.synchronize()
    ids, tok, score, status, taken = (t.cpu().numpy() for t in out)
    res, pos, k0 = [], 0, 0
    for b, t in enumerate(T):
        n = len(clips[b][1])
        res.append((ids[pos:pos + t], tok[pos:pos + t], float(score[b]), int(status[b]), taken[k0:k0 + n]))
        pos += t
        k0 += n
    return res


def _run_chain(clips):
    """clips: list of (z, alternatives) -> wfl_align's numpy (ids, tok, score, status) per clip."""
    lg = torch.from_numpy(np.ascontiguousarray(np.concatenate([c[0] for c in clips]))).cuda()
    T = [len(c[0]) for c in clips]
    out = AL.viterbi_align(lg, T, [c[1] for c in clips], [GAPS] * len(clips), O_ID)
    torch.cuda.synchronize()
    ids, tok, score, status = (t.cpu().numpy() for t in out)
    res, pos = [], 0
    for b, t in enumerate(T):
        res.append((ids[pos:pos + t], tok[pos:pos + t], float(score[b]), int(status[b])))
        pos += t
    return res


def _path_states(ids, tok, alts):
    """(ids, tok) -> the state sequence the kernel walked (B classes are the odd ones here): a gap frame is in G of the next slot
    the path takes, G_end behind the last."""
    N = len(alts)
    s = np.zeros(len(ids), np.int64)
    nxt = N
    for t in range(len(ids) - 1, -1, -1):
        k = int(tok[t])
        if k < 0:
            s[t] = 3 * nxt
        else:
            s[t] = 3 * k + (1 if any(int(ids[t]) == b for b, _ in alts[k]) else 2)
            nxt = k
    return s


def _check(z, alts, preds, final, got, planted=None):
    ids, tok, score, status, taken = got
    T = len(z)
    ref, ref_score = G.viterbi(z, alts, preds, final, GAPS)
    if ref is None:
        assert status == 1
        assert (ids == O_ID).all() and (tok == -1).all() and (taken == 0).all() and score == 0.0
        return
    assert status == 0
    states = _path_states(ids, tok, alts)
    assert G.legal(states, preds, final), "the kernel's path is not a legal path of the graph"
    rid, rtok, rtaken = G.outputs(ref, z, alts, O_ID)
    mine = G.path_score(states, z, alts, GAPS)
    print(f"T {T} N {len(alts)}: path {mine:.6f} reference {ref_score:.6f} score {score:.6f}")
    assert mine >= ref_score - 1e-3, (mine, ref_score)
    assert abs(score - ref_score) <= 1e-3 * T, (score, ref_score)
    assert (taken == np.bincount(tok[tok >= 0], minlength=len(alts)).clip(0, 1)).all()
    if planted is not None:
        assert (ref == planted).all(), "the planted path is not the reference's optimum (test setup)"
        assert (states == ref).all()
        assert (ids == rid).all() and (tok == rtok).all() and (taken == rtaken).all()


# ------------------------------------------------------------------------------------------------------------ 1. chain graphs
def test_chain_graphs_are_wfl_align():
    rng = np.random.default_rng(21)
    clips = []
    for N in (0, 1, 5, 127, 128, 300, 512, 1024):
        T = N + int(rng.integers(3, 40))
        clips.append((rng.standard_normal((T, C)).astype(np.float32) * 3, _alts(N, rng)))
    clips.append((rng.standard_normal((20, C)).astype(np.float32) * 3, _alts(31, rng)))          # T < N: no path
    got = _run([(z, a, *AL.chain_graph(len(a))) for z, a in clips])
    want = _run_chain(clips)
    for (z, a), g, w in zip(clips, got, want):
        assert g[3] == w[3] and (g[0] == w[0]).all() and (g[1] == w[1]).all(), len(a)
        assert abs(g[2] - w[2]) <= 1e-3 * len(z), (len(a), g[2], w[2])
        assert (g[4] == (1 if g[3] == 0 else 0)).all()
    assert [g[3] for g in got] == [0] * 8 + [1] and got[-1][2] == 0.0 and (got[-1][1] == -1).all()


# ------------------------------------------------------------------------------------------------------------ 2. planted paths
KINDS = [(1, 3), (2, 0), (1, 2, 1)]           # variant lengths: 1 vs 3, 2 vs empty, three variants


def _graph_with_groups(N, starts, first_kind, last_kind):
    """~N slots: plain tokens, a group wherever the slot count reaches one of `starts` (kinds in turn), a group of first_kind as
    the first element and one of last_kind as the last -> (align.TranscriptGraph, the kind of every group)."""
    names = (f"s{i}" for i in itertools.count())
    starts, kinds, elements, count, turn = sorted(starts), [], [], 0, 0

    def group(kind):
        nonlocal count
        kinds.append(kind)
        elements.append(tuple(tuple(next(names) for _ in range(n)) for n in kind))
        count += sum(kind)
    group(first_kind)
    while count < N - sum(last_kind):
        if starts and count >= starts[0]:
            starts.pop(0)
            group(KINDS[turn % 3])
            turn += 1
        else:
            elements.append(next(names))
            count += 1
    group(last_kind)
    return AL.compile_graph(elements), kinds


def _ways(graph, kinds):
    """-> (the way through a non-first variant of every group, the way through the empty variants and else the first ones)."""
    def walk(pick):
        seq, k, gi = [], 0, 0
        for el in graph.elements:
            if isinstance(el, str):
                seq.append(k)
                k += 1
            else:
                a, b = graph.groups[gi][pick(kinds[gi])]
                seq.extend(range(a, b))
                k = graph.groups[gi][-1][1]
                gi += 1
        return seq
    return walk(lambda kind: len(kind) - 1), walk(lambda kind: kind.index(0) if 0 in kind else 0)


@pytest.mark.parametrize("N,R", [(100, 2), (300, 2), (800, 4), (1600, 8)])
def test_planted_paths_in_every_configuration(N, R):
    rng = np.random.default_rng(N)
    # groups around slots 0, 1 and R - 1 of a thread, on both sides of the first wave boundary, at 128 R, as first and last element
    starts = [4 * R, 7 * R + 1, 11 * R - 1, 64 * R - 2, 64 * R + 3, 128 * R - 1, 128 * R + 4]
    for first, last in ([(1, 3), (2, 0)], [(2, 0), (1, 2, 1)]):
        graph, kinds = _graph_with_groups(N, [s for s in starts if s < N - 12], first, last)
        assert abs(len(graph.slots) - N) <= 4
        alts = _alts(len(graph.slots), rng)
        clips, planted = [], []
        for seq in _ways(graph, kinds):
            T = len(seq) + len(seq) // 3 + 17
            z, st = G.plant(T, seq, C, alts, GAPS, rng)
            clips.append((z, alts, graph.preds, graph.final))
            planted.append(st)
        for clip, st, got in zip(clips, planted, _run(clips)):
            _check(*clip, got, st)


# ------------------------------------------------------------------------------------------------------------ 3. the existing kernel
def test_small_graphs_against_wfl_align_over_every_expansion():
    rng = np.random.default_rng(33)
    for trial in range(3):
        names = (f"s{i}" for i in itertools.count())
        elements, places = [], sorted(rng.choice(np.arange(0, 30), size=3, replace=False))
        for i in range(30):
            if i in places:
                lens = [int(x) for x in rng.integers(0 if trial else 1, 4, size=3)]
                if lens.count(0) > 1:
                    lens = [1, 0, 2]
                elements.append(tuple(tuple(next(names) for _ in range(n)) for n in lens))
            else:
                elements.append(next(names))
        graph = AL.compile_graph(elements)
        alts = _alts(len(graph.slots), rng)
        slot_of = {n: k for k, n in enumerate(graph.slots)}
        T = 120
        z = rng.standard_normal((T, C)).astype(np.float32) * 3
        got = _run([(z, alts, graph.preds, graph.final)])[0]
        _check(z, alts, graph.preds, graph.final, got)
        ways = [[slot_of[n] for n in toks] for toks in G.expansions(elements)]
        assert 8 <= len(ways) <= 27
        chains = _run_chain([(z, [alts[k] for k in way]) for way in ways])
        assert all(c[3] == 0 for c in chains)
        best = int(np.argmax([c[2] for c in chains]))
        assert abs(got[2] - chains[best][2]) <= 1e-3 * T, (got[2], chains[best][2])
        ctok = chains[best][1]
        as_slots = np.where(ctok >= 0, np.asarray(ways[best])[np.maximum(ctok, 0)], -1)
        assert (got[1] == as_slots).all() and (got[0] == chains[best][0]).all()
        assert sorted(np.nonzero(got[4])[0]) == sorted(ways[best])


# ------------------------------------------------------------------------------------------------------------ 4. status codes
def test_status_codes_and_undisturbed_neighbours():
    rng = np.random.default_rng(44)
    good_graph = AL.compile_graph(AL.parse_variants("a b ( c | d e ) f ( g | ) h".split()))
    good = (rng.standard_normal((40, C)).astype(np.float32) * 3, _alts(len(good_graph.slots), rng), good_graph.preds, good_graph.final)
    n = 6
    z = rng.standard_normal((30, C)).astype(np.float32) * 3
    alts = _alts(n, rng)
    preds, final = AL.chain_graph(n)

    def with_pred(k, row):
        return [row if j == k else p for j, p in enumerate(preds)]
    far_preds, far_final = AL.chain_graph(300)
    far_preds[299] = [298, 43]                                        # 256 slots back
    bad = {
        "a bad class": (z, [a if k != 2 else [(C + 3, 4)] for k, a in enumerate(alts)], preds, final),
        "a slot without a predecessor": (z, alts, with_pred(3, []), final),
        "a predecessor >= k": (z, alts, with_pred(3, [3]), final),
        "a later predecessor": (z, alts, with_pred(2, [1, 4]), final),
        "a predecessor < -2": (z, alts, with_pred(3, [2, -3]), final),
        "a predecessor 256 slots back": (rng.standard_normal((320, C)).astype(np.float32), _alts(300, rng), far_preds, far_final),
        "used entries not first": (z, alts, with_pred(3, [-2, 2]), final),
        "a slot_final of 2": (z, alts, preds, [0, 0, 0, 0, 0, 2]),
        "a negative slot_final": (z, alts, preds, [0, 0, 0, -1, 0, 1]),
        "no final slot": (z, alts, preds, [0] * n),
    }
    over = (rng.standard_normal((10, C)).astype(np.float32), _alts(2048, rng), *AL.chain_graph(2048))
    at_cap = (rng.standard_normal((5, C)).astype(np.float32), _alts(2047, rng), *AL.chain_graph(2047))      # at the cap: T < N, no path
    short = (good[0][:3],) + good[1:]                                 # the shortest way through needs 5 frames
    clips = [good] + list(bad.values()) + [good, over, at_cap, short, good]
    got = _run(clips)
    alone = _run([good])[0]
    for b in (0, len(bad) + 1, len(clips) - 1):                       # the good clips, bit for bit what they are alone
        assert got[b][3] == 0 and (got[b][0] == alone[0]).all() and (got[b][1] == alone[1]).all() and (got[b][4] == alone[4]).all()
        assert np.float32(got[b][2]).tobytes() == np.float32(alone[2]).tobytes()
    _check(*good, alone)
    for (what, clip), g in zip(bad.items(), got[1:]):
        assert g[3] == 4, what
        assert (g[0] == O_ID).all() and (g[1] == -1).all() and (g[4] == 0).all() and g[2] == 0.0, what
    for g, code in zip(got[len(bad) + 2:len(bad) + 5], (2, 1, 1)):
        assert g[3] == code and (g[0] == O_ID).all() and (g[1] == -1).all() and (g[4] == 0).all() and g[2] == 0.0
    # 5 frames are enough for the shortest way: a b c f h
    _check(good[0][:5], *good[1:], _run([(good[0][:5],) + good[1:]])[0])
    _check(*short, got[len(bad) + 4])


# ------------------------------------------------------------------------------------------------------------ 5. a ragged batch
def test_a_ragged_batch_of_6_equals_the_clips_alone():
    rng = np.random.default_rng(55)
    clips = []
    for N, starts in [(40, [5, 20]), (130, [64, 100]), (90, [10]), (600, [254, 300, 511]), (1100, [1022, 1030]), (260, [3, 128, 200])]:
        graph, _ = _graph_with_groups(N, starts, (1, 3), (1, 2, 1))
        T = len(graph.slots) + int(rng.integers(5, 60))
        clips.append((rng.standard_normal((T, C)).astype(np.float32) * 3, _alts(len(graph.slots), rng), graph.preds, graph.final))
    batch = _run(clips)
    for b, clip in enumerate(clips):
        alone = _run([clip])[0]
        assert batch[b][3] == alone[3] == 0
        assert (alone[0] == batch[b][0]).all() and (alone[1] == batch[b][1]).all() and (alone[4] == batch[b][4]).all()
        assert np.float32(alone[2]).tobytes() == np.float32(batch[b][2]).tobytes()
    for b in (0, 3):
        _check(*clips[b], batch[b])
