"""align.AlignBatch, the Labeler's record of a wave's ragged batch, and align.reuses_packed, the one rule for running a scoring call on
the PackedClips of the search or on tables packed again.  No library, no GPU: the logits are a stand-in with a shape."""
from types import SimpleNamespace

import numpy as np

from wfl_asr_amd import align as AL

LG = SimpleNamespace(shape=(12, 13))
ALTS = [[[(1, 2)], [(3, 4)]], [[(5, 6)]], [[(1, 2)], [(1, 2)], [(3, 4)]]]
GAPS = [[0], [0, 7], [0]]
W1 = [(0, 2)]
D2 = [2, 1, 1]


def _batch(wins=None, mins=None):
    return AL.AlignBatch.of(LG, [4, 3, 5], ALTS, GAPS, 0, wins, mins)


def test_no_constraint_in_the_batch_is_none_and_one_is_the_whole_list():
    b = _batch()
    assert b.windows is None and b.min_frames is None
    assert b.f0.tolist() == [0, 4, 7] and b.f0.dtype == np.int64
    assert b.args() == (LG, [4, 3, 5], ALTS, GAPS, 0)
    b = _batch(wins=[None, W1, None])
    assert b.windows == [None, W1, None] and b.min_frames is None
    b = _batch(mins=[None, None, D2])
    assert b.windows is None and b.min_frames == [None, None, D2]


def test_select_keeps_the_order_the_offsets_and_the_clips_own_constraints():
    b = _batch(wins=[None, W1, None], mins=[[1, 3], None, D2])
    s = b.select([2, 0])
    assert s.frames == [5, 4] and s.f0.tolist() == [7, 0]
    assert s.alts == [ALTS[2], ALTS[0]] and s.gaps == [GAPS[2], GAPS[0]]
    assert s.wins == [None, None] and s.mins == [D2, [1, 3]] and s.min_frames == [D2, [1, 3]]
    assert s.lg is LG and s.o_id == 0
    assert s.args() == (LG, [5, 4], [ALTS[2], ALTS[0]], [GAPS[2], GAPS[0]], 0)
    assert b.frames == [4, 3, 5] and b.wins == [None, W1, None]                   # the parent is as it was
    one = b.select(np.array([1]))
    assert one.frames == [3] and one.f0.tolist() == [4] and one.windows == [W1] and one.min_frames is None


def test_a_sub_batch_without_windows_has_none_although_its_parent_has_some():
    b = _batch(wins=[None, W1, None])
    assert b.windows is not None and b.select([0, 2]).windows is None
    b = _batch(mins=[None, None, D2])
    assert b.select([0, 1]).min_frames is None and b.select([2]).min_frames == [D2]


def test_reuse_or_repack_row_by_row_of_the_docstring_table():
    plain = AL.PackedClips(3, 0, 0, 0, 0, 0, 0)                                    # (d_win, d_min: None)
    with_min = AL.PackedClips(3, 0, 0, 0, 0, 0, 0, None, object())
    windowed = AL.PackedClips(3, 0, 0, 0, 0, 0, 0, object())
    rows = [                       # packed, clips of the batch, clips selected, with_min -> reuse
        (None, 3, 3, False, False), (None, 3, 2, False, False), (None, 3, 3, True, False),
        (plain, 3, 3, False, True), (windowed, 3, 3, False, True),
        (plain, 3, 2, False, False),
        (with_min, 3, 3, True, True),
        (with_min, 3, 2, True, False),
        (with_min, 3, 3, False, False), (with_min, 3, 1, False, False),
        (plain, 3, 3, True, False), (plain, 3, 2, True, False),
    ]
    for packed, n, k, m, want in rows:
        assert AL.reuses_packed(packed, n, k, m) is want, (packed, n, k, m)


def test_scored_on_hands_back_the_search_tables_only_where_the_rule_allows(monkeypatch):
    packs = []
    monkeypatch.setattr(AL, "pack_clips", lambda *a, **kw: packs.append((a, kw)) or "packed again")
    b = _batch(wins=[None, W1, None], mins=[None, None, D2])
    search = AL.PackedClips(3, 0, 0, 0, 0, 0, 0, object())
    sub, got = b.scored_on([0, 1, 2], search, False)
    assert got is search and sub.frames == b.frames and not packs
    sub, got = b.scored_on([1, 2], search, False)
    assert got == "packed again" and sub.frames == [3, 5]
    (lg, frames, alts, gaps, f0), kw = packs.pop()
    assert lg is LG and frames == [3, 5] and alts == ALTS[1:] and gaps == GAPS[1:] and f0.tolist() == [4, 7]
    assert kw == dict(windows=[W1, None], min_frames=None)                          # no durations for a score without them
    b.scored_on([2], search, True)
    assert packs.pop()[1] == dict(windows=None, min_frames=[D2])
    assert b.pack(False) == "packed again" and packs.pop()[1] == dict(windows=[None, W1, None], min_frames=None)
    assert b.pack(True) == "packed again" and packs.pop()[1] == dict(windows=[None, W1, None], min_frames=[None, None, D2])
