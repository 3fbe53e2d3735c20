"""No GPU: pronunciation variants (`postprocess.transcript_variants`) -- the parser and the graph compiler of align.py, the float64
restatement of wfl_align_graph (tests/viterbi_graph_ref.py) against the maximum of tests/viterbi_ref.py over every expansion of the
transcript, the option's rules, the report rows, and the host side of the ABI entry."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__  # noqa: F401
import viterbi_graph_ref as G
import viterbi_ref as V
from wfl_asr_amd import _lib, align as AL, options as O, reports as R
from wfl_asr_amd.options import resolve

EXAMPLE = "k a ( t | d ) o ( N | ) ( ts u | s u )"
NC = 41
GAPS = [0]


# ------------------------------------------------------------------------------------------------------------ parser and compiler
def test_the_example_compiles_to_its_slots_predecessors_and_finals():
    el = AL.parse_variants(EXAMPLE.split())
    assert el == ["k", "a", (("t",), ("d",)), "o", (("N",), ()), (("ts", "u"), ("s", "u"))]
    assert AL.parse_variants("k a (t|d) o (N|) (ts u|s u)".split()) == el              # attached to a name or alone
    assert AL.parse_variants(["k", "a(t", "|d)o(", "N", "|)(ts", "u|s", "u)"]) == el
    g = AL.compile_graph(el)
    assert g.slots == ["k", "a", "t", "d", "o", "N", "ts", "u", "s", "u"]
    assert g.preds == [[-1], [0], [1], [1], [2, 3], [4], [5, 4], [6], [5, 4], [8]]
    assert g.final == [0, 0, 0, 0, 0, 0, 0, 1, 0, 1]
    assert g.groups == [[(2, 3), (3, 4)], [(5, 6), (6, 6)], [(6, 8), (8, 10)]]
    assert [g.slots[k] for k in g.first] == "k a t o N ts u".split()
    assert g.spelling(2, 1) == "s u" and g.spelling(1, 1) == ""
    # groups as first and as last element, an optional first element: START travels with the frontier
    g = AL.compile_graph(AL.parse_variants("( a | ) b ( c | d e )".split()))
    assert g.preds == [[-1], [0, -1], [1], [1], [3]] and g.final == [0, 0, 1, 0, 1]


def test_a_transcript_without_groups_compiles_to_the_chain():
    toks = "a b c d".split()
    assert not AL.has_variants(toks) and AL.has_variants(["a", "b)"])
    g = AL.compile_graph(AL.parse_variants(toks))
    assert (g.preds, g.final) == AL.chain_graph(4) == ([[-1], [0], [1], [2]], [0, 0, 0, 1])
    assert g.groups == [] and g.first == [0, 1, 2, 3] and g.slots == toks
    assert AL.chain_graph(0) == ([], [])


@pytest.mark.parametrize("text,message", [
    ("a ( b | ( c | d ) )", "word 5: a group inside the group opened at word 2 (variants do not nest)"),
    ("a ( b | c", "word 2: '(' is never closed"),
    ("a b ) c", "word 3: ')' without a '('"),
    ("a | b", "word 2: '|' outside a group"),
    ("a ( b ) c", "word 4: the group opened at word 2 needs at least 2 distinct variants"),
    ("a ( b | b ) c", "word 6: the group opened at word 2 needs at least 2 distinct variants"),
    ("a ( b | c | d | e | f )", "word 12: the group opened at word 2 has 5 variants (at most 4)"),
])
def test_the_parser_refuses_by_place(text, message):
    with pytest.raises(ValueError) as e:
        AL.parse_variants(text.split())
    assert str(e.value) == message


def test_duplicates_collapse_with_one_line_and_the_compiler_refuses():
    notes = []
    assert AL.parse_variants("( a | b | a ) c".split(), notes) == [(("a",), ("b",)), "c"]
    assert notes == ["the group opened at word 1 repeats a variant: 1 dropped"]
    with pytest.raises(ValueError, match="every element of the transcript is a group with an empty variant: it could spell nothing"):
        AL.compile_graph(AL.parse_variants("( a | ) ( b | c | )".split()))
    # four adjacent optional groups of two non-empty variants each: the token behind them would follow 8 slots and the one in front
    many = "x " + " ".join(f"( a{i} | b{i} | )" for i in range(4)) + " y"
    with pytest.raises(ValueError, match=r"element 6: token 'y' would need 9 predecessors \(at most 8\)"):
        AL.compile_graph(AL.parse_variants(many.split()))
    AL.compile_graph(AL.parse_variants(("x " + " ".join(f"( a{i} | b{i} | )" for i in range(3)) + " y").split()))      # 7: fine
    big = [(tuple(f"p{i}" for i in range(200)), tuple(f"q{i}" for i in range(56)))]
    with pytest.raises(ValueError, match=r"element 1: a group of 256 slots \(at most 255\)"):
        AL.compile_graph(big + ["z"])
    ok = AL.compile_graph([(tuple(f"p{i}" for i in range(200)), tuple(f"q{i}" for i in range(55))), "z"])
    assert ok.preds[255] == [199, 254] and max(255 - p for p in ok.preds[255]) <= AL.MAX_SPAN
    assert AL.variant_name_collisions(["a", "b(", "c|d", "e"]) == ["b(", "c|d"]


# ------------------------------------------------------------------------------------------------------------ the reference
def _alts_for(names, rng):
    """A (B, I) pair per token name, one phoneme per distinct name."""
    uniq = sorted(set(names))
    ph = dict(zip(uniq, rng.choice(np.arange(1, (NC - 1) // 2 + 1), size=len(uniq), replace=False)))
    return [[(int(2 * ph[n] - 1), int(2 * ph[n]))] for n in names]


def _random_elements(rng):
    pool = [f"p{i}" for i in range(12)]
    out = []
    for _ in range(int(rng.integers(1, 6))):
        if rng.random() < 0.5:
            out.append(str(rng.choice(pool)))
            continue
        while True:
            group = tuple(dict.fromkeys(tuple(str(x) for x in rng.choice(pool, size=int(rng.integers(0, 4))))
                                        for _ in range(int(rng.integers(2, 4)))))
            if len(group) >= 2:
                break
        out.append(group)
    return out


def test_the_reference_optimum_is_the_maximum_over_all_expansions():
    rng = np.random.default_rng(2024)
    done = infeasible = 0
    while done < 200:
        el = _random_elements(rng)
        try:
            g = AL.compile_graph(el)
        except ValueError:
            continue                                                   # (all groups optional: could spell nothing)
        T = int(rng.integers(1, 14))
        z = rng.standard_normal((T, NC)) * 3
        names = sorted(set(g.slots))
        ph = dict(zip(names, rng.choice(np.arange(1, 21), size=len(names), replace=False)))
        pair = {n: [(int(2 * ph[n] - 1), int(2 * ph[n]))] for n in names}
        states, score = G.viterbi(z, [pair[n] for n in g.slots], g.preds, g.final, GAPS)
        best = None
        for toks in G.expansions(el):
            st, sc = V.viterbi(z, [pair[n] for n in toks], GAPS)
            if st is not None and (best is None or sc > best):
                best = sc
        if best is None:
            assert states is None
            infeasible += 1
        else:
            assert states is not None and abs(score - best) <= 1e-9, (el, T, score, best)
            assert G.legal(states, g.preds, g.final)
            assert abs(G.path_score(states, z, [pair[n] for n in g.slots], GAPS) - score) <= 1e-9
        done += 1
    assert 5 <= infeasible <= 150


def test_on_a_chain_the_reference_is_viterbi_refs_state_for_state():
    rng = np.random.default_rng(7)
    for T, N in [(1, 0), (5, 0), (1, 1), (9, 1), (12, 12), (30, 7), (40, 13), (4, 6)]:
        alts = [[(int(2 * p - 1), int(2 * p))] for p in rng.choice(np.arange(1, 21), size=N, replace=N > 20)]
        z = rng.standard_normal((T, NC)) * 3
        want, wsc = V.viterbi(z, alts, GAPS)
        got, gsc = G.viterbi(z, alts, *AL.chain_graph(N), GAPS)
        if want is None:
            assert got is None
            continue
        assert (got == want).all() and abs(gsc - wsc) <= 1e-12
        ids, tok, taken = G.outputs(got, z, alts, 0)
        wid, wtok = V.outputs(want, z, alts, 0)
        assert (ids == wid).all() and (tok == wtok).all() and (taken == 1).all()


def test_plant_goes_through_the_chosen_variants():
    rng = np.random.default_rng(3)
    g = AL.compile_graph(AL.parse_variants(EXAMPLE.split()))
    alts = _alts_for(g.slots, rng)
    seq = [0, 1, 3, 4, 8, 9]                                           # d, no N, s u
    z, st = G.plant(30, seq, NC, alts, GAPS, rng)
    assert G.legal(st, g.preds, g.final)
    got, _ = G.viterbi(z, alts, g.preds, g.final, GAPS)
    assert (got == st).all()
    assert list(G.outputs(got, z, alts, 0)[2]) == [1, 1, 0, 1, 1, 0, 0, 0, 1, 1]


# ------------------------------------------------------------------------------------------------------------ the option
def test_option_rules_50_to_52():
    base = {"align": "viterbi"}
    assert resolve(base).transcript_variants is False and resolve(None).transcript_variants is False
    a = resolve(base, transcript_variants=True)
    assert a.transcript_variants is True and resolve(dict(base, transcript_variants=True)) == a
    assert resolve(dict(base, transcript_variants=True), transcript_variants=False).transcript_variants is False
    for bad in (1, "yes", 0.5):
        with pytest.raises(ValueError, match="transcript_variants must be true or false"):
            resolve(base, transcript_variants=bad)
    with pytest.raises(ValueError, match="transcript_variants needs align='viterbi'"):
        resolve(None, transcript_variants=True)
    beside = {"align_draft": "drafts", "min_duration": 0.04, "optional_tokens": ["a"], "filler_token": "<x>", "duration_prior": "d.json",
              "align_scores": True, "align_edits": True, "align_insertions": True}
    assert set(beside) < set(O.CHAIN_ONLY_OPTIONS) and len(O.CHAIN_ONLY_OPTIONS) == 12
    for name, value in beside.items():
        with pytest.raises(ValueError) as e:
            resolve(base, transcript_variants=True, **{name: value})
        assert str(e.value) == O.transcript_variants_error([name]), name
    # the scorers that need an option of their own are refused with it: both by name, in the table's order
    for name, needs in [("duration_scores", {"min_duration": 0.04}), ("optional_scores", {"optional_tokens": "*"}),
                        ("filler_scores", {"filler_token": "<x>"}), ("duration_prior_scores", {"duration_prior": "d.json"})]:
        with pytest.raises(ValueError) as e:
            resolve(base, transcript_variants=True, **needs, **{name: True})
        assert str(e.value) == O.transcript_variants_error(list(needs) + [name]), name
    assert "cannot be combined with align_scores, align_edits:" in O.transcript_variants_error(["align_scores", "align_edits"])
    # the free decode's options are not the alignment's: they stay
    assert resolve(base, transcript_variants=True, decode="viterbi", decode_scores=True).transcript_variants is True
    assert " 50. " in O.__doc__ and " 51. " in O.__doc__ and " 52. " in O.__doc__
    # the record
    plain = resolve(base)
    assert "transcript_variants" in O.PostOptions._KEYWORD and len(O.PostOptions._KEYWORD) == len(O.PostOptions._KEYWORD_DEFAULTS)
    assert a != plain and hash(a) != hash(plain) and a._replace(transcript_variants=False) == plain
    assert a._asdict()["transcript_variants"] is True and "transcript_variants=True" in repr(a)
    assert O.PostOptions._make(tuple(a), transcript_variants=True).transcript_variants is True
    assert plain == tuple(plain) and not a.scored


# ------------------------------------------------------------------------------------------------------------ the report
def test_the_report_rows_from_a_hand_made_taken():
    g = AL.compile_graph(AL.parse_variants(EXAMPLE.split()))
    taken = [1, 1, 0, 1, 1, 0, 0, 0, 1, 1]                             # k a d o - s u
    segs = [(0.0, 0.1, "k"), (0.1, 0.2, "a"), (0.2, 0.35, "d"), (0.35, 0.5, "o"), (0.6, 0.7, "s"), (0.7, 0.9, "u")]
    rows = AL.variant_choices(g, taken, segs, 2.5)
    assert rows == [R.VariantChoice(0, 0.2, 0.35, 1, "d", "t", 2.5), R.VariantChoice(1, 0.6, 0.6, 1, "", "N", 2.5),
                    R.VariantChoice(2, 0.6, 0.9, 1, "s u", "ts u", 2.5)]
    assert R.file_text("variants", rows) == ("index\tstart_s\tend_s\tvariant\tspelling\twritten\tgain_nats\n"
                                             "0\t0.2000000\t0.3500000\t1\td\tt\t2.5\n"
                                             "1\t0.6000000\t0.6000000\t1\t\tN\t2.5\n"
                                             "2\t0.6000000\t0.9000000\t1\ts u\tts u\t2.5\n")
    as_written = AL.variant_choices(g, [1, 1, 1, 0, 1, 1, 1, 1, 0, 0],
                                    [(0.1 * i, 0.1 * i + 0.1, n) for i, n in enumerate("k a t o N ts u".split())], None)
    assert [r.choice for r in as_written] == [0, 0, 0] and as_written[0].gain is None
    assert R.file_text("variants", as_written).splitlines()[1].endswith("\tt\tt\tnone")
    # an optional group at the end: the time of the place is the end of the last segment
    h = AL.compile_graph(AL.parse_variants("a ( b | )".split()))
    assert AL.variant_choices(h, [1, 0], [(0.0, 0.4, "a")], 0.0) == [R.VariantChoice(0, 0.4, 0.4, 1, "", "b", 0.0)]
    with pytest.raises(ValueError, match="not one variant"):
        AL.variant_choices(g, [1, 1, 1, 1, 1, 0, 0, 0, 1, 1], segs + [(0.9, 1.0, "x")], 0.0)
    # the folder file: only the choices that are not as written, the file with the largest gain first, a file without one last
    small = [r._replace(gain=0.5) for r in rows[:1]]
    none = [r._replace(gain=None) for r in rows[1:2]]
    text = R.folder_text("variants", [("a.wav", small), ("w.wav", as_written), ("n.wav", none), ("b.wav", rows)])
    lines = text.splitlines()
    assert lines[0] == "file\t" + R.KINDS["variants"].header
    assert [ln.split("\t")[0] for ln in lines[1:]] == ["b.wav", "b.wav", "b.wav", "a.wav", "n.wav"]
    # the table: the kind is on with the option alone, and the seven chain kinds stay the table they were
    assert list(R.KINDS) == list(R.REPORTS) + ["variants"] and R.KINDS["variants"].stem == "transcript_variants"
    assert list(R.Reports.for_options(resolve({"align": "viterbi"}, transcript_variants=True)).rows) == ["variants"]
    assert list(R.Reports.for_options(resolve({"align": "viterbi"})).rows) == []
    assert R.file_path("variants", "out/x.lab").endswith("x.variants.tsv")


# ------------------------------------------------------------------------------------------------------------ the ABI's host side
def test_the_entry_is_bound_and_checks_its_arguments_on_the_host():
    lib = _lib.load()
    for name in ("wfl_align_graph", "wfl_align_graph_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["wfl_align_graph"][1]) == 21

    def h(*v):
        return np.array(v, np.int32).ctypes.data_as(C.c_void_p)
    # per frame NT words(N) + 1 end word, rounded up to 64 words per clip; nothing over the cap or without a frame
    for T, N, words in [(10, 5, 65), (10, 127, 65), (10, 128, 257), (10, 1023, 257), (10, 1024, 513), (10, 2047, 513), (3, 0, 65)]:
        assert lib.wfl_align_graph_workspace_bytes(h(T), h(N), 1) == (T * words + 63) // 64 * 64 * 4, (T, N)
    assert lib.wfl_align_graph_workspace_bytes(h(10), h(2048), 1) == 0 and lib.wfl_align_graph_workspace_bytes(h(0), h(5), 1) == 0
    assert lib.wfl_align_graph_workspace_bytes(h(4, 10), h(9, 5), 2) == (320 + 704) * 4          # T < N keeps its words: a graph may skip
    assert lib.wfl_align_graph_workspace_bytes(None, None, 0) == 0 and lib.wfl_align_graph_workspace_bytes(None, None, 1) == -1
    assert AL.graph_workspace_bytes([10], [5]) == 704 * 4
    d = C.c_void_p(64)                                                # never dereferenced: every call below returns on the host
    fo = np.array([0], np.int64).ctypes.data_as(C.c_void_p)

    def call(C_=41, pred=d, fin=d, taken=d, ws=d, ws_bytes=1 << 20, n=1):
        return lib.wfl_align_graph(d, 41, C_, 0, fo, h(10), h(0), h(5), d, d, n, pred, fin, ws, ws_bytes, d, d, d, taken, d, None)
    assert call(C_=0) == -1 and b"wfl_align_graph: C must" in lib.wfl_last_error()
    for kw in ({"pred": None}, {"fin": None}, {"taken": None}):
        assert call(**kw) == -1 and b"wfl_align_graph: null device" in lib.wfl_last_error()
    assert call(ws_bytes=16) == -1 and b"wfl_align_graph: workspace too small (wfl_align_graph_workspace_bytes)" in lib.wfl_last_error()
    assert call(n=0) == 0
    assert AL._ENTRIES["wfl_align_graph"] == ("wfl_align_graph", False, False)
