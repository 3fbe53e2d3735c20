"""The side reports of a labelling run (wfl-asr_amd/reports.py), without a GPU, held string for string to
tests/golden/side_reports_parent.json: what the seven pairs of formatters and the per-kind writers of the commit before reports.py made
of the rows and the fake Labeler of tests/side_report_cases.py (recorded by tests/golden/make_side_reports_parent.py)."""
import json
import os
from types import SimpleNamespace

import pytest

import __graft_entry__  # noqa: F401
import side_report_cases as C
from wfl_asr_amd import infer as I
from wfl_asr_amd import reports as R
from wfl_asr_amd.options import resolve


@pytest.fixture(scope="module")
def parent(golden_dir):
    with open(os.path.join(golden_dir, "side_reports_parent.json"), encoding="utf-8") as f:
        return json.load(f)


def test_the_recorded_rows_are_the_cases_and_hold_the_edge_cases(parent):
    assert parent["rows"] == {kind: [[name, rows] for name, rows in C.ROWS[kind]] for kind in C.KINDS}
    assert list(R.REPORTS) == C.KINDS and sorted(parent["rows"]) == sorted(C.KINDS)
    for kind in C.KINDS:
        per_file = C.per_file(kind)
        assert len(per_file) >= 3 and per_file[-1][1] == []                                   # three files and more, an empty list
        spec = R.REPORTS[kind]
        if spec.order is not None:                                                            # equal sort keys: in one file, across two
            keys = [[spec.order(r) for r in rows if spec.keep is None or spec.keep(r)] for _, rows in per_file]
            assert any(len(set(ks)) < len(ks) for ks in keys)
            assert any(set(a) & set(b) for i, a in enumerate(keys) for b in keys[i + 1:])
        if spec.keep is not None:                                                             # a file with no row the folder file keeps
            assert any(rows and not any(spec.keep(r) for r in rows) for _, rows in per_file)
        if kind != "filler_scores":                                                           # (a kind without a name column)
            assert any("ñã" in "\t".join(spec.cells(r)) for _, rows in per_file for r in rows)                     # a non-ASCII name
    edits, ins = dict(C.per_file("edits")), dict(C.per_file("insertions"))
    assert any(r.best == "" and r.best_ratio == -C.INF and r.second == "" for r in edits["a.wav"])
    assert any(r.best == "" and r.best_ratio == -C.INF for r in ins["a.wav"])
    assert any(r.log_prior is None for r in dict(C.per_file("durations"))["a.wav"])
    assert any(r.names == () for r in dict(C.per_file("fillers"))["a.wav"])


@pytest.mark.parametrize("kind", C.KINDS)
def test_the_texts_of_every_kind_are_the_parents(kind, parent):
    rows = [(name, C.records(kind, rows)) for name, rows in parent["rows"][kind]]            # the records, rebuilt from the JSON
    assert rows == C.per_file(kind)
    for name, recs in rows:
        assert R.file_text(kind, recs) == parent["file_text"][kind][name], name
    assert R.file_text(kind, []) == R.REPORTS[kind].header + "\n"                             # an empty report: its header alone
    assert R.folder_text(kind, rows) == parent["folder_text"][kind]
    assert R.folder_text(kind, []) == "file\t" + R.REPORTS[kind].header + "\n"
    assert [n for n, _ in R.folder_rows(kind, rows)] == [ln.split("\t")[0] for ln in parent["folder_text"][kind].split("\n")[1:-1]]
    assert R.file_path(kind, "out/x.lab") == os.path.join("out", "x" + R.REPORTS[kind].suffix)


def test_the_table_states_what_was_scattered():
    assert list(R.REPORTS) == ["edits", "insertions", "skipped", "optional", "fillers", "filler_scores", "durations"]
    assert [k.suffix for k in R.REPORTS.values()] == [".edits.tsv", ".insertions.tsv", ".skipped.tsv", ".optional.tsv", ".fillers.tsv",
                                                      ".filler_scores.tsv", ".durations.tsv"]
    assert [k.stem for k in R.REPORTS.values()] == ["transcript_edits", "transcript_insertions", "skipped_tokens", "optional_scores",
                                                    "filler_spans", "filler_scores", "token_durations"]
    assert [k.missing for k in R.REPORTS.values()] == ["no transcript edits", "no transcript insertions", None, "no optional-token scores",
                                                       None, "no filler scores", "no duration-prior scores"]
    assert all(k.key == key for key, k in R.REPORTS.items())
    assert sorted(I.NOT_ALIGNED_LINES) == sorted(key for key, k in R.REPORTS.items() if k.missing is not None)
    # skipped and fillers are on with the option that makes them, `is not None`: a value that is not None and not true still reports
    off = dict(align_edits=False, align_insertions=False, optional_tokens=None, optional_scores=False, filler_token=None,
               filler_scores=False, duration_prior_scores=False)
    falsy = SimpleNamespace(**dict(off, optional_tokens=(), filler_token=""))
    assert [key for key, k in R.REPORTS.items() if k.enabled(falsy)] == ["skipped", "fillers"]
    assert not any(k.enabled(SimpleNamespace(**off)) for k in R.REPORTS.values())
    for group, (given, kinds) in C.GROUPS.items():
        assert list(R.Reports.for_options(resolve({"align": "viterbi"}, **given)).rows) == kinds, group
    assert list(R.Reports.for_options(resolve(None)).rows) == []


def _fake(kinds):
    """The fake Labeler: the real option rules, and canned() for the labelling."""
    class Fake:
        def options(self, **given):
            return resolve(None, **given)

        def _label_scored(self, audio_paths, opts, lang_id, confidence_threshold, verbose, reports=None):
            assert list(reports.rows) == kinds and all(v == {} for v in reports.rows.values()) and reports.moves == {}
            final, scores, rows = C.canned(audio_paths, opts, kinds)
            for fi in range(len(audio_paths)):
                reports.take(fi, {kind: rows[kind][fi] for kind in kinds if fi in rows[kind]})
            return final, scores
    return Fake()


@pytest.mark.parametrize("world", list(C.WORLDS))
@pytest.mark.parametrize("group", list(C.GROUPS))
def test_the_drivers_write_and_print_what_the_parents_did(group, world, parent, monkeypatch, tmp_path):
    fake = _fake(C.GROUPS[group][1])
    monkeypatch.setattr(I, "_labeler", lambda *a, **k: fake)
    for name, value in C.WORLDS[world].items():
        monkeypatch.setenv(name, value)
    got, want = C.drive(I, str(tmp_path), group), parent["drivers"][group][world]
    assert sorted(got["files"]) == sorted(want["files"])
    for f, text in want["files"].items():
        assert got["files"][f] == text, f
    assert got["stdout"] == want["stdout"]


@pytest.mark.parametrize("group", list(C.GROUPS))
def test_label_files_returns_the_parents_tuple(group, parent):
    given, kinds = C.GROUPS[group]
    lab = object.__new__(I.Labeler)
    lab.config = {}
    lab._label_scored = _fake(kinds)._label_scored
    got = lab.label_files(["in/" + n for n in C.FOLDER], align="viterbi", **given)
    want = parent["label_files"][group]
    assert json.loads(json.dumps(C.plain(got))) == want
    if not kinds:
        assert isinstance(got, list) and len(got) == len(C.FOLDER)                           # a bare `final`
    else:
        scored = int(resolve(None, align="viterbi", **given).scored)
        assert isinstance(got, tuple) and len(got) == 1 + scored + len(kinds)
        for kind, lists in zip(kinds, got[1 + scored:]):                                      # REPORTS' order; None for a file without rows
            assert lists[1] is None and lists[0] == C.records(kind, dict(C.ROWS[kind])["a.wav"])
            assert all(type(r).__name__ == C.RECORDS[kind] for r in lists[0] + lists[2])
