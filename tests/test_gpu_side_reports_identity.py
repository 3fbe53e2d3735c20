"""The side reports of a labelling run end to end, held string for string to what the commit before wfl-asr_amd/reports.py wrote and
printed: tests/golden/side_reports_e2e_parent.json, recorded by tests/golden/make_side_reports_e2e_parent.py over the folder and the
four runs of tests/side_reports_e2e_cases.py (every .lab and .tsv of every run, and the run's stdout with the temporary directory
spelled <TMP>).  One test, without a GPU, reads the record alone: it shows that the runs wrote the reports they were made for."""
import json
import os

import pytest

import side_reports_e2e_cases as S

NAMES = list(S.RUNS) + [S.AUDIO_RUN]


@pytest.fixture(scope="module")
def parent(golden_dir):
    with open(os.path.join(golden_dir, "side_reports_e2e_parent.json"), encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return S.run_all(str(tmp_path_factory.mktemp("sr")))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_every_file_and_every_printed_line_equal_the_parents(name, runs, parent):
    got, want = runs[name], parent[name]
    assert sorted(got["files"]) == sorted(want["files"])
    for f, text in want["files"].items():
        assert got["files"][f] == text, f"{name}: {f} differs from the parent's"
    assert got["stdout"] == want["stdout"]


def test_the_record_holds_the_reports_the_scenario_was_made_for(parent):
    assert sorted(parent) == sorted(NAMES)
    labs = ["a.lab", "b.lab", "c.lab", "d.lab"]
    files = {name: sorted(rec["files"]) for name, rec in parent.items()}
    scored = ["alignment_scores.tsv", "b.scores.tsv"]
    assert files["optional"] == sorted(labs + scored + ["b.skipped.tsv", "b.optional.tsv", "skipped_tokens.tsv", "optional_scores.tsv"])
    assert files["filler"] == sorted(labs + scored + ["a.scores.tsv", "a.fillers.tsv", "a.filler_scores.tsv", "b.filler_scores.tsv",
                                                      "filler_spans.tsv", "filler_scores.tsv"])
    assert files["duration_prior"] == sorted(labs + scored + ["b.durations.tsv", "token_durations.tsv"])
    assert files[S.AUDIO_RUN] == ["a.filler_scores.tsv", "a.fillers.tsv", "a.lab", "a.scores.tsv"]
    a, c = "<TMP>/side/a.wav: ", "<TMP>/side/c.wav: "
    for name, what in (("optional", "optional-token"), ("filler", "filler"), ("duration_prior", "duration-prior")):
        out = parent[name]["stdout"]
        line = f"no {what} scores (the file was not Viterbi-aligned)"
        assert "'zz' matches no phoneme" in out and c + line in out, name
        assert out.count(line) == (1 if name == "filler" else 2) and (a + line in out) == (name != "filler"), name
    # every report holds rows: the skipped tokens, both decisions of the optional ones, the one filler, a token without a prior row
    rec = parent["optional"]["files"]
    assert rec["b.skipped.tsv"].count("\n") == 17 and "\tkept\t" in rec["b.optional.tsv"] and "\tskipped\t" in rec["b.optional.tsv"]
    rec = parent["filler"]["files"]
    assert rec["a.fillers.tsv"].count("\n") == 2 and rec["a.filler_scores.tsv"].count("\n") == 2 and rec["b.filler_scores.tsv"].count("\n") == 1
    assert rec["a.fillers.tsv"] == parent[S.AUDIO_RUN]["files"]["a.fillers.tsv"]
    rec = parent["duration_prior"]["files"]
    assert rec["b.durations.tsv"].count("\n") == 42 and "\tnone\t" in rec["b.durations.tsv"] and "\tnone\t" not in rec["token_durations.tsv"]
