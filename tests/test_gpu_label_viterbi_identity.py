"""The Labeler's Viterbi-alignment path, held byte for byte to what the commit before its split into stages wrote and printed:
tests/golden/label_viterbi_parent.json, recorded by tests/golden/make_label_viterbi_parent.py over the folder and the seven runs of
tests/label_viterbi_cases.py (every .lab and .tsv of every run, and the run's stdout with the temporary directory spelled <TMP>).
One test, without a GPU, reads the record alone: it shows that the runs reached the fallbacks and sub-batches they were made for."""
import json
import os

import pytest

import label_viterbi_cases as L


@pytest.fixture(scope="module")
def parent(golden_dir):
    with open(os.path.join(golden_dir, "label_viterbi_parent.json"), encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return L.run_all(str(tmp_path_factory.mktemp("lv")))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(L.RUNS))
def test_every_file_and_every_printed_line_equal_the_parents(name, runs, parent):
    got, want = runs[name], parent[name]
    assert sorted(got["files"]) == sorted(want["files"])
    for f, text in want["files"].items():
        assert got["files"][f] == text, f"{name}: {f} differs from the parent's"
    assert got["stdout"] == want["stdout"]


def test_the_record_holds_the_paths_the_scenario_was_made_for(parent):
    from wfl_asr_amd import infer as I
    assert sorted(parent) == sorted(L.RUNS)
    labs = ["a.lab", "b.lab", "long.lab", "over.lab", "unknown.lab", "zplain.lab"]
    for name, rec in parent.items():
        assert [f for f in sorted(rec["files"]) if f.endswith(".lab")] == labs, name
        out = rec["stdout"]
        assert "200 tokens for 150 frames" in out and "'zz' matches no phoneme" in out, name       # over.wav, unknown.wav
    files = {name: sorted(rec["files"]) for name, rec in parent.items()}
    assert files["plain"] == labs and files["durations"] == labs
    scored = sorted(labs + ["a.scores.tsv", "b.scores.tsv", "long.scores.tsv", "alignment_scores.tsv"])
    assert files["scores"] == scored
    assert files["draft_scores"] == files["durations_scores_draft"] == files["kernel_fallback"] == sorted(scored + ["draft_moves.tsv"])
    assert files["edits_insertions"] == sorted(labs + [f"{s}.{k}.tsv" for s in ("a", "b", "long") for k in ("edits", "insertions")]
                                               + ["transcript_edits.tsv", "transcript_insertions.tsv"])
    a, b, over = ("<TMP>/wavs/%s.wav: " % n for n in ("a", "b", "over"))
    # b.wav: its draft's windows fall on the host; a.wav and b.wav lose their durations there; long.wav keeps both, and each file is
    # scored on the lattice it was searched on
    out = parent["draft_scores"]["stdout"]
    assert out.count(I.DRAFT_INFEASIBLE) == 1 and b + I.DRAFT_INFEASIBLE in out
    for name in ("durations", "durations_scores_draft"):
        out = parent[name]["stdout"]
        assert out.count(I.MIN_DURATION_INFEASIBLE) == 2 and a + I.MIN_DURATION_INFEASIBLE in out and b + I.MIN_DURATION_INFEASIBLE in out
    out = parent["durations_scores_draft"]["stdout"]
    assert out.count(I.DURATION_SCORES_PLAIN) == 2 and a + I.DURATION_SCORES_PLAIN in out and b + I.DURATION_SCORES_PLAIN in out
    assert out.count(I.DRAFT_INFEASIBLE) == 1 and "no alignment scores" not in out
    # with the host rule silenced the kernel's status sends a.wav, b.wav and over.wav through the first round and b.wav through the
    # second, and the files are the same
    out = parent["kernel_fallback"]["stdout"]
    assert out.count(I.MIN_DURATION_INFEASIBLE) == 3 and over + I.MIN_DURATION_INFEASIBLE in out and out.count(I.DRAFT_INFEASIBLE) == 1
    assert out.index(a + I.MIN_DURATION_INFEASIBLE) < out.index(b + I.MIN_DURATION_INFEASIBLE) < out.index(b + I.DRAFT_INFEASIBLE)
    assert parent["kernel_fallback"]["files"] == {f: t.replace("out_durations_scores_draft", "out_kernel_fallback")
                                                  for f, t in parent["durations_scores_draft"]["files"].items()}
    # the windows and the durations moved the alignment, the scores did not
    lab = {name: rec["files"] for name, rec in parent.items()}
    assert lab["scores"]["a.lab"] == lab["plain"]["a.lab"] == lab["durations"]["a.lab"] and lab["durations"]["b.lab"] == lab["plain"]["b.lab"]
    assert lab["durations"]["long.lab"] != lab["plain"]["long.lab"] != lab["draft_scores"]["long.lab"] != lab["durations_scores_draft"]["long.lab"]
    assert "no transcript edits (the file was not Viterbi-aligned)" in parent["edits_insertions"]["stdout"]
