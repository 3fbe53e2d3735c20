#!/usr/bin/env python3
"""Records tests/golden/side_reports_parent.json from the rows and the fake Labeler of tests/side_report_cases.py: the per-file and the
folder text of every kind of side report, what infer_folder and infer_audio write and print per group of options (once as the only
process, once as rank 1 of 2), and what Labeler.label_files returns per group.  It was run, without a GPU, with the Python package of
the commit before the side reports got their one table, collector and writer (wfl-asr_amd/reports.py): the formatters and writers named
below and the keyword arguments of `label_scored` are that commit's, and they are gone since, so the script documents the recording and
is not run again.  tests/test_side_reports_cpu.py holds every later build to this text.
usage: make_side_reports_parent.py [output.json]"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.append(os.path.dirname(os.path.dirname(HERE)))         # the repository root, behind PYTHONPATH

import side_report_cases as C


def _read(write, *args):
    with tempfile.TemporaryDirectory() as d:
        write(os.path.join(d, "x.tsv"), *args)
        with open(os.path.join(d, "x.tsv"), "rb") as f:
            return f.read().decode("utf-8")


def formatters(AL):
    """kind -> (per-file text of rows, folder text of [(file name, rows)]), the parent's."""
    return {"edits": (lambda rows: _read(AL.write_edits_tsv, rows), lambda pf: _read(AL.write_folder_edits, pf)),
            "insertions": (lambda rows: _read(AL.write_insertions_tsv, rows), lambda pf: _read(AL.write_folder_insertions, pf)),
            "skipped": (AL.format_skipped_tsv, AL.format_folder_skipped_tsv),
            "optional": (AL.format_optional_tsv, AL.format_folder_optional_tsv),
            "fillers": (AL.format_fillers_tsv, AL.format_folder_fillers_tsv),
            "filler_scores": (AL.format_filler_scores_tsv, AL.format_folder_filler_scores_tsv),
            "durations": (AL.format_durations_tsv, AL.format_folder_durations_tsv)}


def label_scored(kinds):
    """The fake Labeler._label_scored with the parent's signature: canned() into the dicts the caller handed in."""
    def fake(audio_paths, opts, lang_id, confidence_threshold, verbose, moves=None, edits=None, insertions=None, skipped=None,
             optional=None, fillers=None, filler_scores=None, durations=None):
        into = dict(edits=edits, insertions=insertions, skipped=skipped, optional=optional, fillers=fillers,
                    filler_scores=filler_scores, durations=durations)
        assert sorted(k for k, v in into.items() if v is not None) == sorted(kinds)
        final, scores, rows = C.canned(audio_paths, opts, kinds)
        for kind, by_file in rows.items():
            into[kind].update(by_file)
        return final, scores
    return fake


class FakeLabeler:
    def __init__(self, kinds):
        self._label_scored = label_scored(kinds)

    def options(self, **given):
        from wfl_asr_amd.options import resolve
        return resolve(None, **given)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "side_reports_parent.json")
    import wfl_asr_amd
    from wfl_asr_amd import align as AL
    from wfl_asr_amd import infer as I
    print("package:", os.path.dirname(wfl_asr_amd.__file__))
    record = {"rows": {kind: [[name, rows] for name, rows in C.ROWS[kind]] for kind in C.KINDS}, "file_text": {}, "folder_text": {},
              "drivers": {}, "label_files": {}}
    for kind, (one, folder) in formatters(AL).items():
        record["file_text"][kind] = {name: one(rows) for name, rows in C.per_file(kind)}
        record["folder_text"][kind] = folder(C.per_file(kind))
    for group, (given, kinds) in C.GROUPS.items():
        fake = FakeLabeler(kinds)
        I._labeler = lambda *a, **k: fake
        record["drivers"][group] = {}
        for world, env in C.WORLDS.items():
            os.environ.update(env)
            with tempfile.TemporaryDirectory() as d:
                record["drivers"][group][world] = C.drive(I, d, group)
        lab = object.__new__(I.Labeler)
        lab.config = {}
        lab._label_scored = label_scored(kinds)
        record["label_files"][group] = C.plain(lab.label_files(["in/" + n for n in C.FOLDER], align="viterbi", **given))
    with open(out, "w", encoding="utf-8") as f:
        json.dump(record, f, indent=1, sort_keys=True, ensure_ascii=False)
        f.write("\n")
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
