#!/usr/bin/env python3
"""Records tests/golden/side_reports_e2e_parent.json: every file written and every line printed by the runs of
tests/side_reports_e2e_cases.py.  It was run on an MI355X with the Python package of the commit before the side reports got their one
table, collector and writer (wfl-asr_amd/reports.py), twice, and the two recordings were identical;
tests/test_gpu_side_reports_identity.py holds every later build to this text.  A package found on PYTHONPATH wins over this
checkout's.  Running it again on a later build only makes sense after a change that is MEANT to move the outputs.
usage: make_side_reports_e2e_parent.py [output.json]"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.append(os.path.dirname(os.path.dirname(HERE)))         # the repository root, behind PYTHONPATH

import side_reports_e2e_cases as S


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "side_reports_e2e_parent.json")
    import wfl_asr_amd
    print("package:", os.path.dirname(wfl_asr_amd.__file__))
    with tempfile.TemporaryDirectory() as d:
        record = S.run_all(d)
    with open(out, "w", encoding="utf-8") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out, os.path.getsize(out), "bytes;", ", ".join(f"{k}: {len(v['files'])} files" for k, v in record.items()))


if __name__ == "__main__":
    main()
