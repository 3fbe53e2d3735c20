#!/usr/bin/env python3
"""Records tests/golden/epilogue_parent.npz: the outputs of the cases in tests/epilogue_cases.py.  It was run once, on an MI355X, with
the library built from the commit before the epilogue trimming (WFL_LIB_PATH=<that build> python tests/golden/make_epilogue_parent.py);
tests/test_gpu_epilogue_identity.py holds every later build to these bits.  Running it again on a later build only makes sense after a
change that is MEANT to move the outputs.
usage: make_epilogue_parent.py [output.npz]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository root

import numpy as np

import epilogue_cases as E


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "epilogue_parent.npz")
    m = E.build_model()
    wav6 = E.clips(6)
    arrays = {}
    for name in E.CASES:
        for k, v in E.run_case(m, wav6, name).items():
            arrays[f"{name}.{k}"] = v
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes;", ", ".join(f"{k} {v.shape}" for k, v in arrays.items()))


if __name__ == "__main__":
    main()
