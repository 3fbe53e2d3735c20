#!/usr/bin/env python3
"""Records tests/golden/bigram_sumproduct_parent.npz: the outputs of the cases in tests/bigram_sumproduct_cases.py.  It was run on an
MI355X with the library built from the commit before the bigram sum-product chain moved into csrc/bigram_sumproduct.h
(WFL_LIB_PATH=<that build> python tests/golden/make_bigram_sumproduct_parent.py), twice, and the two recordings were equal;
tests/test_gpu_bigram_sumproduct_identity.py holds every later build to these bits.  Running it again on a later build only makes
sense after a change that is MEANT to move the outputs.
usage: make_bigram_sumproduct_parent.py [output.npz]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository root

import numpy as np

import bigram_sumproduct_cases as S


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "bigram_sumproduct_parent.npz")
    arrays = S.run_all()
    np.savez_compressed(out, **arrays)
    full = sum(1 for k in arrays if not k.endswith(".sha256"))
    print(out, os.path.getsize(out), "bytes;", len(arrays), "outputs,", full, "of them in full")
    for k, v in arrays.items():
        if k.startswith("status.") and k.endswith(".status"):
            print(" ", k, v.tolist())


if __name__ == "__main__":
    main()
