#!/usr/bin/env python3
"""DEV-ONLY generator of tests/golden/adamw_bits.json.  Needs an MI355X and the library built from the commit whose bits are to
be kept: it was run at the parent of the change that moved the multi-tensor plumbing of csrc/optim.hip into csrc/multi_tensor.h
and pinned the second-moment form of the plain AdamW step, once per storage build:

    python tests/golden/make_golden_adamw_bits.py
    MC_STORAGE=f16 python tests/golden/make_golden_adamw_bits.py

Each run replaces its own storage build's section of the file and keeps the other.  The cases, the inputs and the digest are
those of tests/_adamw_bits_common.py, which the test uses too; the file holds case names and digests only."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository root


def main():
    import _adamw_bits_common as C
    from mammo_clip_amd import lib as L
    data = {}
    if os.path.exists(C.GOLDEN):
        with open(C.GOLDEN) as f:
            data = json.load(f)
    data[L.STORAGE] = C.run_all()
    with open(C.GOLDEN, "w") as f:
        json.dump(data, f, indent=0, sort_keys=True)
        f.write("\n")
    n = sum(len(v.split()) for case in data[L.STORAGE].values() for v in case.values())
    print(C.GOLDEN, L.STORAGE, len(data[L.STORAGE]), "cases", n, "digests", os.path.getsize(C.GOLDEN), "bytes")
    assert os.path.getsize(C.GOLDEN) <= 200_000


if __name__ == "__main__":
    main()
