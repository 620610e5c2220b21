#!/usr/bin/env python3
"""Golden vectors for the trainer's augmentations: runs the REAL reference module's build_horizontal_flip_permutation and
build_rotate180_permutation (azchess/encoding.py:310-386, called from training/train.py:288-300) and records the two 73-entry
arrays they return.  Build container only; the module's `chess` import is served by tools/refshim.py.

Output tests/golden/ref_augment_perm.json: {"horizontal_flip": [73 ints], "rotate180": [73 ints]}."""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refshim          # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "ref_augment_perm.json")


def main():
    refshim.install()
    enc = importlib.import_module("azchess.encoding")
    blob = {"horizontal_flip": [int(x) for x in enc.build_horizontal_flip_permutation()],
            "rotate180": [int(x) for x in enc.build_rotate180_permutation()]}
    assert all(sorted(v) == list(range(73)) for v in blob.values())
    with open(OUT, "w") as f:
        json.dump(blob, f)
        f.write("\n")
    print("wrote", os.path.relpath(OUT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
