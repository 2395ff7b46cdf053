"""Packs tools/dump_ambi_tables.cpp's JSON (stdin) into the fixture tests/golden/ambi_tables.npz (argv[1]): float32 matrices and
scale tables, uint8 index tables, under the reference's own names (the index tables prefixed "Index")."""
import json
import sys

import numpy as np


def main():
    tables = json.load(sys.stdin)
    arrays = {}
    for name, value in tables.items():
        arrays[name] = np.asarray(value, np.uint8 if name.startswith("Index") else np.float32)
    assert len(arrays) == 14, sorted(arrays)
    for name, rows in (("FirstOrderUp", 4), ("FirstOrder2DUp", 4), ("SecondOrderUp", 9), ("SecondOrder2DUp", 9), ("ThirdOrderUp", 16),
                       ("ThirdOrder2DUp", 16), ("FourthOrder2DUp", 25)):
        assert arrays[name].shape == (rows, 25), (name, arrays[name].shape)
    np.savez_compressed(sys.argv[1], **arrays)
    print(sys.argv[1], {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
