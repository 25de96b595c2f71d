"""Generate tests/golden/cloud.npz -- the reference's own saved point cloud -- from the
reference's data files (no reference code runs).

  * DinoVisalizationData_avgnormals.npy, the pickle main.py:175-176 left behind and
    3Dvisualization.py:76-79 reads: points, colours and averaged view normals, each (688, 3),
    stored here as plain float64 arrays (tests/conftest.py loads with allow_pickle=False).
  * dino_normals.txt, the export of 3Dvisualization.py:139-145: its first 20 lines, as bytes.

Usage:  python tests/golden/make_golden_cloud.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _save  # noqa: E402

TXT_LINES = 20


def main():
    data = np.load(os.path.join(REF, "DinoVisalizationData_avgnormals.npy"), allow_pickle=True)
    points, colors, normals = (np.ascontiguousarray(a, dtype=np.float64) for a in data)
    assert points.shape == colors.shape == normals.shape == (688, 3)
    with open(os.path.join(REF, "dino_normals.txt"), "rb") as f:
        head = b"".join(f.readline() for _ in range(TXT_LINES))
    _save("cloud.npz", points=points, colors=colors, normals=normals,
          txt_head=np.frombuffer(head, dtype=np.uint8))


if __name__ == "__main__":
    main()
