"""Generate tests/golden/evaluation.npz from the reference's data files (no reference code runs).

  * imgdata/dino_Ps.mat, the true cameras evaluation.py:5-7 loads: P (36, 3, 4) float64.
  * R_eval_clean.npy (35, 3, 3) and t_eval_clean.npy (35, 3), the estimated cameras main.py:180-181
    saved through Tables.getCamerasForEvaluation.  main.py:93 adds views 2..34 to the first two,
    so estimate i belongs to P[i], i = 0..34.

Usage:  python tests/golden/make_golden_evaluation.py   (needs scipy for the .mat file)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _save  # noqa: E402


def main():
    import scipy.io as sio
    cell = sio.loadmat(os.path.join(REF, "imgdata", "dino_Ps.mat"))["P"]
    P = np.ascontiguousarray([p for p in cell[0]], dtype=np.float64)
    R = np.ascontiguousarray(np.load(os.path.join(REF, "R_eval_clean.npy")), dtype=np.float64)
    t = np.ascontiguousarray(np.load(os.path.join(REF, "t_eval_clean.npy")), dtype=np.float64)
    assert P.shape == (36, 3, 4) and R.shape == (35, 3, 3) and t.shape == (35, 3)
    _save("evaluation.npz", P=P, R_eval_clean=R, t_eval_clean=t)


if __name__ == "__main__":
    main()
