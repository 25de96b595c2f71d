"""Generate tests/golden/features.npz -- the image front end -- from the reference.

Runs ONLY in the build container (imports the reference as make_golden.py does, with the
import-only cv2 stub).  For a few tiny inputs it records the outputs of

  * lab3.non_max_suppression (lab3.py:160-185), windows 1, 3 and 5, on a random float32 image
    and on one with plateaus;
  * lab3.cut_out_rois (lab3.py:565-602), and which message each bad index raises (the four
    texts of lab3.py:592-599 in their precedence, and the even-size text of lab3.py:586);
  * fun.matchingMatrix (fun.py:113-120) for float64 ROIs and for uint8 ROIs (whose
    subtraction wraps modulo 256);
  * lab3.joint_min (lab3.py:529-563), including a matrix with tied minima.

lab3.harris cannot be recorded: cv2.cornerHarris is the stub (OpenCV is not installed), so the
Harris step is pinned by its documented definition and closed forms instead.

Usage:  python tests/golden/make_golden_features.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, _save  # noqa: E402


def _message(fn, *args):
    try:
        fn(*args)
    except ValueError as e:
        return str(e)
    return ""


def main():
    lab3, fun, _, _ = import_reference()
    rs = np.random.RandomState(7)
    out = {}

    rnd = rs.rand(13, 17).astype(np.float32)
    plat = np.round(rs.rand(12, 15) * 4).astype(np.float32)    # few levels: equal neighbours
    plat[3:6, 4:8] = 9.0
    out["nms_in_rnd"], out["nms_in_plat"] = rnd, plat
    for name, img in (("rnd", rnd), ("plat", plat)):
        for win in (1, 3, 5):
            out[f"nms_{name}_w{win}"] = lab3.non_max_suppression(img, win)

    img = rs.randint(0, 256, size=(11, 14)).astype(np.uint8)
    cols, rows = np.array([2, 11, 5, 2, 7]), np.array([2, 8, 5, 8, 2])
    out["roi_img"], out["roi_cols"], out["roi_rows"] = img, cols, rows
    out["roi_out"] = np.stack(lab3.cut_out_rois(img, cols, rows, 5))
    # (cols, rows, roi_size) of the bad calls; rows high beats rows low beats cols high ...
    bad = {"row_high": ([5], [9], 5), "row_low": ([5], [1], 5), "col_high": ([12], [5], 5),
           "col_low": ([1], [5], 5), "row_high_first": ([1, 12], [1, 9], 5),
           "row_low_first": ([1, 12], [1, 5], 5), "col_high_first": ([1, 12], [5, 5], 5),
           "even": ([5], [5], 4)}
    out["roi_bad_names"] = np.array(sorted(bad))
    for name, (c, r, size) in bad.items():
        out[f"roi_bad_{name}_args"] = np.array([c, r, [size] * len(c)])
        out[f"roi_bad_{name}_msg"] = np.array(_message(lab3.cut_out_rois, img, c, r, size))

    f1, f2 = rs.randn(5, 7, 7) * 50.0, rs.randn(6, 7, 7) * 50.0
    f2[2] = f1[3]
    out["mm_f64_r1"], out["mm_f64_r2"] = f1, f2
    out["mm_f64"] = fun.matchingMatrix(list(f1), list(f2))
    u1 = rs.randint(0, 256, size=(6, 3, 3)).astype(np.uint8)
    u2 = rs.randint(0, 256, size=(4, 3, 3)).astype(np.uint8)
    u2[1] = u1[4]
    out["mm_u8_r1"], out["mm_u8_r2"] = u1, u2
    out["mm_u8"] = fun.matchingMatrix(list(u1), list(u2))

    A = rs.rand(7, 9)
    T = np.round(rs.rand(6, 8) * 3)                            # many ties
    for name, mat in (("rnd", A), ("tie", T), ("mm", out["mm_f64"])):
        vals, ri, ci = lab3.joint_min(mat)
        out[f"jm_{name}_in"] = mat
        out[f"jm_{name}_vals"], out[f"jm_{name}_ri"], out[f"jm_{name}_ci"] = \
            np.asarray(vals, np.float64), np.asarray(ri, np.int64), np.asarray(ci, np.int64)
    _save("features.npz", **out)


if __name__ == "__main__":
    main()
