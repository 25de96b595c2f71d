"""The host-side parts of tsbb15_amd.dense that need no GPU: refine_depth, depth_points,
plane_warps and table_views against tests/dense_ref.py, and the argument checks, which raise
before the library is touched."""
import types

import numpy as np
import pytest

import dense_fixture as df
import dense_ref as dr
from tsbb15_amd import dense


def test_refine_depth_and_points_match_the_restatement():
    index, delta, *_ = df.reference_sweeps()["slanted_p7"]
    got = dense.refine_depth(index, delta, df.DEPTHS)
    want = dr.refine_depth(index, delta, df.DEPTHS)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[index < 0]).all() and (index < 0).any()
    neg = dense.refine_depth(index, delta, -df.DEPTHS)
    assert np.array_equal(neg, -got, equal_nan=True)
    cams = df.cameras()
    pts = dense.depth_points(got, cams[2], df.K)
    assert pts.shape == index.shape + (3,)
    assert np.allclose(pts, dr.depth_points(want, cams[2], df.K), rtol=0, atol=1e-12,
                       equal_nan=True)
    # a point of depth d in view 2 has cams[2][2] . [X; 1] = d
    ok = np.isfinite(got)
    assert np.allclose(pts[ok] @ cams[2][2, :3] + cams[2][2, 3], got[ok], rtol=1e-12)


def test_plane_warps_match_and_map_the_plane():
    cams = df.cameras()
    A, b = dense.plane_warps(cams[0], cams[1:], df.K)
    rA, rb = dr.plane_warps(cams[0], cams[1:], df.K)
    assert np.array_equal(A, rA) and np.array_equal(b, rb)
    # a pixel of the fronto-parallel plane z = 4 lands where the source camera sees its point
    p = np.array([30.0, 11.0, 1.0])
    X = 4.0 * np.linalg.inv(df.K) @ p
    q = df.K @ (cams[1] @ np.append(X, 1.0))
    assert np.allclose(4.0 * A[0] @ p + b[0], q, rtol=1e-12)


def test_table_views():
    pose = types.SimpleNamespace(R=np.eye(3), t=np.array([1.0, 2.0, 3.0]))
    T = types.SimpleNamespace(T_views=[types.SimpleNamespace(image=4, camera_pose=pose),
                                       types.SimpleNamespace(image=7, camera_pose=df.cameras()[1])])
    index, cams = dense.table_views(T)
    assert index == [4, 7] and cams.shape == (2, 3, 4)
    assert np.array_equal(cams[0], np.hstack((np.eye(3), [[1.0], [2.0], [3.0]])))
    assert np.array_equal(cams[1], df.cameras()[1])


def test_argument_checks_need_no_gpu():
    ref, rc, srcs, sc, K, depths, patch = df.sweep_cases()["fronto_p5"]
    for kw in (dict(patch=4), dict(patch=13), dict(min_var=0.0), dict(depths=depths * np.tile((1.0, -1.0), 6)),
               dict(depths=[0.0, 1.0]), dict(K=np.eye(3) * 2.0), dict(src_images=[srcs[0]])):
        a = dict(ref_image=ref, ref_cam=rc, src_images=srcs, src_cams=sc, K=K, depths=depths,
                 patch=patch)
        a.update(kw)
        with pytest.raises(ValueError):
            dense.plane_sweep(**a)
    big = np.zeros((8193, 8193), np.uint8)          # h w > 2^26 with both sides allowed
    with pytest.raises(ValueError, match="2\\^26"):
        dense.plane_sweep(big, rc, [big, big], sc, K, depths, patch=patch)
    with pytest.raises(ValueError):
        dense.consistency(np.zeros((2, 4, 4)), df.cameras(), df.K)
