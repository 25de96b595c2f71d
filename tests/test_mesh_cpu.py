"""The mesh clean-up's numpy restatement (tests/mesh_ref.py) on its own, and the host policy of
``surface.remove_small`` with the restatement in the kernels' place.  No GPU.

Figures measured with the restatement are printed before they are asserted.
"""
import numpy as np
import pytest

import mesh_fixture as mfx
import mesh_ref as ref
import surface_fixture as sfx
import surface_ref
from tsbb15_amd import surface


def _component_sizes(label, size):
    roots = np.flatnonzero(label == np.arange(len(label)))
    return sorted((int(size[r]) for r in roots), reverse=True)


def _remove_small(vertices, faces, **kw):
    """surface.remove_small with the restatement injected for both kernels."""
    label, size, _ = ref.components(faces, len(vertices))
    keep = surface._keep_components(label, size, len(faces), kw.get("min_faces"),
                                    kw.get("keep_largest"), kw.get("min_fraction"))
    assert np.array_equal(keep, ref.keep_components(label, size, len(faces), **kw))
    return ref.compact(vertices, faces, keep)


def test_random_fixture_components():
    v, f = mfx.random_mesh()
    label, size, count = ref.components(f, len(v))
    sizes = _component_sizes(label, size)
    print(f"random fixture: {len(f)} faces, {count} components, sizes {sizes}")
    assert len(f) == 2362 and count == 17
    assert sizes[0] == 2154 and sizes[1] == 72 and min(sizes) > 0
    assert sum(sizes) == len(f)
    assert np.all(label <= np.arange(len(v))) and np.array_equal(label[label], label)


def test_small_meshes_by_hand():
    m = mfx.small_meshes()
    label, size, count = ref.components(*m["no_face"])
    assert label.tolist() == [0, 1, 2, 3, 4] and size.tolist() == [0] * 5 and count == 5
    label, size, count = ref.components(*m["shared_vertex"])
    assert label.tolist() == [0] * 5 and size.tolist() == [2] * 5 and count == 1
    label, size, count = ref.components(*m["disjoint"])
    assert label.tolist() == [0, 0, 0, 3, 3, 3] and size.tolist() == [1] * 6 and count == 2
    label, size, count = ref.components(*m["repeated_index"])
    assert label.tolist() == [0, 1, 0, 1, 4] and size.tolist() == [1, 1, 1, 1, 1] and count == 3
    label, size, count = ref.components(*m["unreferenced_middle"])
    assert label.tolist() == [0, 0, 2, 3, 0, 0, 0, 7, 7, 7] and count == 4
    assert size.tolist() == [2, 2, 0, 0, 2, 2, 2, 1, 1, 1]


@pytest.mark.parametrize("order", mfx.ORDERS)
def test_chain_is_one_component(order):
    v, f = mfx.chain(257, order, seed=1)
    label, size, count = ref.components(f, len(v))
    assert count == 1 and np.all(label == 0) and np.all(size == 257)


def test_two_spheres_remove_small():
    v, f = mfx.two_sphere_mesh()
    label, size, count = ref.components(f, len(v))
    sizes = _component_sizes(label, size)
    print(f"two spheres: {len(v)} vertices, {len(f)} faces, components {sizes}")
    assert (len(v), len(f)) == (2724, 5440) and count == 2 and sizes == [5124, 316]
    assert surface_ref.is_closed(f)
    results = [_remove_small(v, f, min_faces=1000), _remove_small(v, f, keep_largest=1),
               _remove_small(v, f, min_fraction=0.5)]
    for v2, f2, vmap in results:
        assert (len(v2), len(f2)) == (2564, 5124)
        assert surface_ref.is_closed(f2) and surface_ref.euler(v2, f2) == 2
        assert np.array_equal(v2, v[vmap >= 0]) and int((vmap >= 0).sum()) == 2564
        assert all(np.array_equal(a, b) for a, b in zip((v2, f2, vmap), results[0]))
    # the floater alone: the criteria are combined with "and"
    v3, f3, _ = _remove_small(v, f, keep_largest=2, min_faces=0)
    assert len(f3) == len(f) and len(v3) == len(v)


def test_policy_ties_and_unreferenced():
    f, n = mfx.small_meshes()["unreferenced_middle"]
    f = np.concatenate((f, [[2, 3, 2]])).astype(np.int32)   # a second component of one face
    label, size, _ = ref.components(f, n)
    keep = surface._keep_components(label, size, len(f), None, 2, None)
    assert np.array_equal(keep, ref.keep_components(label, size, len(f), keep_largest=2))
    # sizes: root 0 has 2 faces, roots 2 and 7 one each: the tie goes to label 2
    assert keep.tolist() == [True, True, True, True, True, True, True, False, False, False]
    with pytest.raises(ValueError):
        surface._keep_components(label, size, len(f), None, None, None)
    # a vertex in no face is dropped whatever the criterion
    f2, n2 = mfx.small_meshes()["unreferenced_middle"]
    label, size, _ = ref.components(f2, n2)
    keep = surface._keep_components(label, size, len(f2), 0, None, None)
    assert keep.tolist() == [True, True, False, False] + [True] * 6


def test_compact_restatement():
    v, f = mfx.random_mesh()
    keep = np.random.RandomState(8).uniform(size=len(v)) < 0.7
    v2, f2, vmap = ref.compact(v, f, keep)
    assert len(v2) == int(keep.sum()) and np.array_equal(v2, v[keep])
    assert np.array_equal(np.flatnonzero(vmap >= 0), np.flatnonzero(keep))
    kept_faces = f[keep[f].all(axis=1)]
    assert np.array_equal(v2[f2], v[kept_faces])
    same = ref.compact(v, f, np.ones(len(v), bool))
    assert np.array_equal(same[0], v) and np.array_equal(same[1], f)
    assert np.array_equal(same[2], np.arange(len(v)))


def test_smoothing_quality():
    """Taubin removes the noise and keeps the volume; the plain Laplacian shrinks."""
    noisy, f, clean = mfx.noisy_sphere()
    _, c, r = sfx.SPHERES["s16"]
    before = ref.radial_rms(noisy, c, r)
    taubin = ref.smooth(noisy, f, 10, 0.5, -0.53, pin_boundary=False)
    after = ref.radial_rms(taubin, c, r)
    vol_clean = surface_ref.signed_volume(clean, f)
    vol_taubin = surface_ref.signed_volume(taubin, f)
    vol_laplace = surface_ref.signed_volume(ref.smooth(noisy, f, 10, 0.5, 0.5, pin_boundary=False), f)
    print(f"rms radial error {before:.4f} -> {after:.4f}; volume clean {vol_clean:.2f}, "
          f"taubin {vol_taubin:.2f}, lambda|lambda {vol_laplace:.2f}")
    assert after < 0.5 * before
    assert abs(vol_taubin - vol_clean) < 0.01 * abs(vol_clean)
    # the contrast: the shrinking filter fails the bar the Taubin filter has just met, ten times over
    assert abs(vol_clean) - abs(vol_laplace) > 0.10 * abs(vol_clean)


def test_boundary_pinning():
    v, f = mfx.plane_mesh("fronto")
    assert not surface_ref.is_closed(f)
    b = ref.boundary(f, len(v))
    # restated from undirected edge counts: an edge of exactly one face
    e = np.sort(surface_ref.directed_edges(f), axis=1)
    ue, n = np.unique(e, axis=0, return_counts=True)
    want = np.zeros(len(v), bool)
    want[ue[n == 1].reshape(-1)] = True
    assert np.array_equal(b, want) and b.any() and not b.all()
    out = ref.smooth(v, f, 3, pin_boundary=True)
    assert np.array_equal(out[b].view(np.int64), v[b].view(np.int64))
    assert np.any(out[~b] != v[~b])
    free = ref.smooth(v, f, 3, pin_boundary=False)
    assert np.any(free[b] != v[b])


def test_input_bits():
    noisy, f, _ = mfx.noisy_sphere()
    out = ref.smooth(noisy, f, 0)
    assert np.array_equal(out.view(np.int64), np.asarray(noisy).view(np.int64))
    v = np.concatenate((noisy, [[1.5, -0.0, 3.25]]))      # an isolated vertex
    out = ref.smooth(v, f, 4, pin_boundary=False)
    assert np.array_equal(out[-1].view(np.int64), v[-1].view(np.int64))
    assert np.any(out[:-1] != v[:-1])
    fixed = np.zeros(len(v), bool)
    fixed[::3] = True
    out = ref.smooth(v, f, 2, fixed=fixed, pin_boundary=False)
    assert np.array_equal(out[fixed].view(np.int64), v[fixed].view(np.int64))


def test_smooth_sum_order_by_hand():
    """One pass on a fan's hub, the sum formed left to right in ascending order by hand."""
    v, f = mfx.fan(65)
    out = ref.smooth(v, f, 1, 0.5, 0.0, pin_boundary=False)   # the mu pass with factor 0
    s = v[1].copy()
    for u in range(2, 66):
        s = s + v[u]
    want = v[0] + 0.5 * (s / 65.0 - v[0])     # the second pass adds 0 (m - x) = +-0
    assert np.array_equal(out[0], want)
