"""Cases for the evaluation stage's mesh distance: one hand-checked triangle, the CPU meshes of
tests/surface_fixture.py with seeded queries, and the edges of the contract.  Every reference
result is computed once by tests/eval_ref.py, cached and read-only.
"""
import collections
import functools

import numpy as np

import eval_ref
import surface_fixture

EPS = float(np.finfo(np.float64).eps)
SCAN_CHUNK = 4096            # cells one workgroup of the scan takes (eval.hip, kEvalScanChunk)

Case = collections.namedtuple("Case", "vertices faces queries cell max_dist")


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- one scalene triangle, the answers written down by hand -----------------------------------
TRIANGLE = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [1.0, 3.0, 0.0]])
# (query, closest point, squared distance, what it checks); all exact in fp64
HAND = (
    ((-1.0, -1.0, 0.0), (0.0, 0.0, 0.0), 2.0, "vertex a, in the plane"),
    ((-1.0, -1.0, 2.0), (0.0, 0.0, 0.0), 6.0, "vertex a, above"),
    ((6.0, -1.0, 0.0), (4.0, 0.0, 0.0), 5.0, "vertex b"),
    ((6.0, -1.0, -3.0), (4.0, 0.0, 0.0), 14.0, "vertex b, below"),
    ((1.0, 5.0, 1.0), (1.0, 3.0, 0.0), 5.0, "vertex c, above"),
    ((2.0, -2.0, 0.0), (2.0, 0.0, 0.0), 4.0, "edge ab"),
    ((2.0, -2.0, -1.0), (2.0, 0.0, 0.0), 5.0, "edge ab, below"),
    ((-2.5, 2.5, 0.0), (0.5, 1.5, 0.0), 10.0, "edge ac"),
    ((-2.5, 2.5, 1.0), (0.5, 1.5, 0.0), 11.0, "edge ac, above"),
    ((3.5, 2.5, 2.0), (2.5, 1.5, 0.0), 6.0, "edge bc, above"),
    ((3.5, 2.5, 0.0), (2.5, 1.5, 0.0), 2.0, "edge bc, in the plane"),
    ((1.75, 1.5, 3.0), (1.75, 1.5, 0.0), 9.0, "interior, above"),
    ((1.75, 1.5, -3.0), (1.75, 1.5, 0.0), 9.0, "interior, below"),
    ((1.75, 1.5, 0.0), (1.75, 1.5, 0.0), 0.0, "on the triangle"),
    ((2.0, 0.0, 0.0), (2.0, 0.0, 0.0), 0.0, "on edge ab"),
    ((4.0, 0.0, 0.0), (4.0, 0.0, 0.0), 0.0, "at vertex b"),
)


def box_of(vertices, faces):
    """(lo, hi) of the faces with finite coordinates."""
    tri = np.asarray(vertices)[np.asarray(faces).reshape(-1, 3)]
    tri = tri[np.isfinite(tri).all(axis=(1, 2))]
    return tri.min(axis=(0, 1)), tri.max(axis=(0, 1))


def diagonal(case):
    lo, hi = box_of(case.vertices, case.faces)
    return float(np.sqrt(((hi - lo) ** 2).sum()))


def _mesh_queries(v, f, seed, voxel):
    """The mesh's own vertices, the vertices displaced by a seeded 0.3-voxel noise, and 500 seeded
    uniform points in the box grown by 50 % (inside and outside the grid)."""
    rs = np.random.RandomState(seed)
    lo, hi = box_of(v, f)
    mid, half = (lo + hi) / 2.0, (hi - lo) / 2.0
    noisy = v + 0.3 * voxel * rs.standard_normal(v.shape)
    uniform = mid + 1.5 * half * rs.uniform(-1.0, 1.0, (500, 3))
    return np.concatenate((v, noisy, uniform))


def _edge_queries(v, f, cell):
    """Exactly on the box, on cell boundaries of this `cell`, and 100 box widths away."""
    lo, hi = box_of(v, f)
    rs = np.random.RandomState(5)
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1])
                        for z in (lo[2], hi[2])])
    on_face = lo + (hi - lo) * rs.uniform(0.0, 1.0, (12, 3))
    for j in range(12):
        on_face[j, j % 3] = (lo if j % 2 else hi)[j % 3]
    dims = np.floor((hi - lo) / cell).astype(int) + 1
    k = np.stack([rs.randint(0, d + 1, 40) for d in dims], axis=1)
    boundary = lo + k * cell                       # all three coordinates on a boundary
    one_axis = lo + (hi - lo) * rs.uniform(0.0, 1.0, (40, 3))
    one_axis[:, 0] = lo[0] + k[:, 0] * cell        # the x coordinate only
    width = (hi - lo).max()
    far = np.array([[lo[0] - 100.0 * width, (lo[1] + hi[1]) / 2, (lo[2] + hi[2]) / 2],
                    [hi[0] + 100.0 * width, hi[1] + 100.0 * width, hi[2] + 100.0 * width],
                    [(lo[0] + hi[0]) / 2, lo[1] - 100.0 * width, hi[2] + 3.0 * width]])
    return np.concatenate((corners, on_face, boundary, one_axis, far))


EDGE_CELL = 1.0
RANDOM_CELL = 0.25           # 21 x 19 x 17 cells: past one scan chunk
HALF_MAX_DIST = 1.5


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case."""
    out = {}
    tri_f = np.array([[0, 1, 2]], dtype=np.int32)
    out["one_triangle"] = Case(TRIANGLE, tri_f, np.array([h[0] for h in HAND]), None, np.inf)

    v, f = surface_fixture.reference_extract("s12")
    q12 = _mesh_queries(v, f, 31, 1.0)
    out["s12"] = Case(v, f, q12, None, np.inf)
    rv, rf = surface_fixture.reference_extract("random")
    out["random"] = Case(rv, rf, _mesh_queries(rv, rf, 32, 0.5), RANDOM_CELL, np.inf)

    # s12 and one triangle that spans its whole box: a face registered in every cell
    lo, hi = box_of(v, f)
    big = np.array([lo, [hi[0], hi[1], lo[2]], [lo[0], hi[1], hi[2]]])
    bv = np.concatenate((v, big))
    bf = np.concatenate((f, [[len(v), len(v) + 1, len(v) + 2]])).astype(np.int32)
    out["big_and_small"] = Case(bv, bf, q12[-700:], None, np.inf)

    out["edges"] = Case(v, f, _edge_queries(v, f, EDGE_CELL), EDGE_CELL, np.inf)
    out["half"] = Case(v, f, q12[-500:], None, HALF_MAX_DIST)

    # invalid faces among valid ones, and queries that are not finite
    dv = np.concatenate((TRIANGLE, [[0.0, 0.0, 1.0], [1.0, 1.0, 2.0], [2.0, 2.0, 3.0],
                                    [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [5.0, 5.0, 5.0],
                                    [6.0, 5.0, 5.0], [5.0, 6.0, 7.0]]))
    df = np.array([[3, 4, 5],      # no area: three points on a line
                   [0, 1, 2],
                   [0, 0, 1],      # a repeated index
                   [0, 1, 6],      # a NaN vertex
                   [8, 9, 10],
                   [1, 7, 2],      # an infinite vertex
                   [2, 1, 0]],     # face 1 again, the other way round: a tie in d2
                  dtype=np.int32)
    dq = np.concatenate((np.array([h[0] for h in HAND]),
                         [[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [1.0, 1.0, -np.inf],
                          [5.2, 5.3, 5.9], [100.0, -50.0, 3.0]]))
    out["degenerate"] = Case(dv, df, dq, None, np.inf)
    for c in out.values():
        _freeze(c.vertices, c.faces, c.queries)
    return out


CASE_NAMES = ("one_triangle", "s12", "random", "big_and_small", "edges", "half", "degenerate")
DEGENERATE_SKIPPED = 4
QUERY_COUNTS = (255, 256, 257)   # of s12's queries: around one workgroup


@functools.lru_cache(maxsize=None)
def reference(name):
    """(d2, face, closest, pairs) of the fp64 restatement; pairs is (n, nf)."""
    c = cases()[name]
    return _freeze(*eval_ref.mesh_distance(c.queries, c.vertices, c.faces, c.max_dist,
                                           return_pairs=True))


# The worst |d2 - d2_longdouble| / L^2 of the fp64 restatement against its own longdouble run,
# L the case's box diagonal, as tests/test_eval_cpu.py measures and asserts it.  The GPU's bar is
# 4 x this, floored at 16 eps.
MEASURED = {                  # the run's own figure, rounded up
    "one_triangle": 0.0,      # 0: every answer is exact
    "s12": 4.5e-17,           # 4.485e-17
    "random": 1.6e-17,        # 1.587e-17
    "big_and_small": 4.5e-17,  # 4.485e-17
    "edges": 1.4e-12,         # 1.312e-12: the queries 100 box widths away, d2 = 1e4 L^2
    "half": 1.4e-17,          # 1.304e-17
    "degenerate": 1e-21,      # 4.9e-22
}


def bar(name):
    return max(4.0 * MEASURED[name], 16.0 * EPS)
