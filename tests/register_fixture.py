"""Cases for the registration step and loop: the "blob", an asymmetric closed mesh with a source
cloud moved off it by a known similarity, and small hand-placed clouds over the one triangle of
tests/eval_fixture.py that put the trimmed selection and the moments' blocks on their edges.  The
restatement (tests/register_ref.py) runs once per case, cached and read-only.
"""
import functools

import numpy as np

import eval_fixture
import register_ref as ref

EPS = float(np.finfo(np.float64).eps)
BLOCK = ref.BLOCK
METRICS = ("point", "plane")
COMPARE_ITERATIONS = 8      # of a loop that a GPU test compares with the restatement's


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def rotation(axis, degrees):
    axis = np.asarray(axis, dtype=np.float64)
    return ref.rodrigues(np.radians(degrees) * axis / np.sqrt((axis * axis).sum()))


# ---- the blob -----------------------------------------------------------------------------------
BLOB_DIVISIONS = (20, 40)
TRUTH = (1.04, rotation((1.0, 2.0, 3.0), 8.0), np.array([0.4, -0.3, 0.5]))
SAMPLES, OUTLIERS, NOISE_SIGMA = 1200, 300, 0.02


def _blob_point(th, ph):
    r = (1.0 + 0.25 * np.sin(th) ** 2 * np.cos(2.0 * ph + 0.4)
         + 0.2 * np.cos(th) * np.sin(th) * np.sin(ph) + 0.15 * np.sin(th) ** 3 * np.cos(3.0 * ph))
    x = r * np.sin(th) * np.cos(ph)
    y = 0.8 * r * np.sin(th) * np.sin(ph)
    z = 0.6 * r * np.cos(th) + 0.1 * r * np.sin(th) * np.cos(ph)
    return 5.0 * np.stack([x, y, z], axis=-1) + np.array([3.0, -2.0, 7.0])


@functools.lru_cache(maxsize=None)
def blob():
    """(vertices (762, 3), faces (1520, 3) int32): a latitude / longitude mesh, the poles first."""
    nt, nph = BLOB_DIVISIONS
    th = np.pi * np.arange(1, nt) / nt
    ph = 2.0 * np.pi * np.arange(nph) / nph
    ring = _blob_point(th[:, None], ph[None, :]).reshape(-1, 3)
    v = np.concatenate((_blob_point(np.array(0.0), np.array(0.0))[None],
                        _blob_point(np.array(np.pi), np.array(0.0))[None], ring))
    at = lambda i, j: 2 + i * nph + j % nph          # noqa: E731
    f = []
    for j in range(nph):
        f.append((0, at(0, j), at(0, j + 1)))
        f.append((1, at(nt - 2, j + 1), at(nt - 2, j)))
        for i in range(nt - 2):
            f.append((at(i, j), at(i + 1, j), at(i + 1, j + 1)))
            f.append((at(i, j), at(i + 1, j + 1), at(i, j + 1)))
    return _freeze(v, np.array(f, dtype=np.int32))


def back(points):
    """The points the truth maps onto ``points``: R^T (p - t) / s."""
    s, R, t = TRUTH
    return (np.asarray(points) - t) @ R / s


@functools.lru_cache(maxsize=None)
def clouds():
    """name -> (source points, keep): ``clean`` 1 200 surface samples moved back through the
    truth, ``outlier`` those and 300 uniform points of the box grown by 25 %, ``noisy`` the
    samples with sigma = 0.02 of normal noise."""
    from tsbb15_amd import evaluation as ev
    v, f = blob()
    on = ev.sample_surface(v, f, SAMPLES, seed=7)[0]
    lo, hi = v.min(axis=0), v.max(axis=0)
    mid, half = (lo + hi) / 2.0, (hi - lo) / 2.0
    out = mid + 1.25 * half * np.random.RandomState(11).uniform(-1.0, 1.0, (OUTLIERS, 3))
    noise = NOISE_SIGMA * np.random.RandomState(13).standard_normal(on.shape)
    res = {"clean": (back(on), 1.0), "outlier": (back(np.concatenate((on, out))), 0.75),
           "noisy": (back(on + noise), 1.0)}
    for p, _ in res.values():
        _freeze(p)
    return res


CLOUD_NAMES = ("clean", "outlier", "noisy")


def blob_diagonal():
    return ref.mesh_box(*blob())[1]


def trace_iterations(name, metric):
    """The steps a loop is compared over: 8, and 4 where the slow point metric runs on the clouds
    no CPU test needs a longer trace of (the restatement takes a second a step)."""
    return 4 if metric == "point" and name != "clean" else COMPARE_ITERATIONS


@functools.lru_cache(maxsize=None)
def blob_trace(name, metric):
    """The restatement's loop on a cloud of the blob, at most trace_iterations steps."""
    v, f = blob()
    pts, keep = clouds()[name]
    return ref.register(pts, v, f, metric=metric, keep=keep,
                        max_iter=trace_iterations(name, metric))


@functools.lru_cache(maxsize=None)
def blob_step(name, metric, dtype=np.float64):
    """The restatement's first step (the identity, 8 degrees from the truth)."""
    v, f = blob()
    pts, keep = clouds()[name]
    return ref.step(pts, v, f, 1.0, np.eye(3), np.zeros(3), ref.mesh_box(v, f)[0], keep,
                    np.inf, metric, dtype)


# ---- small cases over one triangle ------------------------------------------------------------
TRIANGLE = eval_fixture.TRIANGLE
TRI_FACES = np.array([[0, 1, 2]], dtype=np.int32)
IDENTITY = (1.0, np.eye(3), np.zeros(3))
MOVE = (1.1, rotation((2.0, -1.0, 0.5), 5.0), np.array([0.2, -0.1, 0.3]))
ABOVE = (1.75, 1.5)            # over the interior: d2 = z^2 exactly


def _above(zs):
    zs = np.asarray(zs, dtype=np.float64)
    return np.stack([np.full(len(zs), ABOVE[0]), np.full(len(zs), ABOVE[1]), zs], axis=1)


def _random(n, seed):
    rs = np.random.RandomState(seed)
    return np.array([1.5, 1.0, 0.0]) + np.array([4.0, 3.0, 2.0]) * rs.uniform(-1.0, 1.0, (n, 3))


@functools.lru_cache(maxsize=None)
def small_cases():
    """name -> dict(points, T, keep, max_dist) against TRIANGLE."""
    one = 1.0
    steps = [one]
    for _ in range(4):
        steps.append(np.nextafter(steps[-1], 2.0))
    # 1 + 2^-b squares to 1 + 2^(1 - b) (+ 2^(-2 b)): the keys leave the prefix of 1.0 at byte
    # 6, 5, 4, 3, 2, 1, 0 in turn, and three more binades make the top byte decide as well
    spread = [2.0 ** -10, 2.0 ** -3, 32.0, 1.0] + [1.0 + 2.0 ** -b for b in (3, 9, 17, 25, 33, 41, 49)]
    c = {
        "ties": dict(points=_above([0.5, 1.0, 1.0, 2.0, 3.0]), keep=0.4),          # k 2, kept 3
        "neighbours": dict(points=_above(steps), keep=0.6),                         # k 3
        "binades": dict(points=_above(spread), keep=4.0 / 11.0),                    # k 4
        "on_face": dict(points=np.array([[1.75, 1.5, 0.0], [2.0, 0.0, 0.0], [4.0, 0.0, 0.0],
                                         [1.75, 1.5, 1.0], [1.0, 1.0, -2.0]]), keep=0.4),
        "unmatched": dict(points=np.concatenate((_above([0.5, 1.5, 2.5, 10.0]),
                                                 [[np.nan, 0.0, 1.0], [1.0, np.inf, 1.0]])),
                          keep=1.0, max_dist=5.0),
        "k_one": dict(points=_random(40, 1), keep=1e-6),
        "k_all": dict(points=_random(40, 2), keep=1.0),
        "seven_of_ten": dict(points=_random(10, 3), keep=0.7),
        "seven_of_hundred": dict(points=_random(100, 5), keep=0.07),   # 0.07 x 100 > 7 in fp64
        "none": dict(points=_above([0.5, 1.0, 2.0]), keep=1.0, max_dist=1e-3),
    }
    for n in (255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1):
        c[f"count_{n}"] = dict(points=_random(n, n), keep=0.75, T=MOVE, max_dist=6.0)
    for case in c.values():
        case.setdefault("T", IDENTITY)
        case.setdefault("max_dist", np.inf)
        _freeze(case["points"])
    return c


SMALL_NAMES = ("ties", "neighbours", "binades", "on_face", "unmatched", "k_one", "k_all",
               "seven_of_ten", "seven_of_hundred", "none", "count_255", "count_256", "count_257",
               f"count_{BLOCK - 1}", f"count_{BLOCK}", f"count_{BLOCK + 1}",
               f"count_{2 * BLOCK + 1}")
# (matched, k, kept) the hand-placed cases are built to give
EXPECTED = {"ties": (5, 2, 3), "neighbours": (5, 3, 3), "binades": (11, 4, 4),
            "on_face": (5, 2, 3), "unmatched": (3, 3, 3), "k_one": (40, 1, 1),
            "k_all": (40, 40, 40), "seven_of_ten": (10, 7, 7),
            "seven_of_hundred": (100, 7, 7), "none": (0, 0, 0)}


@functools.lru_cache(maxsize=None)
def small_step(name, metric, dtype=np.float64):
    case = small_cases()[name]
    s, R, t = case["T"]
    return ref.step(case["points"], TRIANGLE, TRI_FACES, s, R, t,
                    ref.mesh_box(TRIANGLE, TRI_FACES)[0], case["keep"], case["max_dist"], metric,
                    dtype)


# ---- bars -------------------------------------------------------------------------------------
def deviation(got, want, scale):
    """The worst |got - want| over the slots, each relative to the sum of its terms' magnitudes;
    slots without a term must agree exactly."""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    diff = np.abs(got - want).astype(np.float64)
    if (diff[scale == 0.0] != 0.0).any():
        return np.inf
    used = scale > 0.0
    return float((diff[used] / scale[used]).max()) if used.any() else 0.0


# The worst deviation of the fp64 moments from the restatement's own longdouble run, per slot
# relative to the sum of the terms' magnitudes, as tests/test_register_cpu.py measures and asserts
# it, over the small cases and the blob's first steps.  The GPU's bar is 4 x this, floored at
# 16 eps.
MEASURED = {                  # the run's own figure, rounded up
    "point": 1.9e-16,         # 1.808e-16, k_one
    "plane": 2.5e-16,         # 2.432e-16, count_2048
}


def bar(metric):
    return max(4.0 * MEASURED[metric], 16.0 * EPS)
