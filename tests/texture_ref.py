"""The definitions of rs_surface_render_depth and rs_surface_colorize (include/rsamd.h) restated
in numpy: plain loops over views, faces and vertices, fp64, no vectorisation across faces.  The
oracle of tests/test_gpu_texture.py; tests/test_texture_cpu.py tests it alone.

Both functions take P = K C as the public functions build it and turn the cameras themselves.
``margins`` (a dict) receives the smallest distances to every decision that a last-bit difference
could flip:
  b        |b_k| over all evaluated (face, pixel) pairs
  inside   the distance of a vertex's u, v to 0, w - 1, h - 1 (vertices in front)
  visible  |z - far (1 + rel_tol)| / (far (1 + rel_tol))
  cos      |g - min_cos|
"""
import numpy as np


def turn(P):
    """(s_v P_v, c_v): the cameras with positive depths in front, and their centres."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3, 4)
    out, centres = np.empty_like(P), np.empty((len(P), 3))
    for v, p in enumerate(P):
        M = p[:, :3]
        det = M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) \
            - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0]) \
            + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0])
        if not np.all(np.isfinite(p)) or not np.isfinite(det) or det == 0.0:
            raise ValueError("a camera is not finite or singular")
        out[v] = -p if det < 0.0 else p
        centres[v] = -np.linalg.solve(out[v][:, :3], out[v][:, 3])
    return out, centres


def _note(margins, key, value):
    if margins is not None:
        margins[key] = min(margins.get(key, np.inf), float(value))


def project(Pv, X):
    """q = P_v [X; 1] for rows of X, summed left to right as the kernels do."""
    X = np.atleast_2d(X)
    return np.stack([Pv[r, 0] * X[:, 0] + Pv[r, 1] * X[:, 1] + Pv[r, 2] * X[:, 2] + Pv[r, 3]
                     for r in range(3)], axis=1)


def render_depth(vertices, faces, P, shape, margins=None):
    """(V, h, w) float32 z-buffers, NaN where no face covers the pixel."""
    vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    h, w = shape
    Ps, _ = turn(P)
    zbuf = np.full((len(Ps), h, w), np.inf, np.float32)
    with np.errstate(all="ignore"):
        for v, Pv in enumerate(Ps):
            qall = project(Pv, vertices) if len(vertices) else np.zeros((0, 3))
            for f in faces:
                q = qall[f]
                if not np.all(np.isfinite(q)) or not np.all(q[:, 2] > 0.0):
                    continue                      # crosses the camera plane: skipped, not clipped
                z = q[:, 2]
                x, y = q[:, 0] / z, q[:, 1] / z
                A = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
                if not np.isfinite(A) or A == 0.0:
                    continue
                lox, hix = max(np.ceil(x.min()), 0.0), min(np.floor(x.max()), w - 1.0)
                loy, hiy = max(np.ceil(y.min()), 0.0), min(np.floor(y.max()), h - 1.0)
                if not (lox <= hix and loy <= hiy):
                    continue
                py, px = np.mgrid[int(loy):int(hiy) + 1, int(lox):int(hix) + 1].astype(np.float64)
                b0 = ((x[2] - x[1]) * (py - y[1]) - (y[2] - y[1]) * (px - x[1])) / A
                b1 = ((x[0] - x[2]) * (py - y[2]) - (y[0] - y[2]) * (px - x[2])) / A
                b2 = ((x[1] - x[0]) * (py - y[0]) - (y[1] - y[0]) * (px - x[0])) / A
                _note(margins, "b", min(np.abs(b0).min(), np.abs(b1).min(), np.abs(b2).min()))
                cover = (b0 >= 0.0) & (b1 >= 0.0) & (b2 >= 0.0)
                zeta = (1.0 / (b0 / z[0] + b1 / z[1] + b2 / z[2])).astype(np.float32)
                win = zbuf[v, int(loy):int(hiy) + 1, int(lox):int(hix) + 1]
                win[cover] = np.minimum(win[cover], zeta[cover])
    zbuf[np.isinf(zbuf)] = np.nan
    return zbuf


def box_pixels(vertices, face, P, shape):
    """The number of pixels in the clipped bounding box of one face in view 0 (0: not drawn)."""
    h, w = shape
    q = project(turn(P)[0][0], np.asarray(vertices, dtype=np.float64)[np.asarray(face)])
    if not np.all(np.isfinite(q)) or not np.all(q[:, 2] > 0.0):
        return 0
    x, y = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
    lox, hix = max(np.ceil(x.min()), 0.0), min(np.floor(x.max()), w - 1.0)
    loy, hiy = max(np.ceil(y.min()), 0.0), min(np.floor(y.max()), h - 1.0)
    return int(max(hix - lox + 1, 0) * max(hiy - loy + 1, 0))


def vertex_colors(vertices, faces, images, P, normals=None, rel_tol=0.01, min_cos=0.0,
                  depth=None, margins=None, detail=None):
    """(colors (Nv, ch) float64, count (Nv,) int32, depth).  ``depth``: z-buffers to use in
    place of this module's own.  ``detail`` (a dict) receives u, v and g, each (Nv, V), NaN
    where the view did not contribute."""
    vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    images = np.asarray(images)
    V, h, w = images.shape[:3]
    img = images.reshape(V, h, w, -1).astype(np.float64)
    ch = img.shape[3]
    Ps, centres = turn(P)
    if depth is None:
        depth = render_depth(vertices, faces, P, (h, w), margins)
    nv = len(vertices)
    colors, count = np.zeros((nv, ch)), np.zeros(nv, np.int32)
    keep = {k: np.full((nv, V), np.nan) for k in ("u", "v", "g")}
    with np.errstate(all="ignore"):
        for i, X in enumerate(vertices):
            acc, wsum = np.zeros(ch), 0.0
            for v, Pv in enumerate(Ps):
                q = project(Pv, X)[0]
                z = q[2]
                if not (np.all(np.isfinite(q)) and z > 0.0):
                    continue
                u, r = q[0] / z, q[1] / z
                _note(margins, "inside", min(abs(u), abs(u - (w - 1)), abs(r), abs(r - (h - 1))))
                if not (0.0 <= u <= w - 1 and 0.0 <= r <= h - 1):
                    continue
                x0, y0 = int(np.floor(u)), int(np.floor(r))
                x1, y1 = min(x0 + 1, w - 1), min(y0 + 1, h - 1)
                foot = np.array([depth[v, y0, x0], depth[v, y0, x1], depth[v, y1, x0],
                                 depth[v, y1, x1]], dtype=np.float64)
                foot = foot[np.isfinite(foot)]
                if not len(foot):
                    continue
                limit = foot.max() * (1.0 + rel_tol)
                _note(margins, "visible", abs(z - limit) / limit)
                if not z <= limit:
                    continue
                g = 1.0
                if normals is not None:
                    d = centres[v] - X
                    g = (normals[i, 0] * d[0] + normals[i, 1] * d[1] + normals[i, 2] * d[2]) / \
                        np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
                    _note(margins, "cos", abs(g - min_cos))
                    if not g > min_cos:
                        continue
                fx, fy = u - x0, r - y0
                top = img[v, y0, x0] + fx * (img[v, y0, x1] - img[v, y0, x0])
                bot = img[v, y1, x0] + fx * (img[v, y1, x1] - img[v, y1, x0])
                acc += g * (top + fy * (bot - top))
                wsum += g
                count[i] += 1
                keep["u"][i, v], keep["v"][i, v], keep["g"][i, v] = u, r, g
            if count[i]:
                colors[i] = acc / (255.0 * wsum)
    if detail is not None:
        detail.update(keep)
    return colors, count, depth
