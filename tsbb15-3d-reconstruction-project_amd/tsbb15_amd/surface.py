"""The surface stage (HIP kernels of surface.hip): depth maps fused into a truncated signed
distance volume, a triangle mesh extracted from it, and the mesh written as PLY.  The reference
project's final artefact is a .ply of vertices without a face, written by an outside tool; it
has no such stage and nothing here restates code of it.

  * ``integrate``       TSDF fusion of V depth maps into a volume (rs_surface_integrate)
  * ``extract``         marching tetrahedra: welded vertices and oriented faces
                        (rs_surface_extract)
  * ``bounds``          origin and dims of a volume that encloses a cloud (host)
  * ``vertex_normals``  area-weighted normals (host)
  * ``save_ply`` / ``load_ply``   binary little-endian PLY (host)
  * ``reconstruct``     ``dense.fuse`` -> ``integrate`` -> ``extract`` (-> ``clean``
                        -> ``simplify`` -> ``vertex_colors``)
  * ``render_depth``    the mesh rendered into a z-buffer per view (rs_surface_render_depth,
                        surface_texture.hip)
  * ``vertex_colors``   a colour per vertex from the views that see it (rs_surface_colorize)
  * ``components``      connected components of an index mesh (rs_mesh_components, mesh.hip)
  * ``compact``         drop vertices and renumber (rs_mesh_compact)
  * ``remove_small``    ``components``, a policy on the host, ``compact``: floaters go
  * ``smooth``          Taubin's lambda|mu smoothing (rs_mesh_smooth)
  * ``clean``           ``remove_small`` -> ``smooth``
  * ``simplify``        vertex clustering on a grid, quadric placement (rs_mesh_simplify,
                        simplify.hip)
  * ``points_volume``   the signed distance volume of an oriented cloud
                        (rs_surface_points_volume, cloud_knn.hip)
  * ``points_field``    the same field, and colours, at given positions (rs_surface_points_eval)
  * ``from_points``     oriented cloud -> ``points_volume`` -> ``extract`` (-> ``clean``
                        -> ``simplify`` -> colours from ``points_field``)

Conventions are those of ``dense``: cameras are the project's normalised (3, 4) ``C``,
``P = K @ C``, pixel centres at integers, the depth of X in a view is ``C[2] @ [X; 1]`` and may
be negative.  A volume is indexed ``[iz, iy, ix]``; its node (ix, iy, iz) lies at
``origin + voxel * (ix, iy, iz)``.  The contract of both kernels stands in include/rsamd.h.
"""
from __future__ import annotations

import numpy as np

from . import _ffi, dense

_d = _ffi.C.c_double
_f = _ffi.C.c_float
_i32 = _ffi.C.c_int32

MAX_SIDE = 2048
MAX_NODES = 1 << 27
MAX_VIEWS = dense.MAX_VIEWS
STAGES = ("integrate", "classify", "scan", "emit")
TEXTURE_STAGES = ("raster_small", "raster_large", "gather")
RASTER_SMALL = 32            # RS_SURFACE_RASTER_SMALL
TEXTURE_LIST_CAP = 1 << 20   # RS_SURFACE_TEXTURE_LIST_CAP
MESH_STAGES = ("components", "compact", "adjacency", "smooth")
MESH_MAX_VERTICES = 1 << 27  # RS_MESH_MAX_VERTICES
MESH_MAX_FACES = 1 << 27     # RS_MESH_MAX_FACES
MESH_MAX_ROUNDS = 64         # RS_MESH_MAX_ROUNDS
MESH_MAX_ITERATIONS = 65536  # RS_MESH_MAX_ITERATIONS
MESH_SCAN_CHUNK = 2048       # RS_MESH_SCAN_CHUNK
SIMPLIFY_STAGES = ("cluster", "rows", "quadric", "faces")
SIMPLIFY_PLACEMENTS = ("mean", "quadric")   # RS_SIMPLIFY_MEAN, RS_SIMPLIFY_QUADRIC
SIMPLIFY_MAX_CELLS = 1 << 27                # RS_SIMPLIFY_MAX_CELLS
POINTS_STAGES = ("box", "grid", "scan", "scatter", "field")
POINTS_MAX_K = 64                           # RS_CLOUD_KNN_MAX_K
POINTS_MAX = 1 << 28                        # RS_CLOUD_MAX_POINTS


def _ctx(ctx):
    return (ctx or _ffi.default_context()).handle


def _grid(origin, voxel, dims):
    origin = _ffi.f64c(origin).reshape(-1)
    if origin.shape != (3,) or not np.all(np.isfinite(origin)):
        raise ValueError('origin must be three finite numbers')
    voxel = float(voxel)
    if not np.isfinite(voxel) or not voxel > 0.0:
        raise ValueError('voxel must be finite and positive')
    try:
        dims = tuple(int(n) for n in dims)
    except TypeError:
        raise ValueError('dims must be (nz, ny, nx)') from None
    if len(dims) != 3:
        raise ValueError('dims must be (nz, ny, nx)')
    if min(dims) < 1 or max(dims) > MAX_SIDE:
        raise ValueError('each side of the volume must be in 1..2048')
    if dims[0] * dims[1] * dims[2] > MAX_NODES:
        raise ValueError('a volume of more than 2^27 nodes')
    return origin, voxel, dims


def _volume(a, name, dims=None):
    a = np.asarray(a)
    if a.dtype != np.float32 or a.ndim != 3 or (dims is not None and a.shape != dims):
        raise ValueError(f'{name} must be a float32 volume' +
                         (f' of shape {dims}' if dims is not None else ' (nz, ny, nx)'))
    return np.ascontiguousarray(a)


def integrate(depth_maps, cams, K, origin, voxel, dims, trunc, weights=None, tsdf=None,
              weight=None, ctx=None):
    """TSDF fusion (rs_surface_integrate).  depth_maps is (V, h, w) float64 with NaN for "no
    depth", cams (V, 3, 4), ``weights`` (V, h, w) float32 or None for 1 everywhere.

    Per node X and view v, in index order and in fp64: q = P_v [X; 1], z = q[2], the pixel is
    (floor(q0 / z + 0.5), floor(q1 / z + 0.5)).  The view contributes when the pixel is inside,
    its depth d is finite, d z > 0, its weight wv is finite and > 0 and s = |d| - |z| >= -trunc;
    it adds wv min(1, s / trunc) to acc and wv to wsum.  W = W0 + wsum and
    T = (W0 T0 + acc) / W, NaN when W == 0.

    Returns (tsdf, weight), float32 (nz, ny, nx).  Given a running ``tsdf`` and ``weight`` (both
    or neither) the views are added to that volume; the arrays passed in are not modified.

    ValueError before any launch: a side of the volume outside 1..2048, more than 2^27 nodes, V
    outside 1..128, the image limits of ``dense.consistency``, cameras, origin or voxel not
    finite, voxel or trunc <= 0, shapes that do not match, a running volume of the wrong shape
    or dtype."""
    K = dense._calibration(K)
    depth = _ffi.f64c(depth_maps)
    cams = dense._cameras(cams, 'cams')
    if depth.ndim != 3 or len(depth) != len(cams):
        raise ValueError('depth_maps must be (V, h, w), one per camera')
    V, h, w = depth.shape
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError('1 to 128 views')
    if min(h, w) < 1 or max(h, w) > dense.MAX_SIDE or h * w > dense.MAX_PIXELS or \
            V * h * w > dense.MAX_VOLUME:
        raise ValueError('depth maps of more than 2^26 pixels each or 2^28 in all')
    origin, voxel, dims = _grid(origin, voxel, dims)
    trunc = float(trunc)
    if not np.isfinite(trunc) or not trunc > 0.0:
        raise ValueError('trunc must be finite and positive')
    if weights is not None:
        weights = np.asarray(weights)
        if weights.dtype != np.float32 or weights.shape != depth.shape:
            raise ValueError('weights must be float32 of the depth maps\' shape')
        weights = np.ascontiguousarray(weights)
    if (tsdf is None) != (weight is None):
        raise ValueError('a running volume is tsdf and weight together')
    prior = tsdf is not None
    if prior:
        tsdf = _volume(tsdf, 'tsdf', dims).copy()
        weight = _volume(weight, 'weight', dims).copy()
    else:
        tsdf, weight = np.empty(dims, np.float32), np.empty(dims, np.float32)
    P = np.ascontiguousarray(K @ cams)
    _ffi.check(_ffi.lib().rs_surface_integrate(
        _ctx(ctx), _ffi.ptr(depth, _d), _ffi.ptr(weights, _f) if weights is not None else None,
        V, h, w, _ffi.ptr(P, _d), _ffi.ptr(origin, _d), voxel, dims[0], dims[1], dims[2], trunc,
        int(prior), _ffi.ptr(tsdf, _f), _ffi.ptr(weight, _f)))
    return tsdf, weight


def extract(tsdf, weight, origin, voxel, min_weight=2.0, ctx=None):
    """Marching tetrahedra on the Kuhn decomposition of every cell (rs_surface_extract).

    A cell is valid when all 8 nodes have weight >= min_weight and a finite tsdf; a node is
    negative iff tsdf < 0.  A vertex sits on a tet edge whose nodes differ in sign and that a
    valid cell contains, at origin + voxel (o + t e) with t = fa / (fa - fb); vertices are
    numbered by owning node in row-major order, then by edge type, and faces by cell, tet and
    the case table's order.  The geometric normal of a face points to the positive side.

    Returns (vertices (Nv, 3) float64, faces (Nf, 3) int32); both are empty for a volume
    without a sign change in a valid cell.  The ABI is called twice: once with zero capacities
    for the sizes and once with exact arrays.

    ValueError before any launch: tsdf or weight not a 3-D float32 volume or of different
    shapes, the volume limits of ``integrate``, origin or voxel not finite, voxel <= 0,
    min_weight not finite or <= 0."""
    tsdf = _volume(tsdf, 'tsdf')
    weight = _volume(weight, 'weight', tsdf.shape)
    origin, voxel, dims = _grid(origin, voxel, tsdf.shape)
    min_weight = float(min_weight)
    if not np.isfinite(min_weight) or not min_weight > 0.0:
        raise ValueError('min_weight must be finite and positive')
    lib, h = _ffi.lib(), _ctx(ctx)
    nv, nf = _ffi.C.c_int64(-1), _ffi.C.c_int64(-1)

    def call(vertices, faces):
        return lib.rs_surface_extract(
            h, _ffi.ptr(tsdf, _f), _ffi.ptr(weight, _f), dims[0], dims[1], dims[2],
            _ffi.ptr(origin, _d), voxel, min_weight,
            _ffi.ptr(vertices, _d) if len(vertices) else None, len(vertices),
            _ffi.ptr(faces, _i32) if len(faces) else None, len(faces),
            _ffi.C.byref(nv), _ffi.C.byref(nf))

    vertices, faces = np.empty((0, 3)), np.empty((0, 3), np.int32)
    st = call(vertices, faces)
    if st != 0 and nv.value <= 0 and nf.value <= 0:
        _ffi.check(st)                     # an error, not "the mesh does not fit"
    if nv.value > 0 or nf.value > 0:
        if nv.value > 2**31 - 1 or 3 * nf.value > 2**31 - 1:
            _ffi.check(st)
        vertices = np.empty((nv.value, 3))
        faces = np.empty((nf.value, 3), np.int32)
        _ffi.check(call(vertices, faces))
    return vertices, faces


def bounds(points, voxel, margin=0.0):
    """(origin (3,), dims (nz, ny, nx)) of the smallest volume of `voxel` spacing whose nodes
    enclose the finite points of an (N, 3) cloud -- the cloud of ``dense.fuse`` for instance --
    with `margin` (world units) around it."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    pts = pts[np.all(np.isfinite(pts), axis=1)]
    voxel, margin = float(voxel), float(margin)
    if not len(pts):
        raise ValueError('no finite point')
    if not np.isfinite(voxel) or not voxel > 0.0 or not np.isfinite(margin) or margin < 0.0:
        raise ValueError('voxel must be finite and positive, margin finite and not negative')
    lo, hi = pts.min(axis=0) - margin, pts.max(axis=0) + margin
    n = np.ceil((hi - lo) / voxel).astype(np.int64) + 1      # nodes per axis, x y z
    return lo, (int(n[2]), int(n[1]), int(n[0]))


def vertex_normals(vertices, faces):
    """Unit vertex normals (Nv, 3): the sum of the adjacent faces' normals, each weighted by the
    face's area.  A vertex without a face of non-zero area gets a zero normal.  Host numpy."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])   # |fn| = 2 area
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.divide(n, length, out=np.zeros_like(n), where=length > 0)


def save_ply(path, vertices, faces=None, normals=None, colors=None):
    """Binary little-endian PLY: float x y z, optional float nx ny nz, optional uchar red green
    blue, and the faces as ``list uchar int vertex_indices`` (an ``element face 0`` without
    faces).  colors are uint8, or floats in [0, 1] as ``cloud`` gives them."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.zeros((0, 3), np.int32) if faces is None else np.asarray(faces).reshape(-1, 3)
    fields = [(n, '<f4') for n in 'xyz']
    props = [f'property float {n}' for n in 'xyz']
    if normals is not None:
        normals = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
        if len(normals) != len(v):
            raise ValueError('one normal per vertex')
        fields += [(n, '<f4') for n in ('nx', 'ny', 'nz')]
        props += [f'property float {n}' for n in ('nx', 'ny', 'nz')]
    if colors is not None:
        colors = np.asarray(colors).reshape(-1, 3)
        if len(colors) != len(v):
            raise ValueError('one colour per vertex')
        if colors.dtype != np.uint8:
            colors = np.clip(np.rint(colors.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
        fields += [(n, 'u1') for n in ('red', 'green', 'blue')]
        props += [f'property uchar {n}' for n in ('red', 'green', 'blue')]
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError('a face index is out of range')
    rec = np.zeros(len(v), dtype=fields)
    for k, n in enumerate('xyz'):
        rec[n] = v[:, k]
    if normals is not None:
        for k, n in enumerate(('nx', 'ny', 'nz')):
            rec[n] = normals[:, k]
    if colors is not None:
        for k, n in enumerate(('red', 'green', 'blue')):
            rec[n] = colors[:, k]
    frec = np.zeros(len(f), dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    frec['n'] = 3
    frec['i'] = f
    header = ['ply', 'format binary_little_endian 1.0', f'element vertex {len(v)}'] + props + \
        [f'element face {len(f)}', 'property list uchar int vertex_indices', 'end_header']
    with open(path, 'wb') as fh:
        fh.write(('\n'.join(header) + '\n').encode('ascii'))
        fh.write(rec.tobytes())
        fh.write(frec.tobytes())


def load_ply(path):
    """What ``save_ply`` writes, read back: a dict with vertices (Nv, 3) float64, faces (Nf, 3)
    int32, and normals (float64) and colors (uint8) or None.  Only that layout is understood:
    binary little-endian, float and uchar vertex properties, triangles."""
    with open(path, 'rb') as fh:
        data = fh.read()
    end = data.find(b'end_header\n')
    if not data.startswith(b'ply\n') or end < 0:
        raise ValueError('not a PLY file')
    lines = data[:end].decode('ascii').split('\n')
    body = data[end + len(b'end_header\n'):]
    if lines[1].strip() != 'format binary_little_endian 1.0':
        raise ValueError('only binary little-endian PLY is read')
    counts, fields, element = {}, [], None
    kinds = {'float': '<f4', 'uchar': 'u1'}
    for line in lines[2:]:
        tok = line.split()
        if not tok or tok[0] == 'comment':
            continue
        if tok[0] == 'element':
            element = tok[1]
            counts[element] = int(tok[2])
        elif tok[0] == 'property' and element == 'vertex':
            if tok[1] not in kinds:
                raise ValueError(f'vertex property type {tok[1]} is not read')
            fields.append((tok[2], kinds[tok[1]]))
        elif tok[0] == 'property' and element == 'face':
            if tok[1:4] != ['list', 'uchar', 'int']:
                raise ValueError('faces must be list uchar int')
    nv, nf = counts.get('vertex', 0), counts.get('face', 0)
    vdt = np.dtype(fields)
    fdt = np.dtype([('n', 'u1'), ('i', '<i4', (3,))])
    if len(body) < nv * vdt.itemsize + nf * fdt.itemsize:
        raise ValueError('the PLY file is truncated')
    rec = np.frombuffer(body, dtype=vdt, count=nv)
    frec = np.frombuffer(body, dtype=fdt, count=nf, offset=nv * vdt.itemsize)
    if nf and np.any(frec['n'] != 3):
        raise ValueError('only triangles are read')
    names = rec.dtype.names or ()

    def cols(keys, dtype):
        if not all(k in names for k in keys):
            return None
        return np.stack([rec[k] for k in keys], axis=1).astype(dtype)

    return {"vertices": cols('xyz', np.float64), "faces": frec['i'].astype(np.int32).reshape(-1, 3),
            "normals": cols(('nx', 'ny', 'nz'), np.float64),
            "colors": cols(('red', 'green', 'blue'), np.uint8)}


def _mesh(vertices, faces):
    vertices = _ffi.f64c(vertices)
    if vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError('vertices must be (Nv, 3)')
    faces = np.asarray(faces)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.kind not in 'iu':
        raise ValueError('faces must be (Nf, 3) integers')
    if len(vertices) > 2**31 - 1 or 3 * len(faces) > 2**31 - 1:
        raise ValueError('nv and 3 nf must be at most 2^31 - 1')
    if len(faces) and (faces.min() < 0 or faces.max() >= len(vertices)):
        raise ValueError('a face index is out of range')
    return vertices, np.ascontiguousarray(faces, dtype=np.int32)


def _views(cams, K, h, w):
    """P = K C of every view after the limits of ``dense.consistency``; the turn to positive
    depths and the test of det P[:, :3] are the ABI's."""
    K = dense._calibration(K)
    cams = dense._cameras(cams, 'cams')
    V = len(cams)
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError('1 to 128 views')
    if min(h, w) < 1 or max(h, w) > dense.MAX_SIDE or h * w > dense.MAX_PIXELS or \
            V * h * w > dense.MAX_VOLUME:
        raise ValueError('images of more than 2^26 pixels each or 2^28 in all')
    return np.ascontiguousarray(K @ cams)


def render_depth(vertices, faces, cams, K, shape, ctx=None):
    """The z-buffers of a mesh (rs_surface_render_depth): (V, h, w) float32 for ``shape`` (h, w),
    NaN where no face covers the pixel.  vertices (Nv, 3), faces (Nf, 3), cams (V, 3, 4).

    Every camera is turned so that depths are positive, P = s K C with s = sign det(K C)[:, :3].
    Per view and face, in fp64: q_i = P [X_i; 1]; the face is drawn iff q is finite and all three
    z_i = q_i2 > 0 -- a face that crosses the camera plane is skipped, not clipped -- and its
    projected area is neither 0 nor infinite.  Both windings are drawn.  A pixel centre (px, py)
    of the bounding box is covered iff its three barycentric coordinates, each from its own edge
    function, are >= 0; its depth is 1 / (b0 / z0 + b1 / z1 + b2 / z2) rounded to float32, and
    the pixel keeps the smallest.  Bitwise reproducible, whatever the order of the faces.

    ValueError before any launch: Nv or 3 Nf above 2^31 - 1, a face index out of range, V outside
    1..128, the image limits of ``dense.consistency``, a camera that is not finite or has
    det(K C)[:, :3] zero."""
    vertices, faces = _mesh(vertices, faces)
    try:
        h, w = (int(n) for n in shape)
    except (TypeError, ValueError):
        raise ValueError('shape must be (h, w)') from None
    P = _views(cams, K, h, w)
    depth = np.empty((len(P), h, w), np.float32)
    _ffi.check(_ffi.lib().rs_surface_render_depth(
        _ctx(ctx), _ffi.ptr(vertices, _d), len(vertices), _ffi.ptr(faces, _i32), len(faces),
        _ffi.ptr(P, _d), len(P), h, w, _ffi.ptr(depth, _f)))
    return depth


def vertex_colors(vertices, faces, images, cams, K, normals=None, rel_tol=0.01, min_cos=0.0,
                  return_depth=False, ctx=None):
    """A colour per mesh vertex from the views that see it (rs_surface_colorize).  images is
    (V, h, w) or (V, h, w, 3) uint8, normals (Nv, 3) or None.

    The z-buffers of ``render_depth`` are the occluder.  Per vertex and view, in index order and
    fp64: the view is skipped unless the vertex lies in front and projects to (u, v) inside
    [0, w - 1] x [0, h - 1].  It is visible iff its depth z <= far (1 + rel_tol), far the largest
    finite z-buffer value among the four pixels of the bilinear footprint of (u, v).  With
    normals the view contributes iff g = n . (c - X) / |c - X| > min_cos, c the camera centre,
    with weight g; without them the weight is 1.  The colour is the weighted mean of the
    bilinear samples, divided by 255.

    Returns (colors (Nv, ch) float64 in [0, 1], count (Nv,) int32: the views that contributed;
    the colour is 0 where it is 0), and the z-buffers (V, h, w) float32 as a third item when
    ``return_depth`` is set.  Bitwise reproducible.

    ValueError before any launch: what ``render_depth`` lists, images not uint8 of such a shape
    or not one per camera, normals not (Nv, 3), rel_tol not finite or negative, min_cos not
    finite."""
    vertices, faces = _mesh(vertices, faces)
    images = np.asarray(images)
    if images.dtype != np.uint8 or images.ndim not in (3, 4) or \
            (images.ndim == 4 and images.shape[3] != 3):
        raise ValueError('images must be uint8 (V, h, w) or (V, h, w, 3)')
    images = np.ascontiguousarray(images)
    V, h, w = images.shape[:3]
    ch = 1 if images.ndim == 3 else 3
    P = _views(cams, K, h, w)
    if len(P) != V:
        raise ValueError('one image per camera')
    if normals is not None:
        normals = _ffi.f64c(normals)
        if normals.shape != vertices.shape:
            raise ValueError('normals must be (Nv, 3)')
    rel_tol, min_cos = float(rel_tol), float(min_cos)
    if not np.isfinite(rel_tol) or rel_tol < 0.0 or not np.isfinite(min_cos):
        raise ValueError('rel_tol must be finite and not negative, min_cos finite')
    nv = len(vertices)
    colors, count = np.empty((nv, ch)), np.empty(nv, np.int32)
    depth = np.empty((V, h, w), np.float32) if return_depth else None
    _ffi.check(_ffi.lib().rs_surface_colorize(
        _ctx(ctx), _ffi.ptr(vertices, _d), nv, _ffi.ptr(faces, _i32), len(faces),
        _ffi.ptr(images, _ffi.C.c_uint8), ch, _ffi.ptr(P, _d), V, h, w,
        _ffi.ptr(normals, _d) if normals is not None else None, rel_tol, min_cos,
        _ffi.ptr(colors, _d), _ffi.ptr(count, _i32),
        _ffi.ptr(depth, _f) if return_depth else None))
    return (colors, count, depth) if return_depth else (colors, count)


def _index_mesh(faces, n_vertices):
    """faces as contiguous (Nf, 3) int32 after the ABI's size and range rules."""
    faces = np.asarray(faces)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.kind not in 'iu':
        raise ValueError('faces must be (Nf, 3) integers')
    if n_vertices > MESH_MAX_VERTICES or len(faces) > MESH_MAX_FACES:
        raise ValueError('more than 2^27 vertices or faces')
    if len(faces) and (faces.min() < 0 or faces.max() >= n_vertices):
        raise ValueError('a face index is out of range')
    return np.ascontiguousarray(faces, dtype=np.int32)


def _mask(a, name, n):
    a = np.asarray(a)
    if a.dtype not in (np.bool_, np.uint8) or a.shape != (n,):
        raise ValueError(f'{name} must be bool or uint8 of shape (Nv,)')
    return np.ascontiguousarray(a, dtype=np.uint8)


def components(faces, n_vertices, return_rounds=False, ctx=None):
    """Connected components over shared vertex indices (rs_mesh_components).  faces is (Nf, 3)
    integers in 0..n_vertices - 1; a face may repeat an index.

    Returns (label (Nv,) int32: the smallest vertex index of the vertex's component, a vertex in
    no face labels itself; size (Nv,) int32: the faces of the vertex's component, 0 for a vertex
    in no face; count: the number of components, the vertices in no face included), and as a
    fourth item, when ``return_rounds`` is set, the hook rounds the device ran.

    ValueError before any launch: faces not (Nf, 3) integers, more than 2^27 vertices or faces,
    a face index out of range."""
    try:
        n = int(n_vertices)
    except (TypeError, ValueError):
        raise ValueError('n_vertices must be an integer') from None
    if n < 0:
        raise ValueError('n_vertices must not be negative')
    faces = _index_mesh(faces, n)
    label, size = np.empty(n, np.int32), np.empty(n, np.int32)
    count, rounds = _ffi.C.c_int64(0), _ffi.C.c_int32(0)
    _ffi.check(_ffi.lib().rs_mesh_components(
        _ctx(ctx), _ffi.ptr(faces, _i32) if len(faces) else None, len(faces), n,
        _ffi.ptr(label, _i32) if n else None, _ffi.ptr(size, _i32) if n else None,
        _ffi.C.byref(count), _ffi.C.byref(rounds)))
    if return_rounds:
        return label, size, count.value, rounds.value
    return label, size, count.value


def compact(vertices, faces, keep, ctx=None):
    """Drop the vertices where ``keep`` (Nv, bool or uint8) is false and renumber
    (rs_mesh_compact).  Returns (vertices: the kept ones in their order, bit for bit; faces: those
    all three of whose vertices are kept, in their order, with the new indices; vmap (Nv,) int32:
    the new index of a vertex or -1).  The ABI is called twice, as in ``extract``.

    ValueError before any launch: vertices not (Nv, 3), what ``components`` lists, keep not a
    bool or uint8 mask of length Nv."""
    vertices = _ffi.f64c(vertices)
    if vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError('vertices must be (Nv, 3)')
    n = len(vertices)
    faces = _index_mesh(faces, n)
    keep = _mask(keep, 'keep', n)
    lib, h = _ffi.lib(), _ctx(ctx)
    nv, nf = _ffi.C.c_int64(-1), _ffi.C.c_int64(-1)
    vmap = np.empty(n, np.int32)

    def call(vout, fout):
        return lib.rs_mesh_compact(
            h, _ffi.ptr(vertices, _d) if n else None, n,
            _ffi.ptr(faces, _i32) if len(faces) else None, len(faces),
            _ffi.ptr(keep, _ffi.C.c_uint8) if n else None,
            _ffi.ptr(vout, _d) if len(vout) else None, len(vout),
            _ffi.ptr(fout, _i32) if len(fout) else None, len(fout),
            _ffi.ptr(vmap, _i32) if n else None, _ffi.C.byref(nv), _ffi.C.byref(nf))

    vout, fout = np.empty((0, 3)), np.empty((0, 3), np.int32)
    st = call(vout, fout)
    if st != 0 and nv.value <= 0 and nf.value <= 0:
        _ffi.check(st)                     # an error, not "the result does not fit"
    if nv.value > 0 or nf.value > 0:
        vout = np.empty((nv.value, 3))
        fout = np.empty((nf.value, 3), np.int32)
        _ffi.check(call(vout, fout))
    return vout, fout, vmap


def _keep_components(label, size, n_faces, min_faces, keep_largest, min_fraction):
    """The vertex mask of ``remove_small`` from ``components``' label and size: host numpy."""
    if min_faces is None and keep_largest is None and min_fraction is None:
        raise ValueError('give at least one of min_faces, keep_largest, min_fraction')
    keep = size > 0                                   # a vertex in no face is dropped
    if min_faces is not None:
        keep &= size >= int(min_faces)
    if min_fraction is not None:
        min_fraction = float(min_fraction)
        if not 0.0 <= min_fraction <= 1.0:
            raise ValueError('min_fraction must be in [0, 1]')
        keep &= size >= min_fraction * n_faces
    if keep_largest is not None:
        k = int(keep_largest)
        if k < 0:
            raise ValueError('keep_largest must not be negative')
        roots = np.flatnonzero((label == np.arange(len(label))) & (size > 0))
        # the largest first, ties to the smaller label: roots ascends and the sort is stable
        best = roots[np.argsort(-size[roots].astype(np.int64), kind='stable')[:k]]
        keep &= np.isin(label, best)
    return keep


def remove_small(vertices, faces, min_faces=None, keep_largest=None, min_fraction=None,
                 ctx=None):
    """Drop the small components of a mesh: ``components``, a policy in host numpy, ``compact``.
    A component stays when it meets every criterion given: at least ``min_faces`` faces, among
    the ``keep_largest`` components of most faces (ties go to the smaller label), at least
    ``min_fraction`` of all faces.  Vertices in no face are dropped.  Returns (vertices, faces,
    vmap) as ``compact``.

    ValueError before any launch: what ``compact`` lists, no criterion given."""
    if min_faces is None and keep_largest is None and min_fraction is None:
        raise ValueError('give at least one of min_faces, keep_largest, min_fraction')
    vertices = _ffi.f64c(vertices)
    if vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError('vertices must be (Nv, 3)')
    faces = _index_mesh(faces, len(vertices))
    label, size, _ = components(faces, len(vertices), ctx=ctx)
    keep = _keep_components(label, size, len(faces), min_faces, keep_largest, min_fraction)
    return compact(vertices, faces, keep, ctx=ctx)


def smooth(vertices, faces, iterations=10, lam=0.5, mu=-0.53, fixed=None, pin_boundary=True,
           ctx=None):
    """Taubin's lambda|mu smoothing with uniform weights (rs_mesh_smooth).

    N(v) is the set of vertices other than v that share a face with v.  A pass with factor f, in
    fp64 without fused products: s = the sum of x_u over N(v) in ascending order of u,
    x'_v = x_v + f (s / |N(v)| - x_v).  One iteration is a pass with ``lam``, then one with
    ``mu``.  A vertex is fixed where ``fixed`` (Nv, bool or uint8) is set and, with
    ``pin_boundary``, where it ends a boundary edge (an edge of exactly one face); a fixed
    vertex, and one without a neighbour, keeps its bits.  Returns the new (Nv, 3) float64
    vertices, the input's bits for ``iterations=0``.  Bitwise reproducible.

    ValueError before any launch: vertices not (Nv, 3) or not finite, what ``components``
    lists, iterations outside 0..65536, lam or mu not finite, fixed not a mask of length Nv."""
    vertices = _ffi.f64c(vertices)
    if vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError('vertices must be (Nv, 3)')
    n = len(vertices)
    faces = _index_mesh(faces, n)
    if not np.all(np.isfinite(vertices)):
        raise ValueError('the vertices must be finite')
    iterations, lam, mu = int(iterations), float(lam), float(mu)
    if not 0 <= iterations <= MESH_MAX_ITERATIONS:
        raise ValueError('iterations must be in 0..65536')
    if not np.isfinite(lam) or not np.isfinite(mu):
        raise ValueError('lam and mu must be finite')
    if fixed is not None:
        fixed = _mask(fixed, 'fixed', n)
    out = np.empty_like(vertices)
    _ffi.check(_ffi.lib().rs_mesh_smooth(
        _ctx(ctx), _ffi.ptr(vertices, _d) if n else None, n,
        _ffi.ptr(faces, _i32) if len(faces) else None, len(faces), iterations, lam, mu,
        _ffi.ptr(fixed, _ffi.C.c_uint8) if fixed is not None and n else None,
        int(bool(pin_boundary)), _ffi.ptr(out, _d) if n else None))
    return out


def clean(vertices, faces, min_faces=None, keep_largest=None, min_fraction=None, iterations=10,
          lam=0.5, mu=-0.53, pin_boundary=True, ctx=None):
    """``remove_small`` with the criteria given (skipped when there is none), then ``smooth``
    (skipped for ``iterations=0``).  Returns (vertices, faces, vmap); vmap is the identity when
    no component was looked at."""
    if min_faces is None and keep_largest is None and min_fraction is None:
        vertices, faces = _ffi.f64c(vertices), _index_mesh(faces, len(vertices))
        vmap = np.arange(len(vertices), dtype=np.int32)
    else:
        vertices, faces, vmap = remove_small(vertices, faces, min_faces, keep_largest,
                                             min_fraction, ctx=ctx)
    if iterations:
        vertices = smooth(vertices, faces, iterations, lam, mu, pin_boundary=pin_boundary,
                          ctx=ctx)
    return vertices, faces, vmap


_clean = clean    # ``reconstruct`` has a keyword of that name


def simplify_grid(vertices, cell, origin=None):
    """The grid ``simplify`` clusters on: (origin (3,) float64, dims (d0, d1, d2) along x, y, z).
    With ``origin=None`` the origin is the per-axis minimum of the vertices;
    ``dims = floor((max - origin) / cell) + 1``, so the largest coordinate lies in the last cell.
    An empty mesh gets the origin 0 and one cell.  ValueError: vertices not (Nv, 3) or not finite,
    cell not finite or not positive, origin not three finite numbers, more than 2^27 cells."""
    vertices = _ffi.f64c(vertices)
    if vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError('vertices must be (Nv, 3)')
    if not np.all(np.isfinite(vertices)):
        raise ValueError('the vertices must be finite')
    cell = float(cell)
    if not np.isfinite(cell) or not cell > 0.0:
        raise ValueError('cell must be finite and positive')
    if origin is None:
        origin = vertices.min(axis=0) if len(vertices) else np.zeros(3)
    origin = _ffi.f64c(origin).reshape(-1)
    if origin.shape != (3,) or not np.all(np.isfinite(origin)):
        raise ValueError('origin must be three finite numbers')
    if not len(vertices):
        return origin, (1, 1, 1)
    top = np.floor((vertices.max(axis=0) - origin) / cell)
    if np.any(top < 0.0):
        raise ValueError('a vertex lies outside the grid')
    if np.any(top >= SIMPLIFY_MAX_CELLS) or np.prod(top + 1.0) > SIMPLIFY_MAX_CELLS:
        raise ValueError('a grid of more than 2^27 cells')
    return origin, tuple(int(t) + 1 for t in top)


def simplify(vertices, faces, cell, origin=None, placement="quadric", rank_tol=1e-3,
             drop_unreferenced=True, return_info=False, ctx=None):
    """Vertex clustering on a uniform grid of spacing ``cell`` (rs_mesh_simplify): all vertices
    of a cell become one vertex, placed by the cell's error quadric (Lindstrom 2000).

    The grid is ``simplify_grid``'s.  A vertex belongs to cell ``floor((x - origin) / cell)``
    per axis, a vertex on a cell face to the upper cell; occupied cells are numbered in ascending
    order of ``(i2 * d1 + i1) * d0 + i0``.  ``placement="mean"`` puts the new vertex at the mean
    of the cell's vertices.  ``"quadric"`` accumulates, over the faces with a corner in the cell,
    the squared distance to their planes weighted by squared area and moves the mean to its
    minimum within the eigenvectors whose eigenvalue exceeds ``rank_tol`` times the largest; a
    position that is not finite or leaves the cell falls back to the mean.  A face two of whose
    corners share a cell is dropped, and of the faces with the same three cells the first stays;
    the others keep their order and orientation.  Every new vertex lies in the cell of the
    vertices it replaces, so no vertex moves further than ``cell`` along an axis.  All fp64 with
    every sum in a stated order (include/rsamd.h): bitwise reproducible.

    Returns (vertices (Nc, 3) float64, faces (Nk, 3) int32, vmap (Nv,) int32: the new index of
    an input vertex).  With ``drop_unreferenced`` the new vertices that no remaining face names
    are removed with ``compact`` and vmap is -1 for the input vertices they stood for.  With
    ``return_info`` a fourth item: a dict of ``clusters`` (occupied cells), ``fallbacks``,
    ``degenerate_faces``, ``duplicate_faces``, ``longest_row`` (the most items one lane sorted),
    ``unreferenced`` (occupied cells no remaining face names), ``fmap`` ((Nf,) int32: the new
    index of an input face, -1 for a degenerate face, -2 for a duplicate) and ``quadrics``
    ((Nc, 10) float64 of the returned vertices).

    ValueError before any launch: what ``simplify_grid`` and ``components`` list, a vertex
    outside the grid of a given ``origin``, placement not "mean" or "quadric", rank_tol outside
    [0, 1)."""
    vertices = _ffi.f64c(vertices)
    origin, dims = simplify_grid(vertices, cell, origin)
    n = len(vertices)
    faces = _index_mesh(faces, n)
    if placement not in SIMPLIFY_PLACEMENTS:
        raise ValueError('placement must be "mean" or "quadric"')
    cell, rank_tol = float(cell), float(rank_tol)
    if not 0.0 <= rank_tol < 1.0:
        raise ValueError('rank_tol must be in [0, 1)')
    m = len(faces)
    # the result is never larger than the input: one call with the input's sizes as capacities
    vout, fout = np.empty((n, 3)), np.empty((m, 3), np.int32)
    vmap, fmap = np.empty(n, np.int32), np.empty(m, np.int32)
    quad = np.empty((n, 10))
    nv, nf = _ffi.C.c_int64(0), _ffi.C.c_int64(0)
    rec = _ffi.SimplifyInfo()
    d = np.array(dims, dtype=np.int64)
    _ffi.check(_ffi.lib().rs_mesh_simplify(
        _ctx(ctx), _ffi.ptr(vertices, _d) if n else None, n,
        _ffi.ptr(faces, _i32) if m else None, m, _ffi.ptr(origin, _d), cell,
        _ffi.ptr(d, _ffi.C.c_int64), SIMPLIFY_PLACEMENTS.index(placement), rank_tol,
        _ffi.ptr(vout, _d) if n else None, n, _ffi.ptr(fout, _i32) if m else None, m,
        _ffi.ptr(vmap, _i32) if n else None, _ffi.ptr(fmap, _i32) if m else None,
        _ffi.ptr(quad, _d) if n else None, _ffi.C.byref(nv), _ffi.C.byref(nf),
        _ffi.C.byref(rec)))
    vout, fout, quad = vout[:nv.value].copy(), fout[:nf.value].copy(), quad[:nv.value].copy()
    keep = np.zeros(len(vout), np.uint8)
    keep[fout.reshape(-1)] = 1
    unreferenced = int(len(keep) - keep.sum())
    if drop_unreferenced and unreferenced:
        vout, fout, cmap = compact(vout, fout, keep, ctx=ctx)
        vmap, quad = cmap[vmap], quad[keep != 0]
    if not return_info:
        return vout, fout, vmap
    info = {k: int(getattr(rec, k)) for k, _ in _ffi.SimplifyInfo._fields_}
    info.update(unreferenced=unreferenced, fmap=fmap, quadrics=quad)
    return vout, fout, vmap, info


_simplify = simplify    # ``reconstruct`` has a keyword of that name


def reconstruct(images, cams, K, depths, origin, voxel, dims, trunc, min_weight=2, ctx=None,
                colors=False, clean=None, simplify=None, **fuse_kw):
    """Posed images to a mesh: ``dense.fuse(..., return_maps=True)``, the depth set to NaN where
    ``keep`` is false, ``integrate`` with ``count`` as the weight, ``extract``.  ``fuse_kw`` goes
    to ``dense.fuse``: ``smooth=(p1, p2)`` there picks the depth maps' winners after semi-global
    aggregation.  ``clean``, a dict of the keywords of ``clean``, applies that function to the
    extracted mesh before anything else uses it; with None the mesh is ``extract``'s.
    ``simplify``, a dict of the keywords of ``simplify`` (``cell`` at least), applies that
    function after ``clean`` and before the colours; with None nothing changes.  Returns
    (vertices, faces, tsdf, weight), and with ``colors=True``
    (vertices, faces, tsdf, weight, colors): the first item of ``vertex_colors`` on the same
    images, with the mesh's ``vertex_normals``."""
    fuse_kw.pop('return_maps', None)
    maps = dense.fuse(images, cams, K, depths, return_maps=True, ctx=ctx, **fuse_kw)[-1]
    depth = np.where(maps["keep"], maps["depth"], np.nan)
    tsdf, weight = integrate(depth, cams, K, origin, voxel, dims, trunc,
                             weights=maps["count"].astype(np.float32), ctx=ctx)
    vertices, faces = extract(tsdf, weight, origin, voxel, min_weight=min_weight, ctx=ctx)
    if clean is not None:
        vertices, faces, _ = _clean(vertices, faces, ctx=ctx, **dict(clean))
    if simplify is not None:
        vertices, faces = _simplify(vertices, faces, ctx=ctx,
                                    **dict(simplify, return_info=False))[:2]
    if not colors:
        return vertices, faces, tsdf, weight
    col = vertex_colors(vertices, faces, images, cams, K,
                        normals=vertex_normals(vertices, faces), ctx=ctx)[0]
    return vertices, faces, tsdf, weight, col


def _oriented(points, normals, k, radius, cell):
    """points and normals as contiguous (n, 3) float64 after the ABI's rules for k, radius, cell."""
    points, normals = _ffi.f64c(points), _ffi.f64c(normals)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError('points must be (n, 3)')
    if normals.shape != points.shape:
        raise ValueError('normals must have the shape of points')
    if len(points) > POINTS_MAX:
        raise ValueError('more points than RS_CLOUD_MAX_POINTS = 2^28')
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError('k must be an integer')
    if not 1 <= k <= POINTS_MAX_K:
        raise ValueError('k must be in 1..64 (RS_CLOUD_KNN_MAX_K)')
    radius = float(radius)
    if not np.isfinite(radius) or not radius > 0.0:
        raise ValueError('radius must be finite and positive')
    cell = 0.0 if cell is None else float(cell)
    if not np.isfinite(cell) or cell < 0.0:
        raise ValueError('cell must be finite and >= 0 (None or 0: the default)')
    return points, normals, int(k), radius, cell


def _points_info(info):
    return {"cells": info.cells, "largest_cell": info.largest_cell, "tested": info.tested,
            "defined": info.defined, "saturated": info.saturated}


def points_volume(points, normals, origin, voxel, dims, radius, k=16, trunc=None, cell=None,
                  return_info=False, ctx=None):
    """The signed distance volume of an oriented cloud (rs_surface_points_volume): an implicit
    moving-least-squares field over the k nearest points within ``radius`` of every node.

    points and normals are (n, 3) float64; a point with a non-finite number among its six is
    out, and normals are used as given.  The list of a node X is ``cloud.knn``'s row for the
    query X with ``max_dist=radius``.  Per slot in list order, in fp64 without fused products:
    u = min(sqrt(d2) / radius, 1), a = 1 - u, w = (a^2 a^2)(4 u + 1) (Wendland C2, 0 at the
    rim), acc += w (X - p_j) . n_j, sw += w; f = acc / sw, NaN when sw is not > 0.  f > 0 on the
    side the normals point to.  The result depends neither on ``cell`` (None: a hair above
    ``radius``, which ends the walk after 27 cells) nor on
    anything else about the grid, and two calls give the same bits.

    Returns (tsdf, weight), float32 (nz, ny, nx): tsdf = clip(f / trunc, -1, 1), NaN where f is
    (``trunc=None``: ``radius``), and weight = the number of neighbours, so that
    ``extract(..., min_weight=m)`` keeps the cells with at least m points within ``radius`` of
    all 8 corners.  With ``return_info`` a third item: dict(cells, largest_cell, tested, defined:
    nodes with a finite value, saturated: nodes whose list was full).

    ValueError before any launch: points or normals not (n, 3), k outside 1..64, radius or trunc
    not finite or <= 0, cell negative or not finite, the volume limits of ``integrate``, origin
    or voxel not finite, voxel <= 0."""
    points, normals, k, radius, cell = _oriented(points, normals, k, radius, cell)
    origin, voxel, dims = _grid(origin, voxel, dims)
    trunc = radius if trunc is None else float(trunc)
    if not np.isfinite(trunc) or not trunc > 0.0:
        raise ValueError('trunc must be finite and positive')
    tsdf, weight = np.empty(dims, np.float32), np.empty(dims, np.float32)
    info = _ffi.PointsInfo()
    n = len(points)
    _ffi.check(_ffi.lib().rs_surface_points_volume(
        _ctx(ctx), _ffi.ptr(points, _d) if n else None, _ffi.ptr(normals, _d) if n else None, n,
        k, radius, trunc, cell, _ffi.ptr(origin, _d), voxel, dims[0], dims[1], dims[2],
        _ffi.ptr(tsdf, _f), _ffi.ptr(weight, _f), _ffi.C.byref(info)))
    return (tsdf, weight, _points_info(info)) if return_info else (tsdf, weight)


def points_field(points, normals, queries, radius, k=16, colors=None, cell=None,
                 return_info=False, ctx=None):
    """The field of ``points_volume`` at caller positions (rs_surface_points_eval).  queries is
    (m, 3); colors (n, 3) float64 or None.

    Returns (value (m,) float64: the unclamped f; count (m,) int32: the neighbours found), with
    colours a third item color (m, 3) = sum w col_j / sum w over the same list, NaN where f is,
    and with ``return_info`` the info of ``points_volume`` last.  A non-finite query has count 0
    and NaN.

    ValueError before any launch: what ``points_volume`` lists for the cloud, queries not
    (m, 3) or more than 2^28, colors not of the points' shape."""
    points, normals, k, radius, cell = _oriented(points, normals, k, radius, cell)
    queries = _ffi.f64c(queries)
    if queries.ndim != 2 or queries.shape[1] != 3:
        raise ValueError('queries must be (m, 3)')
    if len(queries) > POINTS_MAX:
        raise ValueError('more queries than RS_CLOUD_MAX_POINTS = 2^28')
    if colors is not None:
        colors = _ffi.f64c(colors)
        if colors.shape != points.shape:
            raise ValueError('colors must have the shape of points')
    n, m = len(points), len(queries)
    value, count = np.full(m, np.nan), np.zeros(m, np.int32)
    color = np.full((m, 3), np.nan) if colors is not None else None
    info = _ffi.PointsInfo()
    # an empty cloud has no array to point to: the call then takes no colours either
    with_col = colors is not None and n > 0
    _ffi.check(_ffi.lib().rs_surface_points_eval(
        _ctx(ctx), _ffi.ptr(points, _d) if n else None, _ffi.ptr(normals, _d) if n else None,
        _ffi.ptr(colors, _d) if with_col else None, n, _ffi.ptr(queries, _d) if m else None, m,
        k, radius, cell, _ffi.ptr(value, _d) if m else None, _ffi.ptr(count, _i32) if m else None,
        _ffi.ptr(color, _d) if with_col else None, _ffi.C.byref(info)))
    out = (value, count) if colors is None else (value, count, color)
    return out + (_points_info(info),) if return_info else out


def oriented_cloud(points, normals, colors=None):
    """The rows ``from_points`` works on: (points, unit normals, colours or None, keep (n,) bool).
    A row goes when one of its numbers (the colours included) is not finite or its normal is
    zero; the normals that stay are divided by their length.  Host numpy."""
    points, normals = _ffi.f64c(points), _ffi.f64c(normals)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError('points must be (n, 3)')
    if normals.shape != points.shape:
        raise ValueError('normals must have the shape of points')
    keep = np.isfinite(points).all(axis=1) & np.isfinite(normals).all(axis=1)
    if colors is not None:
        colors = np.asarray(colors)
        if colors.shape != points.shape or colors.dtype.kind not in 'fiu':
            raise ValueError('colors must have the shape of points')
        colors = colors.astype(np.float64) / (255.0 if colors.dtype == np.uint8 else 1.0)
        keep &= np.isfinite(colors).all(axis=1)
    with np.errstate(invalid='ignore', over='ignore'):
        length = np.sqrt((normals * normals).sum(axis=1))
    keep &= np.isfinite(length) & (length > 0.0)
    unit = normals[keep] / length[keep, None]
    return (np.ascontiguousarray(points[keep]), np.ascontiguousarray(unit),
            np.ascontiguousarray(colors[keep]) if colors is not None else None, keep)


def from_points(points, normals, voxel, radius, k=16, min_count=3, margin=None, colors=None,
                clean=None, simplify=None, return_info=False, ctx=None):
    """An oriented cloud to a mesh: ``oriented_cloud`` (rows with a non-finite entry or a zero
    normal go, normals become unit vectors), ``bounds(points, voxel, margin)`` with
    ``margin=None`` for two voxels, ``points_volume`` with ``trunc = radius``, and
    ``extract(..., min_weight=min_count)``: a cell is meshed when every corner has at least
    ``min_count`` points within ``radius``.  ``clean`` and ``simplify`` are dicts of those
    functions' keywords, applied in that order as ``reconstruct`` applies them.

    With ``colors`` (n, 3), uint8 or floats in [0, 1] as ``cloud.point_attributes`` gives them,
    the colour of a vertex is ``points_field``'s at the final vertices, as uint8 after
    ``rint(255 c)`` clipped to 0..255; a vertex without a neighbour gets 0, the fill of
    ``vertex_colors``.

    Returns (vertices, faces), with colours (vertices, faces, vertex_colors (Nv, 3) uint8), and
    with ``return_info`` a dict last: the info of ``points_volume`` plus origin, dims and points
    (the rows that stayed)."""
    pts, unit, col, keep = oriented_cloud(points, normals, colors)
    voxel = float(voxel)
    if not np.isfinite(voxel) or not voxel > 0.0:
        raise ValueError('voxel must be finite and positive')
    origin, dims = bounds(pts, voxel, 2.0 * voxel if margin is None else margin)
    tsdf, weight, info = points_volume(pts, unit, origin, voxel, dims, radius, k=k,
                                       return_info=True, ctx=ctx)
    vertices, faces = extract(tsdf, weight, origin, voxel, min_weight=min_count, ctx=ctx)
    if clean is not None:
        vertices, faces, _ = _clean(vertices, faces, ctx=ctx, **dict(clean))
    if simplify is not None:
        vertices, faces = _simplify(vertices, faces, ctx=ctx,
                                    **dict(simplify, return_info=False))[:2]
    out = (vertices, faces)
    if col is not None:
        c = points_field(pts, unit, vertices, radius, k=k, colors=col, ctx=ctx)[2]
        c = np.where(np.isnan(c), 0.0, c)
        out += (np.clip(np.rint(c * 255.0), 0, 255).astype(np.uint8),)
    if return_info:
        info.update(origin=origin, dims=dims, points=int(keep.sum()))
        out += (info,)
    return out


def timing(enable, ctx=None):
    """Enable / disable HIP events around the kernels of the next surface calls
    (rs_surface_timing); returns the last timed calls' {integrate, classify, scan, emit: device
    ms}, -1 where none."""
    ctx = ctx or _ffi.default_context()
    ms = np.zeros(len(STAGES))
    _ffi.check(_ffi.lib().rs_surface_timing(ctx.handle, int(enable), _ffi.ptr(ms, _d)))
    return dict(zip(STAGES, ms.tolist()))


def mesh_timing(enable, ctx=None):
    """The same for the next ``components``, ``compact`` and ``smooth`` calls (rs_mesh_timing):
    {components, compact, adjacency, smooth: device ms}, -1 where none."""
    ctx = ctx or _ffi.default_context()
    ms = np.zeros(len(MESH_STAGES))
    _ffi.check(_ffi.lib().rs_mesh_timing(ctx.handle, int(enable), _ffi.ptr(ms, _d)))
    return dict(zip(MESH_STAGES, ms.tolist()))


def simplify_timing(enable, ctx=None):
    """The same for the next ``simplify`` calls (rs_simplify_timing): {cluster, rows, quadric,
    faces: device ms}, -1 where none.  ``mesh_timing`` does not see these calls, nor this one the
    ``compact`` that ``drop_unreferenced`` runs."""
    ctx = ctx or _ffi.default_context()
    ms = np.zeros(len(SIMPLIFY_STAGES))
    _ffi.check(_ffi.lib().rs_simplify_timing(ctx.handle, int(enable), _ffi.ptr(ms, _d)))
    return dict(zip(SIMPLIFY_STAGES, ms.tolist()))


def texture_timing(enable, ctx=None):
    """The same for the next ``render_depth`` and ``vertex_colors`` calls
    (rs_surface_texture_timing): {raster_small, raster_large, gather: device ms}, -1 where none.
    ``timing`` does not see these calls."""
    ctx = ctx or _ffi.default_context()
    ms = np.zeros(len(TEXTURE_STAGES))
    _ffi.check(_ffi.lib().rs_surface_texture_timing(ctx.handle, int(enable), _ffi.ptr(ms, _d)))
    return dict(zip(TEXTURE_STAGES, ms.tolist()))


def points_timing(enable, ctx=None):
    """The same for the next ``points_volume`` and ``points_field`` calls
    (rs_surface_points_timing): {box, grid, scan, scatter, field: device ms}, -1 where none.
    ``cloud.knn_timing`` does not see these calls."""
    ctx = ctx or _ffi.default_context()
    ms = np.zeros(len(POINTS_STAGES))
    _ffi.check(_ffi.lib().rs_surface_points_timing(ctx.handle, int(enable), _ffi.ptr(ms, _d)))
    return dict(zip(POINTS_STAGES, ms.tolist()))
