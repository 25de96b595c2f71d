#!/usr/bin/env python
"""Time mesh colouring (surface.render_depth, surface.vertex_colors, csrc/surface_texture.hip) and
the numpy restatement of the same definitions on this host's CPU.

Inputs: the scene of tools/bench_surface.py -- the slanted plane of tests/dense_fixture.py in 16
views of 576 x 720, fused into a 256^3 volume -- and the mesh surface.extract makes of it; the
views' own rendered images are the colour source and the mesh's vertex_normals the normals.

GPU figures, after `--warmup` calls of vertex_colors: `kernel_ms` is the device time between HIP
events around a slot's kernels (rs_surface_texture_timing: raster_small is the fill and the
lane-per-face kernel, raster_large the wave-per-face kernel and the +inf to NaN pass, gather the
lane-per-vertex kernel; no upload, no download), `wall_ms` the host clock around the whole
synchronous Python call; median, min and max of the timed calls.  `face_views_per_second` = faces
x views over the two raster slots, `vertex_views_per_second` = vertices x views over the gather.
For the gather `bytes` is the least it must move, counted from the shapes: positions and normals
in, colours and counts out, every z-buffer pixel and image byte once; `copy_rate_fraction` is that
over the kernel time against the 6.29e12 B/s a float4 copy kernel reaches on the MI355X.

CPU baseline: tests/texture_ref.py once on the mesh of a `--cpu-side`^3 volume with 4 views of
72 x 90, with the same rates and the differences to the GPU's result.  Needs a GPU; there is no
fallback.  Writes one JSON file (default profiles/texture_bench.json) and prints it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tsbb15-3d-reconstruction-project_amd"),
          os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

COPY_RATE = 6.29e12   # bytes / s, a float4 copy kernel over HBM3E


def stats(x):
    return {"median": round(float(np.median(x)), 4), "min": round(float(min(x)), 4),
            "max": round(float(max(x)), 4)}


def gather_bytes(nv, V, h, w, ch):
    return nv * (24 + 24 + 8 * ch + 4) + V * h * w * (4 + ch)


def make_mesh(df, surface, bs, h, w, V, side):
    """(vertices, faces, images, cams, K) of bench_surface's scene at this size."""
    depth, cams, K = bs.make_scene(df, h, w, V)
    images = np.array([df.render(C, df.SLANTED, h, w, K)[0] for C in cams])
    origin, voxel, dims, trunc = bs.make_volume(side)
    tsdf, weight = surface.integrate(depth, cams, K, origin, voxel, dims, trunc)
    v, f = surface.extract(tsdf, weight, origin, voxel, min_weight=2.0)
    return v, f, images, cams, K


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=10, help="timed GPU calls")
    ap.add_argument("--warmup", type=int, default=2, help="untimed GPU calls before them")
    ap.add_argument("--size", type=int, nargs=2, default=[576, 720], metavar=("H", "W"))
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--side", type=int, default=256, help="nodes per side of the volume")
    ap.add_argument("--cpu-side", type=int, default=48)
    ap.add_argument("--no-reference", action="store_true", help="skip the CPU baseline")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "texture_bench.json"))
    a = ap.parse_args()

    import bench_surface as bs
    import dense_fixture as df
    import texture_ref as tr
    from tsbb15_amd import _ffi, surface
    if _ffi.device_count() < 1:
        raise SystemExit("bench_texture: no GPU visible")
    h, w = a.size
    v, f, images, cams, K = make_mesh(df, surface, bs, h, w, a.views, a.side)
    normals = surface.vertex_normals(v, f)
    nv, nf, V = len(v), len(f), a.views
    res = {"repeats": a.repeats, "warmup": a.warmup, "size": [h, w], "views": V,
           "side": a.side, "vertices": nv, "faces": nf, "raster_small": surface.RASTER_SMALL,
           "library": os.path.basename(os.path.dirname(_ffi.LIB_PATH)),
           "copy_bytes_per_second": COPY_RATE, "gpu": {}}
    print(f"bench_texture: {nv} vertices, {nf} faces, {V} views of {h} x {w}", flush=True)

    surface.texture_timing(1)
    call = lambda: surface.vertex_colors(v, f, images, cams, K, normals=normals)
    for _ in range(a.warmup):
        col, cnt = call()
    wall, kern = [], {k: [] for k in surface.TEXTURE_STAGES}
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        col, cnt = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms = surface.texture_timing(1)
        for k in kern:
            kern[k].append(ms[k])
    raster = float(np.median(np.add(kern["raster_small"], kern["raster_large"]))) * 1e-3
    gather = float(np.median(kern["gather"])) * 1e-3
    need = gather_bytes(nv, V, h, w, 1)
    g = res["gpu"]
    for k in kern:
        g[k] = {"kernel_ms": stats(kern[k])}
    g["raster_small"]["face_views_per_second"] = float(f"{nf * V / raster:.4e}")
    g["raster_small"]["face_views"] = nf * V
    g["gather"].update({"vertex_views": nv * V,
                        "vertex_views_per_second": float(f"{nv * V / gather:.4e}"),
                        "bytes": need, "bytes_per_second": float(f"{need / gather:.4e}"),
                        "copy_rate_fraction": round(need / gather / COPY_RATE, 4)})
    g["vertex_colors"] = {"wall_ms": stats(wall), "coloured_vertices": int((cnt > 0).sum()),
                          "mean_views_per_vertex": round(float(cnt.mean()), 3)}
    wall = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        z = surface.render_depth(v, f, cams, K, (h, w))
        wall.append((time.perf_counter() - t0) * 1e3)
    g["render_depth"] = {"wall_ms": stats(wall),
                         "covered_pixel_share": round(float((~np.isnan(z)).mean()), 4)}
    for k, val in g.items():
        print(f"bench_texture: {k} {val}", flush=True)

    if not a.no_reference:
        cv, cf, ci, cc, cK = make_mesh(df, surface, bs, 72, 90, 4, a.cpu_side)
        cn = surface.vertex_normals(cv, cf)
        t0 = time.perf_counter()
        rz = tr.render_depth(cv, cf, cK @ cc, (72, 90))
        t1 = time.perf_counter()
        rcol, rcnt, _ = tr.vertex_colors(cv, cf, ci, cK @ cc, normals=cn, depth=rz)
        t2 = time.perf_counter()
        gcol, gcnt, gz = surface.vertex_colors(cv, cf, ci, cc, cK, normals=cn, return_depth=True)
        both = ~np.isnan(rz) & ~np.isnan(gz)
        res["cpu"] = {"side": a.cpu_side, "views": 4, "size": [72, 90], "vertices": len(cv),
                      "faces": len(cf), "render_seconds": round(t1 - t0, 4),
                      "cpu_face_views_per_second": float(f"{len(cf) * 4 / (t1 - t0):.4e}"),
                      "gather_seconds": round(t2 - t1, 4),
                      "cpu_vertex_views_per_second": float(f"{len(cv) * 4 / (t2 - t1):.4e}"),
                      "mask_equal": bool(np.array_equal(np.isnan(rz), np.isnan(gz))),
                      "depth_max_diff": float(f"{np.abs(rz[both] - gz[both]).max():.3e}"),
                      "counts_differ": int((rcnt != gcnt).sum()),
                      "colour_max_diff_same_count": float(
                          f"{np.abs(rcol - gcol)[rcnt == gcnt].max():.3e}")}
        print(f"bench_texture: cpu {res['cpu']}", flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
