#!/usr/bin/env python
"""Is the 12-parameter bundle adjustment (tsbb15_amd.tables.bundle_adjust) bytewise what another
build of the library computes?

    RSAMD_LIB=<parent build>/librsamd.so python tools/ba_parity12.py dump a.npz
    python tools/ba_parity12.py dump b.npz
    python tools/ba_parity12.py compare a.npz b.npz

`dump` runs bundle_adjust to convergence on the 5x40 and 7x70 problems of tests/ba_fixture.py at
sigma 5e-2 and on the reference's own problem (tests/golden/tables.npz, noisy_ba_*) with the
library RSAMD_LIB selects (default: the tree's), and writes cameras, points and the info record.
`compare` exits 0 iff every array of the two files has the same bytes.  Needs a GPU for `dump`.

`dump --rigid` runs bundle_adjust_rigid instead, from the rigid starts of
tests/ba_rigid_fixture.py on the two fixture problems (the reference's own problem has no
rotations to start from).
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tsbb15-3d-reconstruction-project_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

INFO_KEYS = ("cost_init", "cost", "lambda", "iterations", "status", "rejected")


def problems(rigid=False):
    import ba_fixture as bf
    for nC, nP in ((5, 40), (7, 70)):
        P = bf.problem(nC, nP)
        if rigid:
            import ba_rigid_fixture as rf
            c0, p0 = rf.rigid_start(P, 5e-2)
        else:
            c0, p0 = bf.start(P, 5e-2)
        yield f"{nC}x{nP}", c0, p0, P["ov"], P["op"], P["uv"]
    if rigid:
        return
    z = np.load(os.path.join(REPO, "tests", "golden", "tables.npz"))
    g = lambda k: z[f"noisy_{k}"]
    nC, nP = int(g("ba_n_views")), int(g("ba_n_points"))
    x0 = g("ba_x0")
    yield ("noisy", x0[:12 * nC].reshape(nC, 3, 4).copy(), x0[12 * nC:].reshape(nP, 3).copy(),
           g("ba_obs_view").astype(np.int32), g("ba_obs_point").astype(np.int32),
           np.ascontiguousarray(g("ba_obs_coords")[:, :2]))


def dump(path, rigid=False):
    from tsbb15_amd import _ffi
    from tsbb15_amd import tables as gt
    if _ffi.device_count() < 1:
        raise SystemExit("ba_parity12: no GPU visible")
    out = {}
    for name, c0, p0, ov, op, uv in problems(rigid):
        c, p, info = (gt.bundle_adjust_rigid if rigid else gt.bundle_adjust)(c0, p0, ov, op, uv)
        out[f"{name}_cams"], out[f"{name}_pts"] = c, p
        out[f"{name}_info"] = np.array([float(info[k]) for k in INFO_KEYS])
        print(f"ba_parity12: {name} cost {info['cost']:.17e} iterations {info['iterations']} "
              f"rejected {info['rejected']} ({_ffi.LIB_PATH})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)


def compare(a, b):
    za, zb = np.load(a), np.load(b)
    same = sorted(za.files) == sorted(zb.files)
    for k in sorted(za.files):
        eq = k in zb.files and za[k].tobytes() == zb[k].tobytes()
        same = same and eq
        print(f"ba_parity12: {k:12s} {'bytewise equal' if eq else 'DIFFERS'}")
    print(f"ba_parity12: {'all bytewise equal' if same else 'NOT equal'}")
    return 0 if same else 1


if __name__ == "__main__":
    rigid = "--rigid" in sys.argv
    if rigid:
        sys.argv.remove("--rigid")
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2], rigid)
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        raise SystemExit(__doc__)
