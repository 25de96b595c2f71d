"""Compare bench.py --dump-outputs directories array for array, bit for bit:
  python tools/compare_dumps.py <dir> <label0> <label1> ...   (<dir>/dump_<label>/*.npy)
prints one line per (label, array) against label0 and exits 1 on any difference."""
import os
import sys

import numpy as np


def main():
    out, labels = sys.argv[1], sys.argv[2:]
    ok = True
    for lab in labels[1:]:
        for f in ("F.npy", "inliers.npy", "record.npy"):
            a = np.load(os.path.join(out, "dump_" + labels[0], f))
            b = np.load(os.path.join(out, "dump_" + lab, f))
            eq = a.shape == b.shape and a.tobytes() == b.tobytes()
            ok &= eq
            print(f"dump {labels[0]} vs {lab}: {f} shape {a.shape} equal={eq}")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
