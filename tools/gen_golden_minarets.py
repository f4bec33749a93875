"""F14: golden digests of extract_minaret_voxels_by_label (reference utils/camera_estimation.py:176-216) and
extract_top_bottom_voxel_points (:329-335) on the five stored grids with the notebook-2 minaret colours
[front_minarets, back_minarets]; captured from the live reference (THIS CONTAINER ONLY).  Writes
tests/golden/f14_minarets.json:
  {"<monument>": {"keys": [...], "parts": {"<name>": {"shape", "sha256"}}, "kps": {"<name>_bottom|_top": [float64 hex x3]}}}

The reference calls `coords[:, 1].ptp()`, which NumPy 2 removed: while it runs, np.argwhere returns a view of an ndarray
subclass whose .ptp is np.ptp (what ndarray.ptp computed under NumPy 1.x).  The shim lives here only."""
import hashlib
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MONUMENTS = ["Akbar", "Bibi", "Charminar", "Itimad", "Taj"]
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class _PtpArray(np.ndarray):
    def ptp(self, axis=None):
        return np.ptp(np.asarray(self), axis=axis)


def _case(mon):
    import ref_import
    vc, vu, pu, cg, ce, cfg = ref_import.load_reference()
    grid = np.load(os.path.join(GOLDEN, f"stored_{mon}_voxel_grid.npz"))["voxel_grid"]
    colors = [cfg.PART_COLORS["front_minarets"], cfg.PART_COLORS["back_minarets"]]
    argwhere = np.argwhere
    np.argwhere = lambda *a, **k: argwhere(*a, **k).view(_PtpArray)
    try:
        parts = ce.extract_minaret_voxels_by_label(grid, colors)
        kps = ce.extract_top_bottom_voxel_points(parts)
    finally:
        np.argwhere = argwhere
    parts = {k: np.asarray(v) for k, v in parts.items()}
    return mon, {"keys": list(parts),
                 "parts": {k: {"shape": list(v.shape), "dtype": str(v.dtype), "sha256": sha(v)} for k, v in parts.items()},
                 "kps": {k: [float(x).hex() for x in np.asarray(v, np.float64)] for k, v in kps.items()}}


def main():
    with ProcessPoolExecutor(max_workers=min(5, os.cpu_count() or 1)) as ex:
        res = dict(ex.map(_case, MONUMENTS))
    with open(os.path.join(GOLDEN, "f14_minarets.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(len(res), "monuments")


if __name__ == "__main__":
    main()
