"""F13: golden digests of extract_top_k_components (reference utils/voxel_utils.py:24-33) on the five
stored grids, every part colour present, k in {4, 1, 0, -1}; captured from the live reference
(THIS CONTAINER ONLY).  Writes tests/golden/f13_top_k_components.json:
  {"<monument>/<part>/k<k>": {"sha256", "zeroed", "n26", "shape"}}
The reference is slow on the large grids (a full-grid argwhere per component), so the cases run in a
process pool."""
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
KS = [4, 1, 0, -1]
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _grid(mon):
    return np.load(os.path.join(GOLDEN, f"stored_{mon}_voxel_grid.npz"))["voxel_grid"]


def _case(args):
    mon, part, k = args
    import ref_import
    from scipy.ndimage import label
    vc, vu, pu, cg, ce, cfg = ref_import.load_reference()
    grid = _grid(mon)
    color = cfg.PART_COLORS[part]
    out = vu.extract_top_k_components(grid, color, k=k)
    mask = np.all(grid == color, axis=-1)
    _, n26 = label(mask, structure=np.ones((3, 3, 3)))
    zeroed = int(np.count_nonzero(mask & np.all(out == 0, axis=-1)))
    return f"{mon}/{part}/k{k}", {"sha256": sha(out), "zeroed": zeroed, "n26": int(n26), "shape": list(out.shape)}


def main():
    import ref_import
    cfg = ref_import.load_reference()[5]
    cases = []
    for mon in MONUMENTS:
        g = _grid(mon)
        present = set(map(tuple, np.unique(g.reshape(-1, 3), axis=0).tolist()))
        for part, col in cfg.PART_COLORS.items():
            if tuple(col) in present:
                cases += [(mon, part, k) for k in KS]
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        res = dict(ex.map(_case, cases))
    res = {key: res[key] for key in sorted(res)}
    with open(os.path.join(GOLDEN, "f13_top_k_components.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(len(res), "cases")


if __name__ == "__main__":
    main()
