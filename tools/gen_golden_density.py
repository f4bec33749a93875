"""Fixtures of the density volume (reference utils/eval_helpers.py:178-189): tests/golden/density_*.npz.

Runs the reference's own pointcloud_to_voxel_grid (through tools/ref_import.py's stubs) with utils.preprocess_helpers stood in by
pb3d.preprocess_helpers -- the file is missing upstream, and the mirror states its arithmetic -- on small clouds, and records the
points, grid_size, sigma and the float32 volume the reference returned.  So the counts are np.add.at's and the smoothing is the real
scipy.ndimage.gaussian_filter.  Nothing of the reference's text is copied.

Every fixture is asserted equal, bit for bit, to tests/density_restate.py before it is written.  G <= 33, compressed.
Run: python tools/gen_golden_density.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "part-based-3d-reconstruction_amd"))

import ref_import  # noqa: E402
import density_restate as dr  # noqa: E402

# name: (cloud, grid_size, sigma)
CASES = {
    "cubic_f32_g16": (lambda: dr.make_cloud("cubic", 4097, np.float32, 1), 16, 1.0),
    "cubic_f64_g33": (lambda: dr.make_cloud("cubic", 4097, np.float64, 2), 33, 0.7),
    "flat_f64_g8": (lambda: dr.make_cloud("flat_y", 65, np.float64, 3), 8, 1.0),
    "tall_f32_g32": (lambda: dr.make_cloud("tall_y", 2000, np.float32, 4), 32, 2.5),
    "tall_f64_g7_wide": (lambda: dr.make_cloud("tall_y", 63, np.float64, 5), 7, 2.0),          # radius 8 > 7
    "cubic_f32_g5_wide": (lambda: dr.make_cloud("cubic", 64, np.float32, 6), 5, 1.5),          # radius 6 > 5
    "cubic_f64_g16_raw": (lambda: dr.make_cloud("cubic", 4097, np.float64, 7), 16, 0.0),       # no filter
    "one_voxel_f32_g8": (lambda: dr.one_voxel_cloud(3000, np.float32), 8, 1.0),
    "tall_f32_g2": (lambda: dr.make_cloud("tall_y", 20, np.float32, 8), 2, 1.0),               # all faces
    "cubic_f64_g1": (lambda: dr.make_cloud("cubic", 5, np.float64, 9), 1, 1.0),
    "ints_g8": (lambda: np.random.default_rng(10).integers(-40, 90, (300, 3)), 8, 1.0),        # int64 -> float64 arithmetic
}


def main():
    ref_import.load_reference()
    from pb3d import preprocess_helpers as mirror
    ref_import._stub("utils.preprocess_helpers", normalize_preserve_aspect=mirror.normalize_preserve_aspect, flip_y_axis=mirror.flip_y_axis)
    import utils.eval_helpers as eh

    for name, (make, G, sigma) in CASES.items():
        pts = make()
        keep = pts.copy()
        vol = eh.pointcloud_to_voxel_grid(pts, grid_size=G, sigma=sigma)
        assert np.array_equal(pts, keep) and vol.dtype == np.float32 and vol.shape == (G, G, G)
        mine = dr.voxel_grid_restate(pts, G, sigma)
        assert np.array_equal(mine.view(np.uint32), vol.view(np.uint32)), name
        np.savez_compressed(os.path.join(GOLDEN, f"density_{name}.npz"), points=pts, grid_size=np.int64(G), sigma=np.float64(sigma),
                            expected=vol)
        print(f"{name}: n = {len(pts)} {pts.dtype}, G = {G}, sigma = {sigma}, sum = {float(vol.sum()):.3f}, max = {float(vol.max()):.3f}",
              file=sys.stderr)


if __name__ == "__main__":
    main()
