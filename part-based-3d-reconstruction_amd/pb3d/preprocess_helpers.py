"""The two normalisation helpers of the reference's utils/preprocess_helpers.py that its evaluation code calls (the file itself is
missing upstream; utils/eval_helpers.py:11 imports normalize_preserve_aspect from it).  Host NumPy, dtype-preserving: a float32 cloud
is normalised in float32, as NumPy's own promotion rules (NEP 50) do with the Python constants below.

normalize_preserve_aspect maps a cloud into the unit cube with one scale for all three axes, then shifts the y column so that its
maximum is exactly 0: y ends in [-1, 0] (-1 itself only where scale + 1e-8 rounds to scale).  pb3d.eval_helpers.pointcloud_to_voxel_grid evaluates the same expressions on the device
(csrc/density.hip).  The ICP and SfM preprocessing of that file is not mirrored."""
import numpy as np

__all__ = ["normalize_preserve_aspect", "flip_y_axis"]


def normalize_preserve_aspect(points):
    pts = np.asarray(points)
    min_val = pts.min(0)
    size = pts.max(0) - min_val
    scale = size.max()
    norm = (pts - min_val) / (scale + 1e-8)
    norm[:, 1] -= norm[:, 1].max()
    return norm


def flip_y_axis(coords):
    c = np.array(coords, copy=True)
    y = c[:, 1]
    c[:, 1] = y.max() - (y - y.min())
    return c
