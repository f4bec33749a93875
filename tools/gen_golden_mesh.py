"""Capture meshify_colored_voxel_grid fixtures from the reference's own function (needs scikit-image and scikit-learn: run it
under a Python that has both).  Only cv2, trimesh, ipywidgets and IPython are stood in for; skimage and sklearn are real.

Writes tests/golden/mesh_synth.npz   full outputs of small synthetic grids (keys <name>_grid, _stride, _verts, _faces, _colors, _normals)
       tests/golden/mesh_stored.npz  the five stored grids at strides 4, 2, 1: counts, sha256 of verts / faces, the
                                     reference's vertex colours as a uint8 index into the grid's unique colours; full
                                     normals at strides 4 and 2
"""
import hashlib
import json
import os
import sys
import types
import warnings

import numpy as np

warnings.filterwarnings("ignore")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REFERENCE_ROOT = "/root/reference"


def _unavailable(*a, **k):
    raise RuntimeError("stubbed third-party function called")


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__getattr__ = lambda attr: _unavailable   # any other name the reference imports
    sys.modules[name] = m
    return m


def load_meshify():
    import matplotlib
    matplotlib.use("Agg")
    _stub("cv2")
    _stub("trimesh")
    _stub("ipywidgets")
    ip = _stub("IPython", get_ipython=lambda: None, version_info=(8, 12, 3))
    ip.display = _stub("IPython.display")
    sys.path.insert(0, REFERENCE_ROOT)
    import utils.voxel_utils as vu
    return vu.meshify_colored_voxel_grid


def synth_grids():
    """(name, grid, stride) cases: every single-cube case, random densities, thin / odd shapes, strides 1-5, colours <= 1."""
    rng = np.random.default_rng(1234)
    out = []
    # all 254 non-trivial cube cases: case c's corners at a1 = 3(c-1) + {0, 1}, one empty lattice row between cases
    g = np.zeros((2, 3 * 254, 2, 3), np.uint8)
    for c in range(1, 255):
        for bit in range(8):
            if (c >> bit) & 1:
                g[(bit >> 2) & 1, 3 * (c - 1) + ((bit >> 1) & 1), bit & 1] = (37 * c % 255 + 1, 11, 200)
    out.append(("cases", g, 1))
    out.append(("cases_t", np.ascontiguousarray(g.transpose(1, 0, 2, 3)), 1))
    pal = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [200, 200, 0], [7, 9, 250]], np.uint8)
    for k, (shape, dens, s) in enumerate([((12, 10, 14), 0.5, 1), ((16, 9, 11), 0.2, 1), ((14, 12, 10), 0.8, 1),
                                           ((2, 9, 8), 0.5, 1), ((9, 2, 7), 0.4, 1), ((8, 7, 2), 0.6, 1),
                                           ((20, 12, 8), 0.5, 1), ((8, 12, 20), 0.3, 1), ((19, 17, 23), 0.5, 2),
                                           ((22, 13, 17), 0.5, 3), ((25, 21, 18), 0.4, 4), ((23, 19, 27), 0.5, 5),
                                           ((17, 11, 13), 0.5, 2), ((30, 8, 6), 0.15, 1)]):
        occ = rng.random(shape) < dens
        g = pal[rng.integers(0, len(pal), shape)] * occ[..., None]
        out.append(("rand%d" % k, g.astype(np.uint8), s))
    # colours all <= 1: the reference keeps the raw uint8 values
    occ = rng.random((11, 9, 10)) < 0.5
    g = (rng.integers(0, 2, (11, 9, 10, 3)) | np.array([1, 0, 0])) * occ[..., None]
    out.append(("small_vals", g.astype(np.uint8), 1))
    # a blob: one connected body well inside the grid (mirrored queries far from the surface)
    a = np.indices((24, 16, 20)).astype(float)
    blob = ((a[0] - 8) ** 2 / 30 + (a[1] - 8) ** 2 / 20 + (a[2] - 12) ** 2 / 25) < 1
    g = pal[rng.integers(0, len(pal), blob.shape)] * blob[..., None]
    out.append(("blob", g.astype(np.uint8), 1))
    return out


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    meshify = load_meshify()
    syn = {}
    names = []
    for name, g, s in synth_grids():
        v, f, c, n = meshify(g, stride=s)
        syn[name + "_grid"] = g
        syn[name + "_stride"] = np.int64(s)
        syn[name + "_verts"] = v
        syn[name + "_faces"] = f
        syn[name + "_colors"] = c
        syn[name + "_normals"] = n
        names.append(name)
        print(name, g.shape, s, len(v), len(f), c.dtype)
    syn["names"] = np.array(names)
    np.savez_compressed(os.path.join(GOLD, "mesh_synth.npz"), **syn)

    st, meta = {}, {}
    for mon in ["Akbar", "Taj", "Charminar", "Bibi", "Itimad"]:
        g = np.load(os.path.join(GOLD, "stored_%s_voxel_grid.npz" % mon))["voxel_grid"]
        uniq = np.unique(g.reshape(-1, 3), axis=0)
        for s in (4, 2, 1):
            v, f, c, n = meshify(g, stride=s)
            raw = np.rint(c * 255.0).astype(np.int64) if c.dtype == np.float64 else c.astype(np.int64)
            key = raw[:, 0] * 65536 + raw[:, 1] * 256 + raw[:, 2]
            ukey = uniq[:, 0].astype(np.int64) * 65536 + uniq[:, 1] * 256 + uniq[:, 2]
            idx = np.searchsorted(ukey, key)
            assert np.array_equal(ukey[idx], key)
            k = "%s_%d" % (mon, s)
            st[k + "_cidx"] = idx.astype(np.uint8)
            if s > 1:
                st[k + "_normals"] = n
            meta[k] = {"nverts": int(len(v)), "nfaces": int(len(f)), "verts_sha256": sha(v), "faces_sha256": sha(f),
                       "normals_sha256": sha(n), "verts_dtype": str(v.dtype), "faces_dtype": str(f.dtype),
                       "colors_dtype": str(c.dtype)}
            print(k, meta[k]["nverts"], meta[k]["nfaces"], flush=True)
    np.savez_compressed(os.path.join(GOLD, "mesh_stored.npz"), **st)
    with open(os.path.join(GOLD, "mesh_stored.json"), "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
