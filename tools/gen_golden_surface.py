"""Fixtures of the mesh regularity metrics (reference utils/eval_helpers.py:198-245): tests/golden/surface_*.npz, surface_ref.json.

Runs the reference's own compute_triangle_normals, compute_vertex_normals and compute_surface_metrics (through tools/ref_import.py's
stubs and the stand-in for utils.preprocess_helpers, as tools/gen_golden_inter.py does) on small meshes and records inputs and
outputs.  The three per-vertex lists of compute_surface_metrics are taken from the running function: its module sees NumPy through
a proxy whose `mean` notes the list it is handed before calling np.mean (the function's three lists reach np.mean in the order of
its returned dict).  Nothing of the reference's text is copied.

Meshes (a few thousand vertices each): a jittered height field (float64 and its float32 rounding), the binary-marching-cubes mesh
of the stored Akbar grid at stride 4 (tests/mesh_restate.py) with jittered vertices, a closed bumpy sphere, a flat sheet.

The reference's answer depends on sklearn's tie-breaking unless d(k+1) > d(k) at every vertex: asserted here for EVERY vertex as
(d(k+1) - d(k)) / d(k) >= 1e-9 by brute force; the smallest gap is printed and recorded.  sklearn's neighbour sets are asserted
equal to the brute force's.

Yardstick of the per-vertex quantities: the same three quantities evaluated in np.longdouble from the same neighbour sets and the
same dtype-rounded normals (tests/surface_restate.py), stored as float64 hi + lo; e_ref = max_i |reference_i - extended_i| /
scale_i with scale 1 degree / lambda_1 of the vertex / d(k) of the vertex.

Also prints and records the reference's wall time per mesh, a CPU measurement on the host that runs this tool, for scale.
Run: python tools/gen_golden_surface.py"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_import  # noqa: E402
import mesh_restate  # noqa: E402
import surface_restate as sr  # noqa: E402

K = 20
MIN_GAP = 1e-9
KEYS = ("Normal StdDev (°)", "Mean Roughness (λ₃)", "Mean Curvature")


class NumpyProxy:
    """numpy as the reference's module sees it; mean() keeps the lists it was called on"""

    def __init__(self):
        self.seen = []

    def __getattr__(self, name):
        return getattr(np, name)

    def mean(self, a, *args, **kwargs):
        if isinstance(a, list):
            self.seen.append(np.array(a))
        return np.mean(a, *args, **kwargs)


def sheet_faces(nx, ny):
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a = (i * ny + j).ravel()
    return np.concatenate([np.stack([a, a + ny, a + 1], 1), np.stack([a + 1, a + ny, a + ny + 1], 1)]).astype(np.int64)


def height_field(rng):
    nx = ny = 56
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    z = 1.5 * np.sin(x / 7.0) * np.cos(y / 9.0)
    v = np.stack([x, y, z], -1).reshape(-1, 3) + rng.uniform(-0.04, 0.04, (nx * ny, 3))
    return v, sheet_faces(nx, ny)


def flat_sheet(rng):
    nx = ny = 50
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    v = np.stack([x, y, np.full_like(x, 0.25)], -1).reshape(-1, 3)
    v[:, :2] += rng.uniform(-0.04, 0.04, (nx * ny, 2))         # in the plane: every normal stays (0, 0, 1)
    return v, sheet_faces(nx, ny)


def bumpy_sphere(rng, levels=4):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.array(v)
    r = 1.0 + 0.05 * np.sin(5 * v[:, 0]) * np.sin(4 * v[:, 1] + 1.0) * np.cos(3 * v[:, 2])
    v = v * r[:, None] * 10.0
    spacing = 10.0 * 4.0 / (2 ** levels * 2.0)
    return v + rng.uniform(-0.03, 0.03, v.shape) * spacing, np.array(f, np.int64)


def marching_cubes_mesh(rng):
    with np.load(os.path.join(GOLDEN, "stored_Akbar_voxel_grid.npz")) as z:
        grid = z["voxel_grid"]
    verts, faces = mesh_restate.meshify(grid, 4)[:2]
    v = verts.astype(np.float64) + rng.uniform(-0.12, 0.12, verts.shape)      # lattice spacing 2 (half of the stride)
    return v.astype(np.float32), faces.astype(np.int64)


def hexs(v):
    return [float(x).hex() for x in np.asarray(v, dtype=np.float64).ravel()]


def main():
    ref_import.load_reference()
    ref_import._stub("utils.preprocess_helpers", normalize_preserve_aspect=ref_import._unavailable)
    import utils.eval_helpers as eh
    from sklearn.neighbors import NearestNeighbors

    rng = np.random.default_rng(20261016)
    hv, hf = height_field(rng)
    meshes = {"height_f64": (hv, hf), "height_f32": (hv.astype(np.float32), hf), "mc_f32": marching_cubes_mesh(rng),
              "sphere_f64": bumpy_sphere(rng), "flat_f64": flat_sheet(rng)}
    meta = {"k": K, "min_gap_required": MIN_GAP, "keys": list(KEYS), "fixtures": {}}
    for name, (v, f) in meshes.items():
        gaps, dk = sr.relative_gaps(v, K)
        assert (gaps >= MIN_GAP).all(), (name, float(gaps.min()))     # every vertex: change the seed or the jitter, never this
        d2, idx = sr.brute_knn(v, v, K)
        _, sk_idx = NearestNeighbors(n_neighbors=K).fit(v).kneighbors(v)
        assert np.array_equal(np.sort(sk_idx, 1), np.sort(idx, 1)), name

        tn = eh.compute_triangle_normals(v, f)
        vn = eh.compute_vertex_normals(v, f)
        proxy, real = NumpyProxy(), eh.np
        eh.np = proxy
        try:
            t0 = time.perf_counter()
            res = eh.compute_surface_metrics(v, f, k=K)
            wall = time.perf_counter() - t0
        finally:
            eh.np = real
        assert list(res) == list(KEYS) and len(proxy.seen) == 3 and all(len(a) == len(v) for a in proxy.seen)
        ref = [np.asarray(a, np.float64) for a in proxy.seen]

        L = np.longdouble
        std, lam, curv = sr.surface_metrics_restate(v, vn, idx, L)
        ext = [std, lam[:, 0], curv]
        scale = [np.ones(len(v)), lam[:, 2].astype(np.float64), dk]
        e_ref = [float((np.abs(r.astype(L) - e) / s.astype(L)).max()) for r, e, s in zip(ref, ext, scale)]
        ext_mean = [float(np.mean(e)) for e in ext]
        arrays = {"vertices": v, "faces": f.astype(np.int32), "triangle_normals": tn, "vertex_normals": vn, "scale_lambda1": scale[1],
                  "scale_dk": dk}
        for tag, r, e in zip(("std", "rough", "curv"), ref, ext):
            arrays[f"ref_{tag}"] = r
            arrays[f"ext_{tag}_hi"], arrays[f"ext_{tag}_lo"] = sr.split_hi_lo(e)
        np.savez_compressed(os.path.join(GOLDEN, f"surface_{name}.npz"), **arrays)
        meta["fixtures"][name] = {"nverts": int(len(v)), "nfaces": int(len(f)), "dtype": str(v.dtype), "min_relative_gap": float(gaps.min()),
                                  "share_excluded": 0, "e_ref": {"std": e_ref[0], "rough": e_ref[1], "curv": e_ref[2]},
                                  "result": {key: float(res[key]).hex() for key in KEYS}, "extended_mean": hexs(ext_mean),
                                  "reference_wall_seconds_cpu": round(wall, 2)}
        print(f"{name}: {len(v)} verts, {len(f)} faces, min gap {gaps.min():.3e}, e_ref {e_ref}, reference {wall:.1f} s on the CPU",
              file=sys.stderr)
    with open(os.path.join(GOLDEN, "surface_ref.json"), "w") as fh:
        json.dump(meta, fh, indent=1, ensure_ascii=False)


if __name__ == "__main__":
    main()
