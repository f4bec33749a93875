"""Fixtures of the inter-method metrics (row I5, reference utils/eval_helpers.py): tests/golden/inter_*.

Runs the reference's own eval_helpers (through tools/ref_import.py's stubs, plus a stand-in for utils.preprocess_helpers, which is
missing upstream) and records every output as float.hex, with the seed set before each call and the first np.random.random() drawn
after it (the global RNG state the call leaves).  Inputs the tests rebuild from the fixtures alone:
  - inter_sfm20k.npz: 20 000 points of results/4.Inter-method_3D/segmented_point_cloud_final.ply (float64 xyz, fixed seed);
  - the Taj grid's occupied voxels (tests/golden/stored_Taj_voxel_grid.npz, np.argwhere order) mapped into the SfM box by
    p = idx * scale + offset (float64, stated in the JSON);
  - inter_synth.npz: small synthetic clouds for the edge cases (lattice ties and duplicates, clusters with outliers, a flat cloud).
Run: python tools/gen_golden_inter.py  (minutes: cKDTree on the full 12 M-point Taj cloud)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, HERE)

import ref_import  # noqa: E402

PLY = os.path.join(ref_import.REFERENCE_ROOT, "results", "4.Inter-method_3D", "segmented_point_cloud_final.ply")
SAMPLE_SEED = 20251016


def load_reference_eval_helpers():
    ref_import.load_reference()
    ref_import._stub("utils.preprocess_helpers", normalize_preserve_aspect=ref_import._unavailable)
    import utils.eval_helpers as eh
    return eh


def read_ply_xyz(path):
    raw = open(path, "rb").read()
    head = raw[:raw.index(b"end_header\n") + len(b"end_header\n")]
    assert b"binary_little_endian" in head and b"property double x" in head
    dt = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    v = np.frombuffer(raw[len(head):], dt)
    return np.stack([v["x"], v["y"], v["z"]], 1)


def taj_points(scale, offset):
    with np.load(os.path.join(GOLDEN, "stored_Taj_voxel_grid.npz")) as f:
        grid = f["voxel_grid"]
    idx = np.argwhere(np.any(grid != 0, axis=-1))
    return idx * scale + offset


def synth_clouds():
    rng = np.random.default_rng(7)
    lat = rng.integers(0, 6, (900, 3)).astype(np.float64)                 # 216 lattice sites: ties and duplicates
    lat_q = rng.integers(-1, 7, (700, 3)).astype(np.float64)
    clu = np.concatenate([rng.normal(0, 0.01, (600, 3)) + c for c in rng.uniform(-1, 1, (4, 3))] + [rng.uniform(-40, 40, (20, 3))])
    clu_q = np.concatenate([rng.normal(0, 0.05, (900, 3)), rng.uniform(-60, 60, (40, 3))])
    flat = np.column_stack([rng.uniform(0, 1, 1000), np.full(1000, 0.25), rng.uniform(0, 2, 1000)])
    flat_q = rng.uniform(-0.5, 2.5, (800, 3))
    return {"lattice_r": lat, "lattice_q": lat_q, "clusters_r": clu, "clusters_q": clu_q, "flat_r": flat, "flat_q": flat_q}


def synth_mesh():
    rng = np.random.default_rng(11)
    verts = rng.uniform(-1, 1, (300, 3))
    faces = rng.integers(0, 300, (500, 3))
    return verts, faces


def hexs(v):
    return [float(x).hex() for x in np.asarray(v, dtype=np.float64).ravel()]


def main():
    eh = load_reference_eval_helpers()
    from scipy.spatial import cKDTree

    xyz = read_ply_xyz(PLY)
    rng = np.random.default_rng(SAMPLE_SEED)
    sfm = xyz[np.sort(rng.choice(len(xyz), 20000, replace=False))]
    lo = sfm.min(0)
    scale = float((sfm.max(0) - lo).max() / 511.0)
    offset = lo.copy()
    taj = taj_points(scale, offset)
    print("taj points:", len(taj), file=sys.stderr)

    synth = synth_clouds()
    verts, faces = synth_mesh()
    np.savez_compressed(os.path.join(GOLDEN, "inter_sfm20k.npz"), sfm=sfm)
    np.savez_compressed(os.path.join(GOLDEN, "inter_synth.npz"), mesh_vertices=verts, mesh_faces=faces, **synth)

    calls = []

    def record(name, fn, args, kwargs, seed, out):
        np.random.seed(seed)
        r = fn(*args, **kwargs)
        after = float(np.random.random()).hex()
        calls.append({"name": name, "seed": seed, "args": out["args"], "kwargs": out.get("kwargs", {}), "result": out["conv"](r),
                      "rng_after": after})
        print(name, out["args"], out.get("kwargs"), file=sys.stderr)

    clouds = {"taj": taj, "sfm": sfm, "taj_f32": taj.astype(np.float32), "sfm_f32": sfm.astype(np.float32)}
    C = lambda *names: [clouds[n] for n in names]      # noqa: E731
    scalar = lambda r: float(r).hex()                   # noqa: E731
    tup = lambda r: [float(v).hex() for v in r]         # noqa: E731
    stats = lambda r: {k: float(v).hex() for k, v in r.items()}    # noqa: E731
    curve = lambda r: [hexs(a) for a in r]              # noqa: E731

    record("chamfer_distance", eh.chamfer_distance, C("taj", "sfm"), {}, 1, {"args": ["taj", "sfm"], "conv": scalar})
    record("chamfer_distance", eh.chamfer_distance, C("taj", "sfm"), {"squared": False}, 2,
           {"args": ["taj", "sfm"], "kwargs": {"squared": False}, "conv": scalar})
    record("chamfer_distance", eh.chamfer_distance, C("sfm", "taj"), {"max_points": 13_000_000}, 3,
           {"args": ["sfm", "taj"], "kwargs": {"max_points": 13_000_000}, "conv": scalar})
    for seed, tau in ((4, 0.01), (5, 0.03), (6, 0.1)):
        record("fscore_with_threshold", eh.fscore_with_threshold, C("taj", "sfm"), {"tau": tau}, seed,
               {"args": ["taj", "sfm"], "kwargs": {"tau": tau}, "conv": tup})
    record("compute_nn_stats", eh.compute_nn_stats, C("taj"), {}, 7, {"args": ["taj"], "conv": stats})
    record("compute_nn_stats", eh.compute_nn_stats, C("sfm_f32"), {}, 8, {"args": ["sfm_f32"], "conv": stats})
    thr = np.linspace(0.0, 0.2, 50)
    record("compute_f1_curve", eh.compute_f1_curve, C("taj", "sfm") + [thr], {"seed": 3}, 9,
           {"args": ["taj", "sfm", "linspace(0, 0.2, 50)"], "kwargs": {"seed": 3}, "conv": curve})
    for seed, (res, frac) in ((10, (96, 0.01)), (11, (97, 0.03)), (12, (64, 0.0))):
        record("voxel_iou", eh.voxel_iou, C("taj", "sfm"), {"resolution": res, "dilate_frac": frac}, seed,
               {"args": ["taj", "sfm"], "kwargs": {"resolution": res, "dilate_frac": frac}, "conv": scalar})
    record("voxel_iou", eh.voxel_iou, C("taj_f32", "sfm_f32"), {"resolution": 97, "dilate_frac": 0.03}, 13,
           {"args": ["taj_f32", "sfm_f32"], "kwargs": {"resolution": 97, "dilate_frac": 0.03}, "conv": scalar})
    record("pca_shape_similarity", eh.pca_shape_similarity, C("taj", "sfm"), {}, 14, {"args": ["taj", "sfm"], "conv": scalar})

    # host-only pieces the CPU tests check: f1_curve_from_distances on cKDTree distances of the synthetic clouds, filter_mesh
    dq = cKDTree(synth["clusters_r"]).query(synth["clusters_q"], k=1)[0]
    dr = cKDTree(synth["clusters_q"]).query(synth["clusters_r"], k=1)[0]
    f1s = eh.f1_curve_from_distances(dq, dr, np.linspace(0.0, 0.5, 50))
    fv, ff = eh.filter_mesh(verts, faces, y_thresh=0.2)

    meta = {
        "sample_seed": SAMPLE_SEED, "ply_points": int(len(xyz)),
        "taj_transform": {"formula": "np.argwhere(np.any(grid != 0, axis=-1)) * scale + offset", "scale": scale.hex(),
                          "offset": hexs(offset), "points": int(len(taj))},
        "calls": calls,
        "f1_curve_from_distances": {"a": "clusters_q", "b": "clusters_r", "thresholds": "linspace(0, 0.5, 50)", "result": curve(f1s)},
        "filter_mesh": {"y_thresh": 0.2, "vertices": hexs(fv), "faces": [int(v) for v in ff.ravel()]},
    }
    with open(os.path.join(GOLDEN, "inter_ref.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
