"""The inter-method metrics (reference utils/eval_helpers.py) and the exact nearest-neighbour search under them (csrc/nn.hip).

tests/golden/inter_ref.json holds the reference's outputs (float.hex) for seeded calls on a 20 000-point sample of the SfM cloud and
the Taj grid's occupied voxels mapped into its box (tools/gen_golden_inter.py); the GPU tests rebuild every input from the fixtures and
must reproduce each output exactly, and the global RNG state the reference leaves behind.  The search itself is checked bit for bit
against cKDTree on clouds built to break a grid search: ties, duplicates, clusters with far outliers, flat clouds, large offsets,
queries far outside the reference box, float32 and float64, and a 2 M x 1 M case."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _meta():
    with open(os.path.join(GOLDEN, "inter_ref.json")) as f:
        return json.load(f)


def _synth():
    with np.load(os.path.join(GOLDEN, "inter_synth.npz")) as f:
        return {k: f[k] for k in f.files}


def _sfm():
    with np.load(os.path.join(GOLDEN, "inter_sfm20k.npz")) as f:
        return f["sfm"]


_TAJ = {}


def _taj():
    if "p" not in _TAJ:
        t = _meta()["taj_transform"]
        with np.load(os.path.join(GOLDEN, "stored_Taj_voxel_grid.npz")) as f:
            grid = f["voxel_grid"]
        idx = np.argwhere(np.any(grid != 0, axis=-1))
        _TAJ["p"] = idx * float.fromhex(t["scale"]) + np.array([float.fromhex(v) for v in t["offset"]])
        assert len(_TAJ["p"]) == t["points"]
    return _TAJ["p"]


def _clouds():
    taj, sfm = _taj(), _sfm()
    return {"taj": taj, "sfm": sfm, "taj_f32": taj.astype(np.float32), "sfm_f32": sfm.astype(np.float32)}


def _unhex(v):
    if isinstance(v, list):
        return [_unhex(x) for x in v]
    if isinstance(v, dict):
        return {k: _unhex(x) for k, x in v.items()}
    return float.fromhex(v)


def brute_knn(q, r, k=1):
    """the k-th smallest sqrt((dx*dx + dy*dy) + dz*dz) from each row of q to the rows of r, in float64 (float32 widened first)"""
    q = np.asarray(q, np.float64)
    r = np.asarray(r, np.float64)
    dx = q[:, None, 0] - r[None, :, 0]
    dy = q[:, None, 1] - r[None, :, 1]
    dz = q[:, None, 2] - r[None, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    return np.sqrt(np.sort(d2, axis=1)[:, k - 1])


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["lattice", "clusters", "flat"])
def test_bruteforce_restatement_equals_ckdtree(case):
    from scipy.spatial import cKDTree
    s = _synth()
    q, r = s[case + "_q"], s[case + "_r"]
    assert np.array_equal(brute_knn(q, r), cKDTree(r).query(q, k=1)[0])
    assert np.array_equal(brute_knn(r, r, 2), cKDTree(r).query(r, k=2)[0][:, 1])
    q32, r32 = q.astype(np.float32), r.astype(np.float32)
    assert np.array_equal(brute_knn(q32, r32), cKDTree(r32).query(q32, k=1)[0])


def test_f1_curve_from_distances_reproduces_reference():
    from scipy.spatial import cKDTree
    import pb3d
    s = _synth()
    g = _meta()["f1_curve_from_distances"]
    dq = cKDTree(s["clusters_r"]).query(s["clusters_q"], k=1)[0]
    dr = cKDTree(s["clusters_q"]).query(s["clusters_r"], k=1)[0]
    got = pb3d.f1_curve_from_distances(dq, dr, np.linspace(0.0, 0.5, 50))
    for a, b in zip(got, _unhex(g["result"])):
        assert a.tolist() == b


def test_filter_mesh_reproduces_reference():
    import pb3d
    s = _synth()
    g = _meta()["filter_mesh"]
    v, f = pb3d.filter_mesh(s["mesh_vertices"], s["mesh_faces"], y_thresh=g["y_thresh"])
    assert v.ravel().tolist() == _unhex(g["vertices"])
    assert f.ravel().tolist() == g["faces"]


def test_pca_shape_similarity_reproduces_reference():
    import pb3d
    cl = _clouds()
    for c in _meta()["calls"]:
        if c["name"] == "pca_shape_similarity":
            np.random.seed(c["seed"])
            got = pb3d.pca_shape_similarity(*[cl[a] for a in c["args"]])
            assert abs(got - float.fromhex(c["result"])) <= 1e-12
            assert float(np.random.random()).hex() == c["rng_after"]


def test_install_rebinds_reference_eval_helpers():
    import sys
    import pb3d
    pkg = types.ModuleType("ref_utils_i5")
    pkg.__path__ = []
    mod = types.ModuleType("ref_utils_i5.eval_helpers")
    for n in ("chamfer_distance", "voxel_iou", "compute_nn_stats", "compute_f1_curve", "filter_mesh"):
        setattr(mod, n, lambda *a, **k: None)
    sys.modules["ref_utils_i5"], sys.modules["ref_utils_i5.eval_helpers"] = pkg, mod
    try:
        patched = pb3d.install(pkg)
    finally:
        del sys.modules["ref_utils_i5"], sys.modules["ref_utils_i5.eval_helpers"]
    assert mod.chamfer_distance is pb3d.chamfer_distance and mod.voxel_iou is pb3d.voxel_iou
    assert mod.compute_f1_curve is pb3d.compute_f1_curve and mod.filter_mesh is pb3d.filter_mesh
    assert ("ref_utils_i5.eval_helpers", "compute_nn_stats") in patched


def test_new_entries_refuse_bad_arguments():
    """argument checks come before any device work (and before the context is looked at)"""
    from pb3d import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x1000)
    out = C.c_void_p(0x2000)

    def nn(q, nq, r, nr, k, o=out):
        return lib.pb3d_nn_dist_dev(None, q, 1, nq, r, 1, nr, k, o)

    for args, msg in (((fake, 4, fake, 4, 3), b"k must be 1 or 2"), ((fake, 4, fake, 4, 0), b"k must be 1 or 2"),
                      ((fake, -1, fake, 4, 1), b"negative"), ((fake, 4, fake, -4, 1), b"negative"),
                      ((fake, 4, fake, 0, 1), b"at least k"), ((fake, 4, fake, 1, 2), b"at least k"),
                      ((None, 4, fake, 4, 1), b"null buffer"), ((fake, 4, None, 4, 1), b"null buffer"),
                      ((fake, 1 << 31, fake, 4, 1), b"2^31 - 1"), ((fake, 4, fake, 4, 1), b"null context")):
        assert nn(*args) == -1, args
        assert msg in lib.pb3d_last_error(), (args, lib.pb3d_last_error())
    assert nn(fake, 4, fake, 4, 1, None) == -1 and b"null buffer" in lib.pb3d_last_error()
    assert nn(fake, 0, None, 0, 1) == 0          # nothing to do

    assert lib.pb3d_points_bounds_dev(None, fake, 1, 0, out) == -1 and b"1 <= n" in lib.pb3d_last_error()
    assert lib.pb3d_points_bounds_dev(None, None, 1, 5, out) == -1 and b"null buffer" in lib.pb3d_last_error()
    assert lib.pb3d_points_bounds_dev(None, fake, 1, 5, out) == -1 and b"null context" in lib.pb3d_last_error()

    lo = np.zeros(3)

    def iou(na=5, nb=5, res=8, iters=1, a=fake, b=fake, lo_=lo, f32=0, af=1, bf=1):
        return lib.pb3d_voxel_iou_counts_dev(None, a, af, na, b, bf, nb, None if lo_ is None else _lib.p_dbl(lo_), 0.5, f32, res, iters, out)

    for kw, msg in (({"res": 0}, b"resolution"), ({"res": 4096}, b"resolution"), ({"iters": -1}, b"iters"), ({"na": -1}, b"negative"),
                    ({"a": None}, b"null buffer"), ({"b": None}, b"null buffer"), ({"lo_": None}, b"null buffer"),
                    ({"f32": 1}, b"float32 points"), ({"nb": 1 << 31}, b"2^31 - 1"), ({}, b"null context")):
        assert iou(**kw) == -1, kw
        assert msg in lib.pb3d_last_error(), (kw, lib.pb3d_last_error())
    assert iou(a=None, na=0, f32=1, af=0, bf=0) == -1 and b"null context" in lib.pb3d_last_error()

    cells = (C.c_int64 * 3)()
    b = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 2.0])
    assert lib.pb3d_nn_grid_shape(_lib.p_dbl(b), 20000, cells) == 0
    assert cells[1] == 1 and cells[0] * cells[1] * cells[2] <= 20000        # the flat axis gets one cell
    assert lib.pb3d_nn_grid_shape(_lib.p_dbl(b), 0, cells) == -1


# ---- GPU: the search against cKDTree --------------------------------------------------------------------------------------------------
def _nn_case(name, rng):
    if name == "uniform":
        return rng.uniform(-1, 1, (5000, 3)), rng.uniform(-1, 1, (3001, 3))
    if name == "clusters_outliers":
        r = np.concatenate([rng.normal(0, 1e-3, (2000, 3)) + c for c in rng.uniform(-1, 1, (5, 3))] + [rng.uniform(-500, 500, (37, 3))])
        q = np.concatenate([rng.normal(0, 0.3, (3000, 3)), rng.uniform(-900, 900, (300, 3))])
        return q, r
    if name == "lattice_ties":
        return rng.integers(-2, 12, (4000, 3)).astype(np.float64), rng.integers(0, 10, (3000, 3)).astype(np.float64)
    if name == "identical":
        return rng.uniform(-1, 1, (777, 3)), np.tile(np.array([[0.5, -0.25, 3.0]]), (129, 1))
    if name == "one_query":
        return rng.uniform(-1, 1, (1, 3)), rng.uniform(-1, 1, (1000, 3))
    if name == "one_reference":
        return rng.uniform(-1, 1, (1000, 3)), rng.uniform(-1, 1, (1, 3))
    if name == "one_one":
        return rng.uniform(-1, 1, (1, 3)), rng.uniform(-1, 1, (1, 3))
    if name == "odd_counts":
        return rng.uniform(0, 1, (65, 3)), rng.uniform(0, 1, (127, 3))
    if name == "flat":
        r = np.column_stack([rng.uniform(0, 1, 4000), np.full(4000, 0.75), rng.uniform(0, 3, 4000)])
        return rng.uniform(-0.5, 3.5, (3000, 3)), r
    if name == "line":
        r = np.column_stack([np.full(3000, -2.0), rng.uniform(0, 5, 3000), np.full(3000, 1.0)])
        return rng.uniform(-3, 6, (2000, 3)), r
    if name == "offset_1e6":
        return rng.uniform(-1, 1, (4000, 3)) + 1e6, rng.uniform(-1, 1, (3000, 3)) + 1e6
    if name == "far_queries":
        r = rng.uniform(0, 1, (5000, 3))
        q = np.concatenate([rng.uniform(0, 1, (500, 3)), rng.normal(0, 1, (1500, 3)) * 1e4, rng.uniform(1e3, 2e3, (200, 3))])
        return q, r
    raise KeyError(name)


NN_CASES = ["uniform", "clusters_outliers", "lattice_ties", "identical", "one_query", "one_reference", "one_one", "odd_counts", "flat",
            "line", "offset_1e6", "far_queries"]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", NN_CASES)
def test_nn_dist_bitexact_vs_ckdtree(pb3d_gpu, case, dtype):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(NN_CASES.index(case))
    q, r = _nn_case(case, rng)
    q, r = q.astype(dtype), r.astype(dtype)
    got = pb3d_gpu.nn_distances(q, r)
    assert got.dtype == np.float64 and got.shape == (len(q),)
    want = cKDTree(r).query(q, k=1)[0]
    assert np.array_equal(got, want), (case, np.flatnonzero(got != want)[:10])
    if len(r) >= 2:
        got2 = pb3d_gpu.nn_distances(r, r, k=2)
        assert np.array_equal(got2, cKDTree(r).query(r, k=2)[0][:, 1]), case
        got2q = pb3d_gpu.nn_distances(q, r, k=2)
        assert np.array_equal(got2q, cKDTree(r).query(q, k=2)[0][:, 1]), case


@pytest.mark.gpu
def test_nn_dist_mixed_precision_and_resident(pb3d_gpu):
    from scipy.spatial import cKDTree
    from pb3d import device as dev
    from pb3d.eval_helpers import nn_distances_resident, points_bounds_resident
    rng = np.random.default_rng(5)
    q = rng.normal(0, 1, (3333, 3)).astype(np.float32)
    r = rng.normal(0, 1, (2222, 3))
    assert np.array_equal(pb3d_gpu.nn_distances(q, r), cKDTree(r).query(q, k=1)[0])
    assert np.array_equal(pb3d_gpu.nn_distances(r, q), cKDTree(q).query(r, k=1)[0])
    d_q, d_r = dev.from_numpy(q), dev.from_numpy(r)
    d_o = nn_distances_resident(d_q, len(q), d_r, len(r), 1, a_f64=False, b_f64=True)
    assert np.array_equal(d_o.download((len(q),), np.float64), cKDTree(r).query(q, k=1)[0])
    bb = points_bounds_resident(d_q, len(q), f64=False).download((6,), np.float64)
    assert np.array_equal(bb, np.concatenate([q.min(0), q.max(0)]).astype(np.float64))
    for b in (d_q, d_r, d_o):
        b.free()


@pytest.mark.gpu
def test_nn_dist_large_bitexact(pb3d_gpu):
    """>= 2 M queries against >= 1 M references, both directions of the k = 1 search and the k = 2 self-query"""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(2024)
    r = np.concatenate([rng.uniform(0, 10, (900_000, 3)), rng.normal(5, 0.05, (148_577, 3))])
    q = np.concatenate([rng.uniform(-1, 11, (2_000_000, 3)), rng.normal(5, 0.5, (3_211, 3))])
    tree = cKDTree(r)
    assert np.array_equal(pb3d_gpu.nn_distances(q, r), tree.query(q, k=1, workers=16)[0])
    assert np.array_equal(pb3d_gpu.nn_distances(r, r, k=2), tree.query(r, k=2, workers=16)[0][:, 1])


@pytest.mark.gpu
def test_nn_dist_sqrt_is_correctly_rounded(pb3d_gpu):
    """one reference point at the origin: the distance of (x, y, 0) is sqrt(x*x + y*y), for squares across many binades"""
    rng = np.random.default_rng(9)
    q = np.column_stack([rng.uniform(0, 1, 200_000) * 10.0 ** rng.integers(-150, 150, 200_000),
                         rng.uniform(0, 1, 200_000) * 10.0 ** rng.integers(-150, 150, 200_000), np.zeros(200_000)])
    got = pb3d_gpu.nn_distances(q, np.zeros((1, 3)))
    assert np.array_equal(got, np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]))


# ---- GPU: the public functions reproduce the reference's recorded outputs ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(_meta()["calls"])))
def test_reference_outputs_reproduced(pb3d_gpu, i):
    c = _meta()["calls"][i]
    cl = _clouds()
    args = [cl[a] if a in cl else np.linspace(0.0, 0.2, 50) for a in c["args"]]
    np.random.seed(c["seed"])
    got = getattr(pb3d_gpu, c["name"])(*args, **c["kwargs"])
    want = _unhex(c["result"])
    if c["name"] == "pca_shape_similarity":
        assert abs(got - want) <= 1e-12
    elif c["name"] == "compute_nn_stats":
        assert {k: float(v) for k, v in got.items()} == want
    elif c["name"] == "compute_f1_curve":
        assert [a.tolist() for a in got] == want
    elif c["name"] == "fscore_with_threshold":
        assert list(got) == want
    else:
        assert got == want, (c, got, want)
    assert float(np.random.random()).hex() == c["rng_after"], "global RNG state differs from the reference's"


# ---- GPU: voxel_iou counts against the SciPy dilation ---------------------------------------------------------------------------------------
def _iou_counts_restated(A, B, resolution, dilate_frac):
    """reference eval_helpers.py:83-111 returning (inter, union)"""
    from scipy.ndimage import binary_dilation
    all_pts = np.vstack([A, B])
    bounds_min, bounds_max = all_pts.min(0), all_pts.max(0)
    step = (bounds_max - bounds_min).max() / resolution

    def to_occ(points):
        idx = ((points - bounds_min) / step).astype(int)
        idx = np.clip(idx, 0, resolution - 1)
        occ = np.zeros((resolution,) * 3, dtype=bool)
        occ[idx[:, 0], idx[:, 1], idx[:, 2]] = True
        return occ

    occA, occB = to_occ(A), to_occ(B)
    if dilate_frac > 0:
        iters = max(1, int(round((dilate_frac * np.linalg.norm(bounds_max - bounds_min)) / step)))
        occA = binary_dilation(occA, iterations=iters)
        occB = binary_dilation(occB, iterations=iters)
    return int(np.count_nonzero(occA & occB)), int(np.count_nonzero(occA | occB)), iters if dilate_frac > 0 else 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f64", "f32", "int", "mixed"])
@pytest.mark.parametrize("res,frac", [(31, 0.1), (47, 0.07), (64, 0.0), (33, 0.02), (5, 0.5)])
def test_voxel_iou_counts_match_binary_dilation(pb3d_gpu, kind, res, frac):
    from pb3d.eval_helpers import voxel_iou_counts
    rng = np.random.default_rng(res * 7 + int(frac * 100))
    A = np.concatenate([rng.normal(0, 1, (3000, 3)), rng.uniform(-4, 4, (50, 3))])
    B = np.concatenate([rng.normal(0.3, 0.8, (2500, 3)) * [1, 2, 0.5], rng.uniform(-3, 5, (40, 3))])
    if kind == "f32":
        A, B = A.astype(np.float32), B.astype(np.float32)
    elif kind == "int":
        A, B = np.round(A * 100).astype(np.int64), np.round(B * 37).astype(np.int32)
    elif kind == "mixed":
        A = A.astype(np.float32)
    inter, union, iters = _iou_counts_restated(A, B, res, frac)
    if (res, frac) in ((31, 0.1), (47, 0.07)):
        assert iters >= 3          # odd resolutions, several dilation passes
    assert voxel_iou_counts(A, B, res, frac) == (inter, union), (kind, res, frac)
    assert pb3d_gpu.voxel_iou(A, B, res, frac) == inter / union


@pytest.mark.gpu
def test_voxel_iou_single_point_and_one_empty_cloud(pb3d_gpu):
    from pb3d.eval_helpers import voxel_iou_counts
    A = np.array([[1.0, 2.0, 3.0]])
    with np.errstate(invalid="ignore", divide="ignore"):
        inter, union, _ = _iou_counts_restated(A, A, 9, 0.0)
        assert voxel_iou_counts(A, A, 9, 0.0) == (inter, union)
    B = np.random.default_rng(1).uniform(0, 1, (500, 3))
    E = np.zeros((0, 3))
    assert voxel_iou_counts(B, E, 21, 0.1) == _iou_counts_restated(B, E, 21, 0.1)[:2]
