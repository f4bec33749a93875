"""compute_triangle_normals, compute_vertex_normals and compute_surface_metrics (reference utils/eval_helpers.py:198-245) on the
device: pb3d_knn_dev (csrc/nn.hip) and csrc/surface.hip, against fixtures captured from the reference's own functions
(tools/gen_golden_surface.py) and the NumPy restatements in tests/surface_restate.py.

Parity bars
  k-NN      indices equal a NumPy brute force sorted by (squared distance as computed, index); distances bit for bit its sqrt.
  normals   array_equal with the reference's arrays, float32 and float64.
  metrics   not bit-exact by nature (BLAS dot in the vertex dtype, pairwise sums, LAPACK's SVD, libm's acos on the reference's
            side).  The yardstick is the reference's own rounding error against the same quantities in np.longdouble from the same
            neighbour sets and the same dtype-rounded normals:  e_ref = max_i |reference_i - extended_i| / scale_i,  scale = 1 degree
            (angle spread), lambda_1 of the vertex (roughness), d(k) of the vertex (curvature).  Required of the device:
            max_i |device_i - extended_i| / scale_i <= 4 e_ref on the float64 fixtures and <= e_ref on the float32 ones.
            Recorded e_ref (tests/golden/surface_ref.json; std, roughness, curvature):
              height_f64   5.3e-12  1.8e-18  8.1e-15        sphere_f64   1.1e-11  2.9e-17  1.9e-15
              height_f32   1.8e-03  1.2e-09  4.5e-06        flat_f64     2.0e-12  0        8.8e-15
              mc_f32       2.3e-03  3.6e-07  3.2e-06
The fixtures are comparable with the reference at all only because every vertex has d(k+1) > d(k) (sklearn breaks ties by traversal
order): test_fixtures_have_no_tie_at_k re-asserts the relative gap >= 1e-9 for every vertex by brute force."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import surface_restate as sr  # noqa: E402

import pb3d  # noqa: E402
from pb3d import eval_helpers as eh  # noqa: E402

META = json.load(open(os.path.join(GOLD, "surface_ref.json"), encoding="utf-8"))
K = META["k"]
FIXTURES = list(META["fixtures"])
KEYS = ("Normal StdDev (°)", "Mean Roughness (λ₃)", "Mean Curvature")
TAGS = ("std", "rough", "curv")
KS = (1, 2, 7, 20, 32)


def fixture(name):
    with np.load(os.path.join(GOLD, f"surface_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def synth_clouds():
    with np.load(os.path.join(GOLD, "inter_synth.npz")) as z:
        return [(n, z[f"{n}_q"], z[f"{n}_r"]) for n in ("lattice", "clusters", "flat")]


def scales(fx):
    return np.ones(len(fx["vertices"])), fx["scale_lambda1"], fx["scale_dk"]


def stored_grid(name):
    with np.load(os.path.join(GOLD, f"stored_{name}_voxel_grid.npz")) as z:
        return z["voxel_grid"]


# ---- CPU: the conditions the GPU checks rest on --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_have_no_tie_at_k(name):
    """every vertex, none left out: (d(k+1) - d(k)) / d(k) >= 1e-9"""
    fx = fixture(name)
    gaps, dk = sr.relative_gaps(fx["vertices"], K)
    print(name, "smallest relative gap", gaps.min())
    assert (gaps >= META["min_gap_required"]).all()
    assert META["fixtures"][name]["share_excluded"] == 0
    assert np.array_equal(dk, fx["scale_dk"])


def test_bruteforce_restatement_equals_sklearn():
    """the brute force's distances are bit for bit NearestNeighbors(20).kneighbors on tied clouds; on the gap-checked fixtures its
    index sets are sklearn's too"""
    nbrs = pytest.importorskip("sklearn.neighbors")
    for name, q, r in synth_clouds():
        for Q, R in ((q, r), (r, r), (q.astype(np.float32), r.astype(np.float32))):
            d2, _ = sr.brute_knn(Q, R, 20)
            want = nbrs.NearestNeighbors(n_neighbors=20).fit(R).kneighbors(Q)[0]
            assert np.array_equal(np.sqrt(d2), want), name
    for name in FIXTURES:
        v = fixture(name)["vertices"]
        d2, idx = sr.brute_knn(v, v, K)
        want_d, want_i = nbrs.NearestNeighbors(n_neighbors=K).fit(v).kneighbors(v)
        assert np.array_equal(np.sqrt(d2), want_d), name
        assert np.array_equal(np.sort(idx, 1), np.sort(want_i, 1)), name


@pytest.mark.parametrize("name", FIXTURES)
def test_scalar_restatement_equals_reference_normals(name):
    """the operation order csrc/surface.hip follows, one rounded operation at a time, is the reference's: bit for bit"""
    fx = fixture(name)
    v, f = fx["vertices"], fx["faces"].astype(np.int64)
    assert np.array_equal(sr.triangle_normals_scalar(v, f), fx["triangle_normals"])
    got = sr.vertex_normals_scalar(v, f)
    assert got.dtype == v.dtype and np.array_equal(got, fx["vertex_normals"])


@pytest.mark.parametrize("name", ["height_f64", "sphere_f64", "mc_f32"])
def test_float64_restatement_within_yardstick(name):
    """tests/surface_restate.py in float64 (what the tied-input check compares the device with) meets the device's own bound"""
    fx = fixture(name)
    v = fx["vertices"]
    _, idx = sr.brute_knn(v, v, K)
    std, lam, curv = sr.surface_metrics_restate(v, fx["vertex_normals"], idx)
    mult = 4.0 if v.dtype == np.float64 else 1.0
    for tag, got, scale in zip(TAGS, (std, lam[:, 0], curv), scales(fx)):
        e = sr.error_over_scale(got, fx[f"ext_{tag}_hi"], fx[f"ext_{tag}_lo"], scale)
        print(name, tag, e, META["fixtures"][name]["e_ref"][tag])
        assert e <= mult * META["fixtures"][name]["e_ref"][tag]


def test_argument_errors_before_device_work(monkeypatch):
    from pb3d import _lib
    monkeypatch.setattr(_lib, "ctx", lambda: (_ for _ in ()).throw(AssertionError("device touched")))
    v = np.random.default_rng(0).uniform(0, 1, (10, 3))
    f = np.array([[0, 1, 2], [2, 3, 4]])
    with pytest.raises(ValueError, match="Expected n_neighbors <= n_samples_fit"):
        pb3d.compute_surface_metrics(v, f, k=11)
    with pytest.raises(ValueError, match="Expected n_neighbors <= n_samples_fit"):
        pb3d.knn(v, v[:4], 5)
    for bad in (0, -3, 33):
        with pytest.raises(ValueError, match="k must be in"):
            pb3d.knn(v, v, bad)
        with pytest.raises(ValueError, match="k must be in"):
            pb3d.surface_metrics_per_vertex(v, f, k=bad)
    with pytest.raises(ValueError, match="n_components=3"):
        pb3d.compute_surface_metrics(v, f, k=2)
    with pytest.raises(TypeError):
        pb3d.knn(v, v, 2.0)
    for bad in (np.nan, np.inf):
        w = v.copy()
        w[3, 1] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            pb3d.compute_surface_metrics(w, f, k=5)
        with pytest.raises(ValueError, match="NaN or infinity"):
            pb3d.knn(v, w, 2)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        pb3d.compute_vertex_normals(v[:, :2], f)
    with pytest.raises(ValueError, match=r"\(m, 3\)"):
        pb3d.compute_triangle_normals(v, f[:, :2])
    with pytest.raises(IndexError):
        pb3d.compute_triangle_normals(v, f.astype(np.float64))
    with pytest.raises(IndexError):
        pb3d.compute_vertex_normals(v, np.array([[0, 1, 2**63 + 5]], np.uint64))
    with pytest.raises(TypeError):
        pb3d.compute_vertex_normals(v.astype(complex), f)


def test_c_entries_refuse_bad_arguments():
    """argument checks come before any device work (and before the context is looked at)"""
    from pb3d import _lib
    lib = _lib.load()
    fake, out = C.c_void_p(0x1000), C.c_void_p(0x2000)

    def knn(q=fake, nq=4, r=fake, nr=40, k=20, d=out, i=out):
        return lib.pb3d_knn_dev(None, q, 1, nq, r, 0, nr, k, d, i)

    for kw, msg in (({"k": 0}, b"k must be in [1, 32]"), ({"k": 33}, b"k must be in [1, 32]"), ({"nq": -1}, b"negative"),
                    ({"nr": 19}, b"at least k"), ({"q": None}, b"null buffer"), ({"r": None}, b"null buffer"), ({"i": None}, b"null buffer"),
                    ({"nr": 1 << 31}, b"2^31 - 1"), ({}, b"null context"), ({"d": None}, b"null context")):
        assert knn(**kw) == -1, kw
        assert msg in lib.pb3d_last_error(), (kw, lib.pb3d_last_error())
    assert knn(nq=0, q=None) == 0

    for fn in (lib.pb3d_triangle_normals_dev, lib.pb3d_vertex_normals_dev):
        for args, msg in (((fake, 0, -1, fake, 0, 4, out), b"negative"), ((fake, 0, 8, fake, 0, -4, out), b"negative"),
                          ((None, 0, 8, fake, 0, 4, out), b"null buffer"), ((fake, 0, 8, None, 0, 4, out), b"null buffer"),
                          ((fake, 0, 8, fake, 0, 4, None), b"null buffer"), ((fake, 1, 1 << 31, fake, 1, 4, out), b"2^31 - 1"),
                          ((fake, 1, 8, fake, 1, 4, out), b"null context")):
            assert fn(None, *args) == -1, args
            assert msg in lib.pb3d_last_error(), (args, lib.pb3d_last_error())

    def met(v=fake, n=fake, nv=50, idx=fake, k=20, a=out, b=out, c=out):
        return lib.pb3d_surface_metrics_dev(None, v, n, 1, nv, idx, k, a, b, c)

    for kw, msg in (({"k": 1}, b"k must be in [2, 32]"), ({"k": 33}, b"k must be in [2, 32]"), ({"nv": -1}, b"0 <= nv"),
                    ({"n": None}, b"null buffer"), ({"idx": None}, b"null buffer"), ({"b": None}, b"null buffer"), ({}, b"null context")):
        assert met(**kw) == -1, kw
        assert msg in lib.pb3d_last_error(), (kw, lib.pb3d_last_error())
    assert met(nv=0, v=None) == 0


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
def check_knn(Q, R, ks=KS):
    """pb3d.knn(Q, R, k) against the brute force, for every k at once (the brute force's first k columns)"""
    d2, idx = sr.brute_knn(Q, R, max(ks))
    for k in ks:
        if k > len(R):
            continue
        gd, gi = pb3d.knn(Q, R, k)
        assert gi.dtype == np.int32 and gd.dtype == np.float64 and gi.shape == gd.shape == (len(Q), k)
        assert np.array_equal(gi, idx[:, :k]), k
        assert np.array_equal(gd, np.sqrt(d2[:, :k])), k
        if k <= 2:
            assert np.array_equal(gd[:, k - 1], pb3d.nn_distances(Q, R, k)), k


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cloud", ["lattice", "clusters", "flat"])
def test_knn_tied_clouds(cloud, dtype):
    """lattice sites with duplicates (ties at every k), clusters with far outliers, a flat cloud: queries = set and queries != set"""
    q, r = next((q, r) for n, q, r in synth_clouds() if n == cloud)
    q, r = q.astype(dtype), r.astype(dtype)
    check_knn(r, r)
    check_knn(q, r)
    check_knn(r.astype(np.float64), r)      # mixed precisions of the two lists, both ways
    check_knn(q.astype(np.float32), r.astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_knn_fixture_meshes(name):
    v = fixture(name)["vertices"]
    check_knn(v, v)
    check_knn((v[::3] + v.dtype.type(0.37)).astype(v.dtype), v)
    if v.dtype == np.float64:
        check_knn(v.astype(np.float32), v.astype(np.float32), ks=(20,))


@pytest.mark.gpu
def test_knn_small_and_degenerate_sets():
    rng = np.random.default_rng(5)
    one = np.repeat(rng.uniform(-1, 1, (1, 3)), 40, 0)      # 40 copies of one point: every distance 0, rows 0..k-1
    check_knn(one, one)
    check_knn(one, one, ks=(8, 9, 21))                      # the last k of the 8-slot list, the first of the 20- and 32-slot lists
    line = np.zeros((70, 3))
    line[:, 1] = np.arange(70) // 2                         # duplicates on a line: two one-cell axes
    check_knn(line, line)
    check_knn(line, line, ks=(8, 9, 21))
    check_knn(rng.uniform(-5, 5, (33, 3)), line)
    few = rng.uniform(0, 1, (7, 3))
    check_knn(rng.uniform(-1, 2, (50, 3)), few, ks=(1, 2, 7))
    d, i = pb3d.knn(np.zeros((0, 3)), few, 3)
    assert d.shape == i.shape == (0, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_normals_equal_reference(name):
    fx = fixture(name)
    v = fx["vertices"]
    for faces in (fx["faces"], fx["faces"].astype(np.int64), fx["faces"].astype(np.uint16 if len(v) < 65536 else np.uint32)):
        tn = pb3d.compute_triangle_normals(v, faces)
        vn = pb3d.compute_vertex_normals(v, faces)
        assert tn.dtype == v.dtype and vn.dtype == v.dtype
        assert np.array_equal(tn, fx["triangle_normals"])
        assert np.array_equal(vn, fx["vertex_normals"])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_normals_special_meshes(dtype):
    """a 3000-face fan round one vertex with the faces in shuffled order, a face that names a vertex twice, vertices in no face,
    negative indices: equal to the scalar restatement (which test_scalar_restatement_equals_reference_normals pins to the reference)"""
    rng = np.random.default_rng(17)
    n = 3000
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rim = np.stack([np.cos(ang), np.sin(ang), rng.uniform(-0.3, 0.3, n)], 1)
    v = np.concatenate([[[0.0, 0.0, 0.5]], rim, rng.uniform(-1, 1, (5, 3))]).astype(dtype)     # the last 5: in no face
    fan = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], 1)
    fan = fan[rng.permutation(n)]
    faces = np.concatenate([fan, [[7, 7, 9], [4, 5, 4], [11, 11, 11]]])          # repeated vertices: added twice, and a zero normal
    neg = faces.copy()
    neg[::2] -= len(v)                                                           # NumPy's wrap-around
    want_t, want_v = sr.triangle_normals_scalar(v, faces), sr.vertex_normals_scalar(v, faces)
    assert not want_v[-5:].any()
    for f in (faces, neg):
        assert np.array_equal(pb3d.compute_triangle_normals(v, f), want_t)
        assert np.array_equal(pb3d.compute_vertex_normals(v, f), want_v)
    assert pb3d.compute_triangle_normals(v, np.zeros((0, 3), np.int64)).shape == (0, 3)
    assert not pb3d.compute_vertex_normals(v, np.zeros((0, 3), np.int64)).any()


@pytest.mark.gpu
def test_face_index_out_of_range_raises_and_device_stays_usable():
    fx = fixture("flat_f64")
    v, f = fx["vertices"], fx["faces"].astype(np.int64)
    for bad in (len(v), -len(v) - 1, 2**40):
        g = f.copy()
        g[len(g) // 2, 1] = bad
        for fn in (pb3d.compute_triangle_normals, pb3d.compute_vertex_normals, pb3d.compute_surface_metrics):
            with pytest.raises(IndexError):
                fn(v, g)
            assert np.array_equal(pb3d.compute_vertex_normals(v, f), fx["vertex_normals"])      # a following call succeeds
    g = fx["faces"].copy()
    g[0, 0] = len(v)
    with pytest.raises(IndexError):
        pb3d.compute_vertex_normals(v, g.astype(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_metrics_within_reference_rounding_error(name):
    """max_i |device_i - extended_i| / scale_i <= 4 e_ref (float64 fixtures), <= e_ref (float32 fixtures); the returned dict to the
    same bound, on the mean scale, against the recorded reference dict"""
    fx = fixture(name)
    v, f = fx["vertices"], fx["faces"]
    m = META["fixtures"][name]
    mult = 4.0 if v.dtype == np.float64 else 1.0
    got = pb3d.surface_metrics_per_vertex(v, f, k=K)
    res = pb3d.compute_surface_metrics(v, f, k=K)
    assert tuple(res) == KEYS
    for tag, key, g, scale in zip(TAGS, KEYS, got, scales(fx)):
        assert g.dtype == np.float64 and g.shape == (len(v),)
        e = sr.error_over_scale(g, fx[f"ext_{tag}_hi"], fx[f"ext_{tag}_lo"], scale)
        e_dict = abs(float(res[key]) - float.fromhex(m["result"][key])) / float(np.mean(scale))
        print(name, tag, "device", e, "dict", e_dict, "e_ref", m["e_ref"][tag])
        assert e <= mult * m["e_ref"][tag]
        assert e_dict <= mult * m["e_ref"][tag]
        assert res[key] == np.mean(g)
    assert (got[1] >= 0).all()


@pytest.mark.gpu
def test_tied_real_mesh_equals_brute_force_and_is_deterministic():
    """the unjittered mesh of the stored Akbar grid at stride 2 (15 722 vertices on a half-integer lattice: ties at almost every
    k-th neighbour; the reference is not comparable).  Indices equal the brute force under the tie rule; the per-vertex metrics
    equal the float64 restatement fed the BRUTE-FORCE rows within the largest recorded e_ref per metric; two runs give the same bits."""
    grid = stored_grid("Akbar")
    v, f = pb3d.meshify_colored_voxel_grid(grid, stride=2)[:2]
    assert v.dtype == np.float32 and len(v) <= 20000
    d2, idx = sr.brute_knn(v, v, K + 1, chunk=256)
    tied = (d2[:, K] == d2[:, K - 1]).mean()
    print("vertices", len(v), "share with d(k+1) == d(k):", tied)
    assert tied > 0.5
    gd, gi = pb3d.knn(v, v, K)
    assert np.array_equal(gi, idx[:, :K]) and np.array_equal(gd, np.sqrt(d2[:, :K]))

    vn = sr.vertex_normals_scalar(v, f.astype(np.int64))
    assert np.array_equal(pb3d.compute_vertex_normals(v, f), vn)
    std, lam, curv = sr.surface_metrics_restate(v, vn, idx[:, :K])
    first = pb3d.surface_metrics_per_vertex(v, f, k=K)
    bound = {t: max(m["e_ref"][t] for m in META["fixtures"].values()) for t in TAGS}
    for tag, g, want, scale in zip(TAGS, first, (std, lam[:, 0], curv), (np.ones(len(v)), lam[:, 2], np.sqrt(d2[:, K - 1]))):
        e = float((np.abs(g - want) / scale).max())
        print(tag, e, "bound", bound[tag])
        assert e <= bound[tag]
    second = pb3d.surface_metrics_per_vertex(v, f, k=K)
    gd2, gi2 = pb3d.knn(v, v, K)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    assert np.array_equal(gi, gi2) and np.array_equal(gd, gd2)


@pytest.mark.gpu
def test_resident_chain_equals_numpy_api():
    """grid handle -> mesh -> metrics without downloading the vertices: the same bits as the NumPy API"""
    from pb3d import device as dev
    grid = stored_grid("Akbar")
    d_grid = dev.DeviceGrid(dev.from_numpy(grid), grid.shape)
    bufs = [d_grid]
    try:
        (dv, df, dn, dc), (nv, nf) = dev.meshify(d_grid, grid.shape, stride=2, download=False)
        bufs += [dv, df, dn, dc]
        d_out = eh.surface_metrics_resident(dv, nv, df, nf, k=K)
        bufs.append(d_out)
        got = d_out.download((3, nv), np.float64)
        d_dist, d_idx = eh.knn_resident(dv, nv, dv, nv, 7, False, False)
        bufs += [d_dist, d_idx]
        gd, gi = d_dist.download((nv, 7), np.float64), d_idx.download((nv, 7), np.int32)
    finally:
        for b in bufs:
            b.free()
    v, f = pb3d.meshify_colored_voxel_grid(grid, stride=2)[:2]
    want = pb3d.surface_metrics_per_vertex(v, f, k=K)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    wd, wi = pb3d.knn(v, v, 7)
    assert np.array_equal(gd, wd) and np.array_equal(gi, wi)


@pytest.mark.gpu
def test_taj_stride1_mesh_completes():
    """scale, once: the ~759 000-vertex mesh of the stored Taj grid through the NumPy API (times: profiles/surface_opbench.jsonl)"""
    v, f = pb3d.meshify_colored_voxel_grid(stored_grid("Taj"), stride=1)[:2]
    res = pb3d.compute_surface_metrics(v, f)
    print(len(v), res)
    assert tuple(res) == KEYS and all(np.isfinite(x) for x in res.values())
