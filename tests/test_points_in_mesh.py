"""points_in_mesh, signed_point_to_mesh_distances and select_points_in_mesh (pb3d/inside.py, csrc/inside.hip) against the NumPy
restatement of tests/inside_restate.py, that restatement against the closed forms of its two exact cases, and the equality with
voxelize_mesh at lattice points that the shared rule exists for.  Every comparison of flags and counts is np.array_equal:
include/pb3d.h states the result to the bit, so there is no tolerance.  That every total is even is asserted only where all arithmetic
is exact (the pinned box, the integer octahedron): on float meshes the header claims "this function of the input" and no more."""
import functools

import numpy as np
import pytest

import inside_restate as ir

import pb3d
import pb3d.inside  # noqa: F401  (without the feature every test of this file fails here)

gpu = pytest.mark.gpu

BOX_SHAPE = (9, 10, 8)
BLOB_SHAPE = (12, 11, 13)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def pinned_box():
    """(lattice points, vertices, faces, the occupancy the header pins)"""
    v, f = ir.box((2, 3, 1), (6, 7, 5))
    ref = np.zeros(BOX_SHAPE, bool)
    ref[3:7, 3:7, 1:5] = True
    return frozen(ir.lattice_points(BOX_SHAPE), v, f, ref)


@functools.lru_cache(maxsize=None)
def octa():
    """(the 68 921 quarter-integer points of [-5, 5]^3, vertices, faces, restated flags, restated counts)"""
    q = ir.quarter_points(5)
    v, f = ir.octahedron((0, 0, 0), 4)
    inside, counts, _ = ir.restate(q, v, f)
    return frozen(q, v, f, inside, counts)


@functools.lru_cache(maxsize=None)
def blob_mask():
    """a random blob with an empty one-voxel border: white noise box-filtered twice along every axis, cut at its upper third"""
    x = np.random.default_rng(12).random(tuple(n - 2 for n in BLOB_SHAPE))
    for axis in range(3):
        for _ in range(2):
            x = x + np.roll(x, 1, axis) + np.roll(x, -1, axis)
    m = np.zeros(BLOB_SHAPE, bool)
    m[1:-1, 1:-1, 1:-1] = x > np.quantile(x, 0.67)
    assert 100 < m.sum() < m.size // 2
    return frozen(m)


@functools.lru_cache(maxsize=None)
def float_mesh(name, vdtype):
    """(vertices in vdtype, int64 faces) of the octahedron of radius 4 or the 320-face icosphere of radius 3, rotated"""
    v, f = ir.octahedron((0, 0, 0), 4) if name == "octahedron" else ir.icosphere(2)
    scale = 1.0 if name == "octahedron" else 3.0
    v = ((scale * v) @ ir.rotation(21).T + np.array([0.3, -0.2, 0.1])).astype(vdtype)
    return frozen(np.ascontiguousarray(v), f)


@functools.lru_cache(maxsize=None)
def float_queries(name, vdtype):
    """uniform random queries around the mesh, and queries that project onto its vertices and edge midpoints"""
    v, f = float_mesh(name, vdtype)
    uniform = np.random.default_rng(8).uniform(-4.5, 4.5, (3000, 3))
    return frozen(uniform, ir.tie_queries(v, f, seed=9))


def same(got, counts, q, v, f, what):
    """flags and counts of the device against the restatement, byte for byte"""
    ref_in, ref_counts, _ = ir.restate(q, v, f)
    assert got.dtype == np.bool_ and got.shape == ref_in.shape, (what, got.dtype, got.shape)
    if not np.array_equal(got, ref_in):
        bad = np.flatnonzero(got != ref_in)
        raise AssertionError((what, "first differing query", int(bad[0]), q[bad[0]].tolist(), "differing", len(bad), "of", len(q)))
    assert counts.dtype == np.int32 and np.array_equal(counts, ref_counts), (what, "counts")
    return ref_in, ref_counts


# ---- CPU: the restatement against its closed forms, and the argument checks ----------------------------------------------------------
def test_restatement_pinned_box():
    q, v, f, ref = pinned_box()
    inside, counts, stats = ir.restate(q, v, f)
    assert np.array_equal(inside.reshape(BOX_SHAPE), ref)
    assert not (counts[:, 1] & 1).any()
    # eight of the twelve triangles are flat in projection; the lattice points outside i 2..6, j 3..7 are outside the vertices' box
    assert stats == dict(inside=64, odd_totals=0, flat_faces=8, outside_box=720 - 5 * 5 * 8)


def test_restatement_octahedron():
    q, v, f, inside, counts = octa()
    assert len(q) == 68921
    l1 = np.abs(q).sum(axis=1)
    assert inside[l1 < 4].all() and not inside[l1 > 4].any()
    assert not (counts[:, 1] & 1).any()
    flipped, fcounts, _ = ir.restate(q, v, f[:, ::-1])
    assert np.array_equal(flipped, inside) and np.array_equal(fcounts, counts)
    on_edges = (q[:, 0] == 0) | (q[:, 1] == 0) | (np.abs(q[:, 0]) + np.abs(q[:, 1]) == 4)
    assert on_edges.sum() > 5000                       # many queries project onto the edges and vertices of the eight faces


def test_restatement_equals_voxelize_restatement():
    """the shared rule, on the CPU: at lattice points the restatement gives the voxelization's restated bytes"""
    import voxelize_restate as vr
    for name in ("pinned_box", "octahedron_box", "sphere_f32", "triangle"):
        v, f, shape, _ = vr.constructed_cases()[name]
        occ, vstats = vr.restate(v, f, shape)
        inside, counts, stats = ir.restate(ir.lattice_points(shape), v, f)
        assert np.array_equal(inside.reshape(shape), occ.astype(bool)), name
        assert stats["flat_faces"] == vstats["flat_faces"] and stats["inside"] == vstats["occupied"], name


def test_nan_query_is_outside_with_zero_counts():
    _, v, f, _ = pinned_box()
    q = np.array([[4.0, 5.0, np.nan], [np.nan, 5.0, 3.0], [4.0, np.nan, 3.0], [4.0, 5.0, 3.0], [4.0, 5.0, np.inf]])
    inside, counts, stats = ir.restate(q, v, f)
    assert inside.tolist() == [False, False, False, True, False]
    assert counts.tolist() == [[0, 0], [0, 0], [0, 0], [1, 2], [2, 2]]
    assert stats["outside_box"] == 3


def test_wall_mesh_exceeds_the_entry_cap_by_construction():
    v, f = ir.wall_among_small()
    cells, entries = ir.first_grid_entries(v, f)
    assert len(f) == 502 and cells == (16, 16) and entries > 8 * len(f)


def flattened_icosphere():
    """the float64 icosphere with every vertex at one a0: no face has a projected area"""
    flat = float_mesh("icosphere", np.float64)[0].copy()
    flat[:, 0] = 0.25
    return flat, float_mesh("icosphere", np.float64)[1]


def test_grid_entries_restates_the_listing_rule():
    v, f = ir.wall_among_small()
    cells, entries = ir.first_grid_entries(v, f)
    assert ir.grid_entries(v, f, cells) == entries
    assert ir.grid_entries(v, f, (1, 1)) == len(f)         # one cell lists every face once: none of them is flat
    flat, faces = flattened_icosphere()
    for cells in ((1, 1), (1, 13)):                         # a box without an a0 extent has one cell there
        assert ir.grid_entries(flat, faces, cells) == 0


def test_argument_errors_need_no_device():
    q, v, f, _ = pinned_box()
    for fn in (pb3d.points_in_mesh, pb3d.signed_point_to_mesh_distances, pb3d.select_points_in_mesh):
        with pytest.raises(ValueError, match=r"\(n, 3\)"):
            fn(q[:, :2], v, f)
        with pytest.raises(ValueError, match=r"\(n, 3\)"):
            fn(q, v[:, :2], f)
        with pytest.raises(ValueError, match=r"\(m, 3\)"):
            fn(q, v, f[:, :2])
        with pytest.raises(IndexError):
            fn(q, v, f.astype(np.float64))
        with pytest.raises(IndexError):
            fn(q, v, f.astype(np.uint32) + np.uint32(len(v)))
        with pytest.raises(IndexError):
            fn(q, np.zeros((0, 3)), f)
        with pytest.raises(TypeError):
            fn(q.astype(complex), v, f)
        for bad in (np.nan, np.inf, -np.inf):
            qb = q.copy()
            qb[17, 2] = bad
            with pytest.raises(ValueError, match="NaN or infinity"):
                fn(qb, v, f)
    vb = v.copy()
    vb[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        pb3d.signed_point_to_mesh_distances(q, vb, f)
    with pytest.raises(ValueError, match="no faces"):
        pb3d.signed_point_to_mesh_distances(q, v, f[:0])
    with pytest.raises(ValueError, match="at most"):
        pb3d.points_in_mesh_resident(None, 2 ** 31, None, 8, None, 12)
    # no queries: nothing needs the device
    assert pb3d.points_in_mesh(q[:0], v, f).shape == (0,)
    inside, counts = pb3d.points_in_mesh(q[:0], v, f, return_counts=True)
    assert inside.dtype == np.bool_ and counts.shape == (0, 2) and counts.dtype == np.int32
    assert pb3d.signed_point_to_mesh_distances(q[:0], v, f).shape == (0,)
    pts, idx = pb3d.select_points_in_mesh(q[:0].astype(np.float32), v, f, return_index=True)
    assert pts.shape == (0, 3) and pts.dtype == np.float32 and idx.shape == (0,)


def test_exports():
    import re
    from conftest import ROOT
    header = open(ROOT + "/include/pb3d.h").read()
    for n in ("points_in_mesh", "signed_point_to_mesh_distances", "select_points_in_mesh"):
        assert callable(getattr(pb3d, n)) and callable(getattr(pb3d, n + "_resident"))
        assert n in pb3d.inside.__all__ and n + "_resident" in pb3d.inside.__all__
    for s in ("pb3d_points_in_mesh_resident", "pb3d_points_in_mesh_last", "pb3d_mesh_dist_sign_resident", "pb3d_flags_not_resident"):
        assert s in pb3d._lib.EXPORTED_SYMBOLS and re.search(r"^int\s+" + s + r"\s*\(", header, re.M)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def run(pb, q, v, f, what):
    inside, counts = pb.points_in_mesh(q, v, f, return_counts=True)
    return (inside, counts) + same(inside, counts, q, v, f, what)


@gpu
def test_pinned_box(pb3d_gpu):
    q, v, f, ref = pinned_box()
    for qd, vd, fd in ((np.float64, np.float64, np.int64), (np.float32, np.float32, np.int32)):
        inside, counts, _, _ = run(pb3d_gpu, q.astype(qd), v.astype(vd), f.astype(fd), "pinned box")
        assert np.array_equal(inside.reshape(BOX_SHAPE), ref)
        assert np.array_equal(inside.reshape(BOX_SHAPE), pb3d_gpu.voxelize_mesh(v.astype(vd), f.astype(fd), BOX_SHAPE) != 0)
        assert not (counts[:, 1] & 1).any()


@gpu
def test_smoke_line(pb3d_gpu):
    """what __graft_entry__.smoke() asks: the 720 lattice points against the pinned box give that grid's occupancy"""
    q, v, f, _ = pinned_box()
    solid = pb3d_gpu.voxelize_mesh(v, f, BOX_SHAPE)
    assert np.array_equal(pb3d_gpu.points_in_mesh(np.indices(BOX_SHAPE).reshape(3, -1).T, v, f).reshape(BOX_SHAPE), solid != 0)


@gpu
def test_same_rule_as_voxelize(pb3d_gpu):
    mask = blob_mask()
    v, f = pb3d_gpu.isosurface(mask.astype(np.float32), 0.5)        # lattice order (a0, a1, a2): no frame conversion enters
    assert v.dtype == np.float32 and f.dtype == np.int32 and len(f) > 500
    q = ir.lattice_points(BLOB_SHAPE)
    inside, counts, _, _ = run(pb3d_gpu, q, v, f, "blob lattice")
    assert np.array_equal(inside.reshape(BLOB_SHAPE), mask)
    assert np.array_equal(inside.reshape(BLOB_SHAPE), pb3d_gpu.voxelize_mesh(v, f, BLOB_SHAPE) != 0)
    rng = np.random.default_rng(4)
    dyadic = q[rng.integers(0, len(q), 4000)] + rng.integers(-4, 5, (4000, 3)) / 8.0      # on and between the faces' half-integer planes
    run(pb3d_gpu, dyadic, v, f, "blob dyadic")
    run(pb3d_gpu, dyadic.astype(np.float32), v, f, "blob dyadic float32")
    run(pb3d_gpu, rng.uniform(-0.5, np.array(BLOB_SHAPE) - 0.5, (4000, 3)), v, f, "blob uniform")


@gpu
def test_ties_on_the_integer_octahedron(pb3d_gpu):
    q, v, f, ref_in, ref_counts = octa()
    inside, counts = pb3d_gpu.points_in_mesh(q, v, f, return_counts=True)
    assert np.array_equal(inside, ref_in) and np.array_equal(counts, ref_counts)
    assert not (counts[:, 1] & 1).any()
    l1 = np.abs(q).sum(axis=1)
    assert inside[l1 < 4].all() and not inside[l1 > 4].any()
    flipped, fcounts = pb3d_gpu.points_in_mesh(q.astype(np.float32), v.astype(np.float32), f[:, ::-1].astype(np.int32), return_counts=True)
    assert np.array_equal(flipped, inside) and np.array_equal(fcounts, counts)


@gpu
@pytest.mark.parametrize("fdtype", (np.int32, np.int64))
@pytest.mark.parametrize("vdtype", (np.float32, np.float64))
@pytest.mark.parametrize("name", ("octahedron", "icosphere"))
def test_float_mesh(pb3d_gpu, name, vdtype, fdtype):
    v, f = float_mesh(name, vdtype)
    uniform, ties = float_queries(name, vdtype)
    neg = np.random.default_rng(5).random(f.shape) < 0.5
    wrapped = np.where(neg, f - len(v), f).astype(fdtype)               # negative indices wrap
    assert wrapped.min() < 0 <= wrapped.max()
    inside, _, _, _ = run(pb3d_gpu, uniform, v, wrapped, (name, "uniform"))
    assert 0 < inside.sum() < len(inside)
    assert ties.dtype == vdtype
    inside, counts, _, _ = run(pb3d_gpu, ties, v, wrapped, (name, "ties"))
    assert 0 < inside.sum() < len(inside) and counts[:, 1].max() >= 2
    run(pb3d_gpu, uniform.astype(np.float32), v, f.astype(fdtype), (name, "uniform float32"))
    pb3d_gpu._lib.set_tuning("inside_table", 1)             # the same bytes from the table of finished set-ups
    try:
        run(pb3d_gpu, ties, v, wrapped, (name, "ties, set-up table"))
    finally:
        pb3d_gpu._lib.set_tuning("inside_table", 0)


@gpu
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 257))
def test_query_counts(pb3d_gpu, n):
    v, f = float_mesh("icosphere", np.float64)
    q = float_queries("icosphere", np.float64)[0][:n]
    inside, counts = pb3d_gpu.points_in_mesh(q, v, f, return_counts=True)
    assert inside.shape == (n,) and counts.shape == (n, 2)
    if n:
        same(inside, counts, q, v, f, n)


@gpu
def test_no_faces(pb3d_gpu):
    q = float_queries("icosphere", np.float64)[0][:100]
    for verts in (float_mesh("icosphere", np.float64)[0], np.zeros((0, 3), np.float32)):
        inside, counts = pb3d_gpu.points_in_mesh(q, verts, np.zeros((0, 3), np.int32), return_counts=True)
        assert not inside.any() and not counts.any() and inside.shape == (100,) and counts.shape == (100, 2)


@gpu
def test_queries_outside_the_box_on_each_side(pb3d_gpu):
    from pb3d import device as dev
    _, v, f, _ = pinned_box()
    q = np.array([[1.99, 5, 3], [6.01, 5, 3], [4, 2.99, 3], [4, 7.01, 3], [4, 5, 0.5], [4, 5, 5.5], [2, 3, 1], [6, 7, 5], [4, 5, 3],
                  [-1e300, 5, 3], [4, 1e300, 3]], np.float64)
    inside, counts, ref_in, _ = run(pb3d_gpu, q, v, f, "outside")
    assert ref_in.tolist() == [False] * 8 + [True, False, False]
    assert not counts[:4].any() and not counts[9:].any() and counts[4].tolist() == [0, 2] and counts[5].tolist() == [2, 2]
    d_q, d_v, d_f = dev.from_numpy(q), dev.from_numpy(v), dev.from_numpy(f)
    try:
        d_in, stats = pb3d_gpu.points_in_mesh_resident(d_q, len(q), d_v, len(v), d_f, len(f), verts_f64=True, faces_i64=True, return_stats=True)
        d_in.free()
        assert stats == ir.restate(q, v, f)[2] == dict(inside=1, odd_totals=0, flat_faces=8, outside_box=6)
    finally:
        for b in (d_q, d_v, d_f):
            b.free()


@gpu
def test_resident_nan_query(pb3d_gpu):
    from pb3d import device as dev
    _, v, f, _ = pinned_box()
    q = np.array([[4.0, 5.0, np.nan], [np.nan, 5.0, 3.0], [4.0, np.nan, 3.0], [4.0, 5.0, 3.0], [4.0, 5.0, np.inf]])
    ref_in, ref_counts, ref_stats = ir.restate(q, v, f)
    for order in (0, 1):                                    # input order, cell order
        d_q, d_v, d_f = dev.from_numpy(q), dev.from_numpy(v), dev.from_numpy(f)
        pb3d_gpu._lib.set_tuning("inside_order", order)
        try:
            d_in, d_cnt, stats = pb3d_gpu.points_in_mesh_resident(d_q, len(q), d_v, len(v), d_f, len(f), verts_f64=True, faces_i64=True,
                                                                  return_counts=True, return_stats=True)
            assert np.array_equal(d_in.download((5,)) != 0, ref_in) and np.array_equal(d_cnt.download((5, 2), np.int32), ref_counts)
            assert stats == ref_stats
            d_in.free()
            d_cnt.free()
        finally:
            pb3d_gpu._lib.set_tuning("inside_order", 0)
            for b in (d_q, d_v, d_f):
                b.free()


@gpu
def test_degenerate_box(pb3d_gpu):
    """every vertex shares one a0: the box has no extent there, every face is flat, nothing is inside"""
    flat, f = flattened_icosphere()
    q = np.concatenate([float_queries("icosphere", np.float64)[0][:500], np.column_stack([np.full(50, 0.25), flat[:50, 1], flat[:50, 2]])])
    inside, counts, _, _ = run(pb3d_gpu, q, flat, f, "degenerate")
    assert not inside.any() and not counts.any()
    cells, entries, _ = pb3d_gpu.points_in_mesh_last()
    assert entries == 0                                     # no face has an area: no entry
    assert entries == ir.grid_entries(flat, f, cells)


@gpu
def test_cell_without_a_face(pb3d_gpu):
    """two boxes far apart: the cells between them list nothing, and queries there walk an empty list"""
    v, f = ir.box((0, 0, 0), (1, 1, 1))
    v2 = v + np.array([9.0, 7.0, 0.0])
    verts, faces = np.concatenate([v, v2]), np.concatenate([f, f + 8])
    rng = np.random.default_rng(6)
    q = np.concatenate([rng.uniform(2, 8, (300, 3)) * (1, 1, 0.2), rng.uniform(-0.2, 1.2, (300, 3)), rng.uniform(-0.2, 1.2, (300, 3)) + (9, 7, 0)])
    inside, counts, _, _ = run(pb3d_gpu, q, verts, faces, "gap")
    assert not counts[:300].any() and inside[300:].sum() > 100
    cells, entries, _ = pb3d_gpu.points_in_mesh_last()
    assert cells[0] * cells[1] > entries                    # more cells than entries: some cell is empty
    assert entries == ir.grid_entries(verts, faces, cells)  # the listing rule, to the entry


@gpu
def test_wall_among_small_faces_coarsens_the_index(pb3d_gpu):
    v, f = ir.wall_among_small()
    cells, entries = ir.first_grid_entries(v, f)
    assert entries > 8 * len(f)                             # the first grid breaks the cap, by construction
    q = np.random.default_rng(10).uniform(-0.05, 1.05, (4000, 3))
    inside, counts, _, _ = run(pb3d_gpu, q, v, f, "wall")
    got_cells, got_entries, halvings = pb3d_gpu.points_in_mesh_last()
    assert halvings >= 1 and got_cells[0] < cells[0] and got_cells[1] < cells[1] and got_entries <= 8 * len(f)
    assert got_entries == ir.grid_entries(v, f, got_cells)  # the listing rule on the halved grid, to the entry
    assert counts[:, 1].max() >= 3 and 0 < inside.sum() < len(q)


@gpu
def test_host_waits_of_the_resident_call(pb3d_gpu):
    """the waits csrc/inside.hip's header states: the mesh check, the box, 1 + halvings entry counts, one more for the stats.  The
    outputs stay on the device inside the counted span"""
    from pb3d import device as dev
    q, v, f, _ = pinned_box()
    bufs = [dev.from_numpy(q), dev.from_numpy(v), dev.from_numpy(f)]
    try:
        for with_stats in (False, True):
            for _ in range(2):                              # the second call finds every scratch slot large enough: no wait for a regrow
                before = dev.sync_count()
                out = pb3d_gpu.points_in_mesh_resident(bufs[0], len(q), bufs[1], len(v), bufs[2], len(f), verts_f64=True, faces_i64=True,
                                                       return_stats=with_stats)
                waits = dev.sync_count() - before
                bufs.append(out[0] if with_stats else out)
            halvings = pb3d_gpu.points_in_mesh_last()[2]
            print("host waits of the resident call:", waits, "halvings", halvings, "stats", with_stats)
            assert waits == 3 + halvings + with_stats
    finally:
        for b in bufs:
            b.free()


@gpu
def test_errors_leave_the_outputs_untouched(pb3d_gpu):
    from pb3d import device as dev
    q, v, f, _ = pinned_box()
    n = len(q)
    cases = []
    for bad in (len(v), -len(v) - 1):
        fb = f.astype(np.int32)
        fb[7, 1] = bad
        cases.append((v.astype(np.float32), fb, IndexError))
    for bad in (np.nan, np.inf, -np.inf):
        vb = v.astype(np.float32)
        vb[5, 2] = bad
        cases.append((vb, f.astype(np.int32), ValueError))
    for vb, fb, error in cases:
        d_q, d_v, d_f = dev.from_numpy(q), dev.from_numpy(vb), dev.from_numpy(fb)
        d_out, d_cnt = dev.from_numpy(np.full(n, 0xAB, np.uint8)), dev.from_numpy(np.full(2 * n, 0x5A5A5A5A, np.int32))
        try:
            with pytest.raises(error):
                pb3d_gpu.points_in_mesh_resident(d_q, n, d_v, len(vb), d_f, len(fb), return_counts=True, return_stats=True, out=d_out,
                                                 counts_out=d_cnt)
            assert np.array_equal(d_out.download((n,)), np.full(n, 0xAB, np.uint8))
            assert np.array_equal(d_cnt.download((2 * n,), np.int32), np.full(2 * n, 0x5A5A5A5A, np.int32))
        finally:
            for b in (d_q, d_v, d_f, d_out, d_cnt):
                b.free()
        with pytest.raises(error):
            pb3d_gpu.points_in_mesh(q, vb, fb)
        with pytest.raises(error):
            pb3d_gpu.select_points_in_mesh(q, vb, fb)
    qb = q.copy()
    qb[3, 0] = np.nan
    with pytest.raises(ValueError):
        pb3d_gpu.points_in_mesh(qb, v, f)


@gpu
def test_signed_distance(pb3d_gpu):
    v, f = ir.icosphere(2)
    rin = ir.inradius(v, f)
    assert 0.9 < rin < 1.0
    rng = np.random.default_rng(13)
    q = np.concatenate([rng.uniform(-1.3, 1.3, (3000, 3)), v[:40], (v[f[:40, 0]] + v[f[:40, 1]] + v[f[:40, 2]]) / 3.0])
    d, face, closest = pb3d_gpu.point_to_mesh_distances(q, v, f, return_faces=True, return_closest=True)
    inside = pb3d_gpu.points_in_mesh(q, v, f)
    sd, sface, sclosest, sinside = pb3d_gpu.signed_point_to_mesh_distances(q, v, f, return_faces=True, return_closest=True, return_inside=True)
    assert sd.dtype == np.float64 and np.array_equal(sd, np.where(inside & (d > 0), -d, d))
    assert np.array_equal(sinside, inside) and np.array_equal(sface, face) and np.array_equal(sclosest, closest)
    assert np.array_equal(pb3d_gpu.signed_point_to_mesh_distances(q, v, f), sd)
    r = np.linalg.norm(q, axis=1)
    assert (sd[r < rin] < 0).all() and (r < rin).sum() > 500 and (sd[r > 1] > 0).all() and (r > 1).sum() > 500
    on = d == 0                                            # the vertices themselves: on the surface, +0.0 whatever the flag says
    assert on.sum() >= 40 and not np.signbit(sd[on]).any()
    # float32 cloud and mesh, int32 faces: the same composition
    q32, v32, f32 = q.astype(np.float32), v.astype(np.float32), f.astype(np.int32)
    d32, in32 = pb3d_gpu.point_to_mesh_distances(q32, v32, f32), pb3d_gpu.points_in_mesh(q32, v32, f32)
    assert np.array_equal(pb3d_gpu.signed_point_to_mesh_distances(q32, v32, f32), np.where(in32 & (d32 > 0), -d32, d32))


@gpu
def test_selection(pb3d_gpu):
    from pb3d import device as dev
    v, f = float_mesh("icosphere", np.float32)
    for q in (float_queries("icosphere", np.float32)[0], float_queries("icosphere", np.float32)[0].astype(np.float32)):
        inside = ir.restate(q, v, f)[0]
        assert 0 < inside.sum() < len(q)
        kept, idx = pb3d_gpu.select_points_in_mesh(q, v, f, return_index=True)
        assert kept.dtype == q.dtype and np.array_equal(kept, q[inside]) and np.array_equal(idx, np.flatnonzero(inside))
        assert np.array_equal(pb3d_gpu.select_points_in_mesh(q, v, f), q[inside])
        out, idx = pb3d_gpu.select_points_in_mesh(q, v, f, invert=True, return_index=True)
        assert np.array_equal(out, q[~inside]) and np.array_equal(idx, np.flatnonzero(~inside))
        d_q, d_v, d_f = dev.from_numpy(q), dev.from_numpy(v), dev.from_numpy(f)
        try:
            for invert, keep in ((False, inside), (True, ~inside)):
                d_out, d_idx, count = pb3d_gpu.select_points_in_mesh_resident(d_q, len(q), d_v, len(v), d_f, len(f), invert,
                                                                              p_f64=q.dtype == np.float64, faces_i64=True)
                assert count == keep.sum()
                assert d_out.download((count, 3), q.dtype).tobytes() == q[keep].tobytes()
                assert np.array_equal(d_idx.download((count,), np.int32), np.flatnonzero(keep))
                d_out.free()
                d_idx.free()
            assert np.array_equal(d_q.download(q.shape, q.dtype), q)       # the cloud stays as it was
        finally:
            for b in (d_q, d_v, d_f):
                b.free()


@gpu
def test_two_runs_and_every_launch_shape_give_equal_bytes(pb3d_gpu):
    """queries in input order and in cell order (knob inside_order), set-ups recomputed and read from a table (knob inside_table),
    each twice"""
    v, f = ir.wall_among_small()
    q = np.random.default_rng(14).uniform(-0.05, 1.05, (5000, 3))
    runs = []
    try:
        for order, table in ((0, 0), (0, 0), (1, 0), (1, 0), (0, 1), (0, 1), (1, 1)):
            pb3d_gpu._lib.set_tuning("inside_order", order)
            pb3d_gpu._lib.set_tuning("inside_table", table)
            inside, counts = pb3d_gpu.points_in_mesh(q, v, f, return_counts=True)
            runs.append(inside.tobytes() + counts.tobytes())
    finally:
        pb3d_gpu._lib.set_tuning("inside_order", 0)
        pb3d_gpu._lib.set_tuning("inside_table", 0)
    assert len(set(runs)) == 1
    same(inside, counts, q, v, f, "orders")


@gpu
def test_timing_knob(pb3d_gpu):
    q, v, f, ref = pinned_box()
    with pytest.raises(ValueError, match="not timed"):
        pb3d_gpu.points_in_mesh(q, v, f)
        pb3d_gpu.points_in_mesh_last(timed=True)
    pb3d_gpu._lib.set_tuning("inside_timing", 1)
    try:
        inside = pb3d_gpu.points_in_mesh(q, v, f)
        cells, entries, halvings, ms = pb3d_gpu.points_in_mesh_last(timed=True)
    finally:
        pb3d_gpu._lib.set_tuning("inside_timing", 0)
    assert np.array_equal(inside.reshape(BOX_SHAPE), ref) and entries >= 4 and ms[0] > 0 and ms[1] > 0
