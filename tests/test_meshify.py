"""meshify_colored_voxel_grid (reference utils/voxel_utils.py:53-96): binary marching cubes and nearest-filled-voxel colours on
the device (csrc/mesh.hip), against fixtures captured from the reference's own function (tools/gen_golden_mesh.py, scikit-image
0.18.3 / scikit-learn 0.24.2) and the NumPy restatement in tests/mesh_restate.py.

Parity bar: verts, faces and normals bit-exact.  Against the reference's fixtures, colours equal the reference's wherever the
nearest occupied voxel is unique or all tied voxels share a colour, and one of the tied voxels' colours otherwise (scikit-learn's
tie choice is not a contract).  Against the restatement, which breaks ties as include/pb3d.h publishes (the smallest lattice
index), colours are equal, dtype included.  tests/test_meshify_pinned.py holds the constructed cases."""
import hashlib
import json
import os
import re
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import mesh_restate as mr  # noqa: E402

STORED = ["Akbar", "Taj", "Charminar", "Bibi", "Itimad"]


def synth():
    z = np.load(os.path.join(GOLD, "mesh_synth.npz"))
    return [(str(n), z[f"{n}_grid"], int(z[f"{n}_stride"]), z[f"{n}_verts"], z[f"{n}_faces"], z[f"{n}_colors"], z[f"{n}_normals"])
            for n in z["names"]]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def check_colors(grid, stride, verts, got, want):
    """got may differ from want only where the nearest occupied lattice voxel is tied between different colours, and then must
    be one of the tied voxels' colours"""
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = np.where(np.any(got != want, axis=1))[0]
    if not len(bad):
        return 0
    g = grid[::stride, ::stride, ::stride]
    mask = np.any(g > 0, axis=-1)
    _, ties = mr.nearest_filled(mask, mr.queries(verts[bad], stride))
    flatcols = g.reshape(-1, g.shape[-1])
    for i, t in zip(bad, ties):
        cands = flatcols[t]
        cands = cands / 255.0 if got.dtype == np.float64 else cands
        assert len(np.unique(flatcols[t], axis=0)) > 1, f"vertex {i}: unique nearest colour differs"
        assert np.any(np.all(cands == got[i], axis=1)), f"vertex {i}: colour is none of the tied voxels'"
    return len(bad)


# ---- CPU: the restatement and the table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", synth(), ids=lambda c: c[0])
def test_restatement_reproduces_reference(case):
    name, grid, s, v, f, c, n = case
    rv, rf, rc, rn = mr.meshify(grid, s)
    assert rv.dtype == v.dtype == np.float32 and rf.dtype == f.dtype == np.int32
    assert np.array_equal(rv, v) and np.array_equal(rf, f)
    assert np.array_equal(rn, n) and rn.dtype == n.dtype
    check_colors(grid, s, v, rc, c)


def test_table_inc_matches_json():
    inc = open(os.path.join(HERE, "..", "part-based-3d-reconstruction_amd", "csrc", "mc_binary_table.inc")).read()
    body = lambda name: [int(x) for x in re.search(r"static const [a-z ]+ " + name + r"\[[^=]*=\s*\{(.*?)\};", inc, re.S).group(1).replace("{", "").replace("}", "").split(",") if x.strip()]
    ntri, off, tri, order = body("MC_NTRI"), body("MC_OFF"), body("MC_TRI"), body("MC_ORDER")
    assert ntri == [len(t) for t in mr.TRIS]
    for c in range(256):
        assert tri[off[c]:off[c] + 3 * ntri[c]] == [k for t in mr.TRIS[c] for k in t]
        row = order[13 * c:13 * c + 13]
        assert row[:len(mr.ORDER[c])] == mr.ORDER[c] and set(row[len(mr.ORDER[c]):]) <= {15}
    assert sum(12 in o for o in mr.ORDER) == 24 and not mr.TRIS[0] and not mr.TRIS[255]


def test_install_rebinds_meshify():
    import pb3d
    pkg = types.ModuleType("fakeutils_mesh")
    vu = types.ModuleType("fakeutils_mesh.voxel_utils")
    vu.meshify_colored_voxel_grid = lambda *a, **k: "old"
    sys.modules["fakeutils_mesh"] = pkg
    sys.modules["fakeutils_mesh.voxel_utils"] = vu
    try:
        patched = pb3d.install(pkg)
        assert ("fakeutils_mesh.voxel_utils", "meshify_colored_voxel_grid") in patched
        assert vu.meshify_colored_voxel_grid is pb3d.meshify_colored_voxel_grid
    finally:
        for m in ("fakeutils_mesh", "fakeutils_mesh.voxel_utils"):
            del sys.modules[m]


@pytest.mark.parametrize("grid,stride,exc", [
    (np.zeros((4, 4, 4), np.uint8), 1, ValueError),            # not (A0, A1, A2, C)
    (np.zeros((4, 4, 4, 3), np.uint8), 0, ValueError),         # stride < 1
    (np.zeros((4, 1, 4, 3), np.uint8), 1, ValueError),         # lattice 1 on axis 1
    (np.zeros((5, 5, 3, 3), np.uint8), 3, ValueError),         # lattice (2, 2, 1)
], ids=["ndim", "stride0", "thin", "lattice1"])
def test_bad_arguments_raise_before_device_work(grid, stride, exc, monkeypatch):
    import pb3d
    from pb3d import _lib
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("device touched")))
    with pytest.raises(exc):
        pb3d.meshify_colored_voxel_grid(grid, stride)


def test_non_uint8_grid_is_refused_before_device_work(monkeypatch):
    import pb3d
    from pb3d import _lib
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("device touched")))
    with pytest.raises(TypeError):
        pb3d.meshify_colored_voxel_grid(np.ones((4, 4, 4, 3), np.float32))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", synth(), ids=lambda c: c[0])
def test_device_matches_reference_fixture(case):
    import pb3d
    name, grid, s, v, f, c, n = case
    gv, gf, gc, gn = pb3d.meshify_colored_voxel_grid(grid, stride=s)
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and gn.dtype == np.float32
    assert np.array_equal(gv, v) and np.array_equal(gf, f)
    assert np.array_equal(gn, n)
    check_colors(grid, s, v, gc, c)


@pytest.mark.gpu
@pytest.mark.parametrize("mon", STORED)
@pytest.mark.parametrize("stride", [4, 2, 1])
def test_stored_grids_match_reference(mon, stride):
    import pb3d
    from scipy.spatial import cKDTree
    meta = json.load(open(os.path.join(GOLD, "mesh_stored.json")))[f"{mon}_{stride}"]
    z = np.load(os.path.join(GOLD, "mesh_stored.npz"))
    grid = np.load(os.path.join(GOLD, f"stored_{mon}_voxel_grid.npz"))["voxel_grid"]
    v, f, c, n = pb3d.meshify_colored_voxel_grid(grid, stride=stride)
    assert (len(v), len(f)) == (meta["nverts"], meta["nfaces"])
    assert sha(v) == meta["verts_sha256"] and sha(f) == meta["faces_sha256"]
    assert sha(n) == meta["normals_sha256"]
    if stride > 1:
        assert np.array_equal(n, z[f"{mon}_{stride}_normals"])
    assert str(c.dtype) == meta["colors_dtype"]
    key = lambda a: a[..., 0].astype(np.int64) * 65536 + a[..., 1].astype(np.int64) * 256 + a[..., 2]
    ukey = np.flatnonzero(np.bincount(key(grid).ravel(), minlength=1 << 24))   # np.unique(grid.reshape(-1, 3), axis=0), as keys
    uniq = np.stack([ukey >> 16, (ukey >> 8) & 255, ukey & 255], axis=1)
    raw = np.rint(c * 255.0).astype(np.int64) if c.dtype == np.float64 else c.astype(np.int64)
    idx = np.searchsorted(key(uniq), key(raw))
    want = z[f"{mon}_{stride}_cidx"].astype(np.int64)
    bad = np.where(idx != want)[0]
    if len(bad):
        g = grid[::stride, ::stride, ::stride]
        mask = np.any(g > 0, axis=-1)
        pts = np.argwhere(mask)
        d, nb = cKDTree(pts).query(mr.queries(v[bad], stride), k=16)
        for r, i in enumerate(bad):
            tied = nb[r][d[r] == d[r][0]]
            assert d[r][-1] > d[r][0], "tie set larger than 16"
            cols = g[tuple(pts[tied].T)]
            assert len(np.unique(cols, axis=0)) > 1, f"vertex {i}: unique nearest colour differs"
            assert np.any(np.all(cols == uniq[idx[i]], axis=1))


def rand_grid(rng, shape, dens):
    pal = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [9, 8, 7]], np.uint8)
    occ = rng.random(shape) < dens
    return (pal[rng.integers(0, 4, shape)] * occ[..., None]).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dens,stride", [((13, 7, 9), 0.5, 1), ((33, 5, 6), 0.3, 1), ((6, 9, 31), 0.5, 1),
                                                ((40, 11, 12), 0.1, 3), ((17, 19, 16), 0.6, 2), ((70, 9, 66), 0.5, 4),
                                                ((5, 130, 7), 0.5, 1), ((9, 8, 200), 0.05, 1)])
def test_random_grids_match_restatement(shape, dens, stride):
    """odd shapes and strides; shape[0] > shape[2] puts the mirrored queries outside the grid; 130 / 200 span several bit words"""
    import pb3d
    grid = rand_grid(np.random.default_rng(hash((shape, stride)) % 2**32), shape, dens)
    v, f, c, n = pb3d.meshify_colored_voxel_grid(grid, stride=stride)
    rv, rf, rc, rn = mr.meshify(grid, stride)
    assert np.array_equal(v, rv) and np.array_equal(f, rf) and np.array_equal(n, rn)
    q0 = mr.queries(v, stride)[:, 0]
    if shape[0] > shape[2] + 2 * stride:
        assert (q0 < 0).any(), "the case meant to put queries outside the grid does not"
    assert c.dtype == rc.dtype and np.array_equal(c, rc)


@pytest.mark.gpu
def test_label_twin_equals_rgb_path():
    import pb3d
    from pb3d import labels
    rng = np.random.default_rng(7)
    pal = np.array(list(pb3d.PART_COLORS.values()), np.uint8)[:9]
    lab = (rng.integers(1, 10, (21, 14, 17)) * (rng.random((21, 14, 17)) < 0.45)).astype(np.uint8)
    for stride in (1, 2):
        a = labels.meshify_colored_voxel_grid_labels(lab, pal, stride=stride)
        b = pb3d.meshify_colored_voxel_grid(labels.label_to_rgb(lab, pal), stride=stride)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y)


@pytest.mark.gpu
def test_resident_form_equals_numpy_form():
    import pb3d
    from pb3d import device as dev
    grid = rand_grid(np.random.default_rng(3), (27, 15, 22), 0.4)
    d = dev.from_numpy(grid)
    try:
        for stride in (1, 2, 3):
            a = dev.meshify(d, grid.shape, stride=stride)
            b = pb3d.meshify_colored_voxel_grid(grid, stride=stride)
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and np.array_equal(x, y)
        (dv, df, dn, dc), (nv, nf) = dev.meshify(d, grid.shape, stride=1, download=False)
        assert np.array_equal(dv.download((nv, 3), np.float32), pb3d.meshify_colored_voxel_grid(grid)[0])
        for buf in (dv, df, dn, dc):
            buf.free()
    finally:
        d.free()


@pytest.mark.gpu
def test_mesh_fill_refuses_reused_state():
    """pb3d_mesh_count_dev(g1) -> pb3d_mesh_colors_dev(g2) -> pb3d_mesh_fill_dev(g1): the colour query rebuilds the lattice bits
    the count left, so the fill refuses (ValueError, nothing launched).  The outputs are sized for every cube plus one 256-cube
    block at the table's maxima (12 vertices, 9 triangles per cube), so even an unchecked fill would stay inside them.
    count -> fill -> fill again: both fills equal the restatement."""
    import ctypes as C
    import pb3d
    from pb3d import device as dev
    from pb3d.voxel_utils import mesh_colors
    L, lib = pb3d._lib, pb3d._lib.load()
    rng = np.random.default_rng(12)
    shape = (13, 11, 9)
    A0, A1, A2 = shape
    g1, g2 = rand_grid(rng, shape, 0.5), rand_grid(rng, shape, 0.3)
    d1, d2 = dev.from_numpy(g1), dev.from_numpy(g2)
    ncubes = (A0 - 1) * (A1 - 1) * (A2 - 1)
    vrows, frows = 12 * (ncubes + 256), 9 * (ncubes + 256)
    outs = [dev.DeviceBuffer(n) for n in (vrows * 12, frows * 12, vrows * 12, vrows * 3)]     # verts, faces, normals, colours
    for b in outs:
        b.upload(np.full(b.nbytes, 0xA5, np.uint8))
    qv, qc = dev.from_numpy(np.zeros((4, 3), np.float32)), dev.DeviceBuffer(4 * 3)
    nv, nf = C.c_int64(0), C.c_int64(0)
    ptr = lambda b: C.c_void_p(b.ptr)

    def fill():
        L.check(lib.pb3d_mesh_fill_dev(L.ctx(), ptr(d1), A0, A1, A2, 3, 1, nv.value, nf.value, *map(ptr, outs)))

    L.check(lib.pb3d_mesh_count_dev(L.ctx(), ptr(d1), A0, A1, A2, 3, 1, C.byref(nv), C.byref(nf)))
    assert nv.value > 0
    L.check(lib.pb3d_mesh_colors_dev(L.ctx(), ptr(d2), A0, A1, A2, 3, 1, ptr(qv), 4, ptr(qc)))
    with pytest.raises(ValueError, match="pb3d_mesh_fill: the state of pb3d_mesh_count was overwritten"):
        fill()
    assert all((b.download((b.nbytes,)) == 0xA5).all() for b in outs)
    L.check(lib.pb3d_mesh_count_dev(L.ctx(), ptr(d1), A0, A1, A2, 3, 1, C.byref(nv), C.byref(nf)))
    rv, rf, rc, rn = mr.meshify(g1, 1)
    for _ in range(2):
        fill()
        v = outs[0].download((nv.value, 3), np.float32)
        assert np.array_equal(v, rv) and np.array_equal(outs[1].download((nf.value, 3), np.int32), rf)
        assert np.array_equal(outs[2].download((nv.value, 3), np.float32), rn)
        gc = mesh_colors(outs[3].download((nv.value, 3)))
        assert gc.dtype == rc.dtype and np.array_equal(gc, rc)
    for b in outs + [d1, d2, qv, qc]:
        b.free()


@pytest.mark.gpu
def test_host_mesh_fill_refuses_restaged_grid():
    """pb3d_mesh_count -> pb3d_carve_mask -> pb3d_mesh_fill: the carve stages its grid where the count left its own, so the fill
    refuses and leaves the caller's arrays alone.  count -> fill still equals the restatement, and the host fill is one-shot as
    before."""
    import ctypes as C
    import pb3d
    from pb3d.voxel_utils import mesh_colors
    L, lib = pb3d._lib, pb3d._lib.load()
    rng = np.random.default_rng(13)
    shape = (12, 10, 14)
    A0, A1, A2 = shape
    g = rand_grid(rng, shape, 0.4)
    mask = np.ones((A0, A1), np.uint8)
    carved = np.empty_like(g)
    nv, nf = C.c_int64(0), C.c_int64(0)

    def count():
        L.check(lib.pb3d_mesh_count(L.ctx(), L.p_u8(g), A0, A1, A2, 3, 1, C.byref(nv), C.byref(nf)))
        assert nv.value > 0
        return (np.full((nv.value, 3), -7.0, np.float32), np.full((nf.value, 3), -7, np.int32), np.full((nv.value, 3), -7.0, np.float32),
                np.full((nv.value, 3), 0xA5, np.uint8))

    def fill(outs):
        L.check(lib.pb3d_mesh_fill(L.ctx(), nv.value, nf.value, *[o.ctypes.data_as(C.c_void_p) for o in outs]))

    outs = count()
    L.check(lib.pb3d_carve_mask(L.ctx(), L.p_u8(g), A0, A1, A2, 3, L.p_u8(mask), L.p_u8(carved)))
    with pytest.raises(ValueError, match="pb3d_mesh_fill: the state of pb3d_mesh_count was overwritten"):
        fill(outs)
    assert all((o == (0xA5 if o.dtype == np.uint8 else -7)).all() for o in outs)
    outs = count()
    fill(outs)
    v, f, n, c = outs
    rv, rf, rc, rn = mr.meshify(g, 1)
    assert np.array_equal(v, rv) and np.array_equal(f, rf) and np.array_equal(n, rn)
    assert mesh_colors(c).dtype == rc.dtype and np.array_equal(mesh_colors(c), rc)
    with pytest.raises(ValueError, match="call pb3d_mesh_count first"):
        fill(outs)


@pytest.mark.gpu
def test_error_cases_raise_like_the_reference():
    import pb3d
    with pytest.raises(ValueError, match="Surface level"):
        pb3d.meshify_colored_voxel_grid(np.zeros((6, 5, 4, 3), np.uint8))
    with pytest.raises(ValueError, match="Surface level"):
        pb3d.meshify_colored_voxel_grid(np.full((6, 5, 4, 3), 3, np.uint8))
    g = np.zeros((6, 5, 4, 3), np.uint8)
    g[1::2] = 9    # occupied only off the stride-2 lattice: an all-empty lattice
    with pytest.raises(ValueError, match="Surface level"):
        pb3d.meshify_colored_voxel_grid(g, stride=2)
    with pytest.raises(ValueError, match="2x2x2"):
        pb3d.meshify_colored_voxel_grid(np.ones((6, 5, 1, 3), np.uint8))
