"""mesh_components, mesh_topology, select_faces and keep_mesh_components (pb3d/meshcomp.py, csrc/meshcomp.hip, csrc/simplify.hip) against
the NumPy / SciPy restatement of tests/meshcomp_restate.py, and that restatement against a plain per-face Python loop.  Every comparison
is np.array_equal (floats by their bytes): include/pb3d.h states the result to the bit, so there is no tolerance anywhere."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import meshcomp_restate as mr
import simplify_restate as sr
from pb3d import keep_mesh_components, mesh_components, mesh_topology, select_faces  # noqa: F401  (without the feature nothing in this file can run)

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONNECTIVITIES = ("edge", "vertex")
SEAM_STRIPS = (682, 683, 1366, 4097)            # 3 m = 2046, 2049, 4098 and 12291 records: the sort's tile is 2048 pairs
SUM_STRIPS = (255, 256, 257, 513, 65537)        # faces: the sums' block is 256


# ---- the cases: name -> (vertices, faces) ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, arg = name.partition("/")
    hand = dict(tets_vertex=mr.tets_sharing_vertex, tets_edge=mr.tets_sharing_edge, flipped=mr.tet_with_flipped_face, open=mr.open_triangle,
                loops=mr.loop_faces, book=mr.book, triangles=mr.disjoint_triangles, fragments=mr.fragments_mesh, ranked=mr.ranked_tets,
                folded=sr.folded_mesh)
    if kind in hand:
        return tuple(hand[kind]())
    if kind == "strip":
        return mr.strip(int(arg))
    V, F = mr.fragments_mesh()
    if kind == "faces_reversed":
        return V, np.ascontiguousarray(F[::-1])
    if kind == "vertices_reversed":
        return np.ascontiguousarray(V[::-1]), (len(V) - 1 - F).astype(F.dtype)
    if kind == "f64i64":
        return V.astype(np.float64) * np.pi, F.astype(np.int64)
    if kind == "uint16":
        return V.astype(np.float16), F.astype(np.uint16)
    if kind == "negative":
        G = F.copy()
        G[np.random.default_rng(4).random(G.shape) < 0.5] -= len(V)
        return V, G
    assert kind == "unreferenced"
    return sr.with_unreferenced(V, F)


HAND = ["tets_vertex", "tets_edge", "flipped", "open", "loops"]
SEAMS = [f"strip/{m}" for m in SEAM_STRIPS] + ["book"]
SUMS = [f"strip/{m}" for m in SUM_STRIPS]
MANY = ["triangles", "fragments"]
PERMUTED = ["faces_reversed", "vertices_reversed"]
TYPED = ["f64i64", "uint16", "negative", "unreferenced"]
CASES = HAND + SEAMS + SUMS + MANY + PERMUTED + TYPED + ["ranked", "folded"]


@functools.lru_cache(maxsize=None)
def want(name, connectivity, measured=True):
    """the restatement of a case, computed once and shared"""
    V, F = case(name)
    r = mr.restate(F, len(V), V if measured else None, connectivity)
    for a in [r["face_labels"], r["vertex_labels"], *r["stats"].values()]:
        a.setflags(write=False)
    return r


def same_result(got, ref, what):
    assert got["totals"] == ref["totals"], (what, got["totals"], ref["totals"])
    for part in ("face_labels", "vertex_labels"):
        g, w = got[part], ref[part]
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (what, part)
    assert list(got["stats"]) == list(ref["stats"]), (what, list(got["stats"]))
    for part, w in ref["stats"].items():
        g = got["stats"][part]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, g.shape)
        if not np.array_equal(g.view(np.uint8), w.view(np.uint8)):
            bad = np.flatnonzero(g != w)
            raise AssertionError((what, part, "first differing component", int(bad[0]), g[bad[0]], w[bad[0]], "differing", len(bad), "of", len(g)))


def same_mesh(got, ref, what):
    for g, w, part in zip(got, ref, sr.PARTS):
        assert (g is None) == (w is None), (what, part)
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint8) if part == "vertices" else g, w.view(np.uint8) if part == "vertices" else w), (what, part)


# =====================================================================================================================
# CPU: the restatement against a loop, its invariants, the pinned counts; exports; validation
# =====================================================================================================================

@pytest.mark.parametrize("name", CASES)
def test_restatement_is_the_loop(name):
    V, F = case(name)
    for conn in CONNECTIVITIES:
        same_result(want(name, conn), mr.loop(F, len(V), V, conn), (name, conn))


@pytest.mark.parametrize("name", CASES)
def test_restatement_invariants(name):
    V, F = case(name)
    for conn in CONNECTIVITIES:
        r = want(name, conn)
        lab, st, t = r["face_labels"], r["stats"], r["totals"]
        nc = t["components"]
        ids, first = np.unique(lab, return_index=True)
        assert np.array_equal(ids, np.arange(nc)) and (np.diff(first) > 0).all() and first[0] == 0           # dense, numbered by first face
        assert st["faces"].sum() == len(F) == t["faces"] and st["edges"].sum() == t["edges"]
        for part in ("boundary_edges", "nonmanifold_edges", "unbalanced_edges"):
            assert st[part].sum() == t[part]
        assert (st["boundary_edges"] <= st["unbalanced_edges"]).all()
        assert t["vertices"] == len(np.unique(np.where(F.astype(np.int64) < 0, F.astype(np.int64) + len(V), F)))
        assert (st["area"] >= 0).all() and np.isfinite(st["volume"]).all()
        assert (r["totals"]["unbalanced_edges"] == 0) == sr.edge_balanced(np.where(F.astype(np.int64) < 0, F.astype(np.int64) + len(V), F))
    e, v = want(name, "edge"), want(name, "vertex")
    assert v["totals"]["components"] <= e["totals"]["components"]
    assert {k: x for k, x in e["totals"].items() if k != "components"} == {k: x for k, x in v["totals"].items() if k != "components"}


def test_pinned_counts():
    t = want("folded", "edge")["totals"]
    assert (t["components"], t["edges"], t["boundary_edges"], t["nonmanifold_edges"], t["unbalanced_edges"]) == (1, 15951, 0, 21, 0)
    assert t["vertices"] - t["edges"] + t["faces"] == -733
    V, F = case("fragments")
    assert (len(V), len(F)) == (2608, 5352)
    e, v = want("fragments", "edge"), want("fragments", "vertex")
    assert e["totals"]["components"] == v["totals"]["components"] == 43 and np.array_equal(e["face_labels"], v["face_labels"])
    assert e["stats"]["faces"].max() == 4088 and e["stats"]["faces"].min() == 8
    t = e["totals"]
    assert t["nonmanifold_edges"] == 24 and t["vertices"] - t["edges"] + t["faces"] == -44


def test_hand_made_meshes():
    n = lambda name, conn: want(name, conn)["totals"]
    assert n("tets_vertex", "vertex")["components"] == 1 and n("tets_vertex", "edge")["components"] == 2
    for conn in CONNECTIVITIES:
        assert (n("tets_edge", conn)["components"], n("tets_edge", conn)["nonmanifold_edges"]) == (1, 1)
        assert (n("flipped", conn)["unbalanced_edges"], n("flipped", conn)["boundary_edges"]) == (3, 0)
        assert (n("open", conn)["boundary_edges"], n("open", conn)["edges"], n("open", conn)["components"]) == (3, 3, 1)
        assert n("loops", conn)["loops"] == 7 and n("loops", conn)["edges"] == 1 and n("loops", conn)["unbalanced_edges"] == 0
        assert n("book", conn)["nonmanifold_edges"] == 1 and n("book", conn)["components"] == 1
        assert n("triangles", conn)["components"] == 5000
    assert mr.restate([[0, 0, 1]], 4)["totals"]["loops"] == 1 and mr.restate([[2, 2, 2]], 4)["totals"]["loops"] == 3
    assert want("loops", "edge")["face_labels"].tolist() == [0, 1, 2] and want("loops", "vertex")["face_labels"].tolist() == [0, 1, 0]
    assert want("tets_vertex", "edge")["stats"]["volume"][0] == 1.0 / 6.0 and want("open", "edge")["stats"]["area"].tolist() == [0.5]
    ranked = want("ranked", "edge")["stats"]
    assert ranked["faces"].tolist() == [4, 4, 4] and int(np.argmax(ranked["area"])) == 1 and int(np.argmax(np.abs(ranked["volume"]))) == 2
    assert ranked["volume"][2] < 0 < ranked["volume"][0]


def test_exports():
    import pb3d
    names = ("mesh_components", "mesh_topology", "select_faces", "keep_mesh_components")
    for n in names + tuple(n + "_resident" for n in names):
        assert callable(getattr(pb3d, n)) and n in pb3d.meshcomp.__all__
    header = open(os.path.join(ROOT, "include", "pb3d.h")).read()
    for s in ("pb3d_mesh_components_resident", "pb3d_mesh_select_faces_resident"):
        assert s in pb3d._lib.EXPORTED_SYMBOLS and re.search(r"^int\s+" + s + r"\s*\(", header, re.M)


def test_validation_needs_no_device():
    import pb3d
    V = np.zeros((4, 3))
    F = np.array([[0, 1, 2]])
    for conn in ("face", None, 0, True):
        for fn in (lambda: pb3d.mesh_components(F, 4, connectivity=conn), lambda: pb3d.keep_mesh_components(V, F, connectivity=conn),
                   lambda: pb3d.mesh_components_resident(None, 1, 4, connectivity=conn),
                   lambda: pb3d.keep_mesh_components_resident(None, 4, None, 1, connectivity=conn)):
            with pytest.raises(ValueError, match="connectivity must be 'edge' or 'vertex'"):
                fn()
    for rank_by in ("size", None, 0):
        for fn in (lambda: pb3d.keep_mesh_components(V, F, k=1, rank_by=rank_by), lambda: pb3d.keep_mesh_components_resident(None, 4, None, 1, k=1, rank_by=rank_by)):
            with pytest.raises(ValueError, match="rank_by must be 'faces', 'area' or 'volume'"):
                fn()
    for k in (0, -1, 1.0, True, "1"):
        for fn in (lambda: pb3d.keep_mesh_components(V, F, k=k), lambda: pb3d.keep_mesh_components_resident(None, 4, None, 1, k=k)):
            with pytest.raises(ValueError, match="k must be an integer >= 1"):
                fn()
    with pytest.raises(ValueError, match="min_faces must be an integer >= 0"):
        pb3d.keep_mesh_components(V, F, min_faces=-1)
    for a in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="min_area must be finite and >= 0"):
            pb3d.keep_mesh_components(V, F, min_area=a)
    for keep in (np.ones(2, bool), np.ones((1, 1), bool), np.ones(1, np.float32), []):
        with pytest.raises(ValueError, match="keep must be a boolean or integer array of shape"):
            pb3d.select_faces(V, F, keep)
    for bad in (np.nan, np.inf, -np.inf):
        p = V.copy()
        p[3, 1] = bad                                                           # a vertex no face names
        for fn in (lambda: pb3d.mesh_components(F, vertices=p), lambda: pb3d.keep_mesh_components(p, F, k=1)):
            with pytest.raises(ValueError, match="NaN or infinity"):
                fn()
    with pytest.raises(ValueError, match="n_vertices"):
        pb3d.mesh_components(F, 5, vertices=V)
    for fn in (lambda v, f: pb3d.mesh_components(f, vertices=v), lambda v, f: pb3d.select_faces(v, f, np.ones(len(f), bool)), pb3d.keep_mesh_components):
        with pytest.raises(ValueError, match=r"\(n, 3\)"):
            fn(np.zeros((4, 2)), F)
        with pytest.raises(ValueError, match=r"\(m, 3\)"):
            fn(V, np.zeros((2, 4), np.int32))
        with pytest.raises(IndexError):
            fn(V, np.zeros((1, 3)))                                             # float indices
        with pytest.raises(IndexError):
            fn(np.zeros((0, 3)), F)                                             # no vertex, one face
        with pytest.raises(IndexError):
            fn(V, np.array([[0, 1, 4]], np.uint32))
    with pytest.raises(IndexError):
        pb3d.mesh_topology(F, 0)
    with pytest.raises(ValueError, match="at most 2\\^31 - 1 vertices"):
        pb3d.mesh_components_resident(None, 1, 2 ** 31)
    with pytest.raises(ValueError, match="faces"):
        pb3d.mesh_components_resident(None, 2 ** 31, 4)


def test_empty_inputs_need_no_device():
    import pb3d
    for vdt, fdt in ((np.float32, np.int32), (np.float64, np.int64), (np.int16, np.uint8)):
        V, F = np.ones((5, 3), vdt), np.zeros((0, 3), fdt)
        for conn in CONNECTIVITIES:
            lab, stats, vlab = pb3d.mesh_components(F, vertices=V, connectivity=conn, return_vertex_labels=True)
            same_result(dict(face_labels=lab, vertex_labels=vlab, stats=stats, totals=dict.fromkeys(mr.TOTALS, 0)), mr.restate(F, 5, V, conn),
                        (vdt, fdt, conn))
            lab, stats = pb3d.mesh_components(F, 5, connectivity=conn)
            assert lab.dtype == np.int32 and lab.shape == (0,) and list(stats) == list(mr.COUNTS)
        t = pb3d.mesh_topology(F, 5)
        assert {k: t[k] for k in mr.TOTALS} == dict.fromkeys(mr.TOTALS, 0) and t["euler"] == 0 and t["closed"] and t["edge_manifold"] and t["watertight"]
        cols = np.zeros((5, 1), np.uint8)
        same_mesh(pb3d.select_faces(V, F, np.zeros(0, bool), colors=cols, return_index=True, return_inverse=True, return_face_index=True),
                  mr.select(V, F, np.zeros(0, bool), cols), (vdt, fdt))
        got = pb3d.keep_mesh_components(V, F, k=1, colors=cols, return_labels=True)
        assert [a.shape for a in got] == [(0, 3), (0, 3), (0, 1), (0,), (0,)] and got[0].dtype == (vdt if vdt == np.float32 else np.float64)
    lab, stats, vlab = pb3d.mesh_components(np.zeros((0, 3), np.int32), return_vertex_labels=True)
    assert lab.shape == (0,) and vlab.shape == (0,) and vlab.dtype == np.int32
    assert len(pb3d.select_faces(np.zeros((0, 3)), np.zeros((0, 3), np.int32), np.zeros(0, bool))) == 2


def test_cabi_refusals_need_no_device():
    import pb3d
    lib = pb3d._lib.load()
    one, two, three = C.c_void_p(256), C.c_void_p(512), C.c_void_p(1024)
    totals = (C.c_int64 * 8)(*([7] * 8))
    counts = (C.c_int64 * 2)(7, 7)
    comp, select = lib.pb3d_mesh_components_resident, lib.pb3d_mesh_select_faces_resident

    def refused(rc, text):
        assert rc == -1 and text in lib.pb3d_last_error().decode(), (rc, lib.pb3d_last_error())

    refused(comp(None, None, 0, -1, one, 0, 1, 0, two, None, None, None, totals), "negative count")
    refused(comp(None, None, 0, 5, one, 0, -1, 0, two, None, None, None, totals), "negative count")
    refused(comp(None, None, 0, 2 ** 31, one, 0, 1, 0, two, None, None, None, totals), "at most 2^31 - 1 vertices")
    refused(comp(None, None, 0, 5, one, 0, (2 ** 31 - 1) // 6 + 1, 0, two, None, None, None, totals), "(2^31 - 1) / 6 faces")
    for conn in (-1, 2):
        refused(comp(None, None, 0, 5, one, 0, 2, conn, two, None, None, None, totals), "connectivity must be 0 (edge) or 1 (vertex)")
    refused(comp(None, None, 0, 5, one, 0, 2, 0, two, None, None, None, None), "null argument")
    refused(comp(None, None, 0, 5, None, 0, 2, 0, two, None, None, None, totals), "null buffer")
    refused(comp(None, None, 0, 5, one, 0, 2, 0, None, None, None, None, totals), "null buffer")
    refused(comp(None, None, 0, 5, one, 0, 2, 0, two, None, None, three, totals), "null buffer")         # measures without vertices
    refused(comp(None, None, 0, 5, one, 0, 2, 0, one, None, None, None, totals), "may not alias")
    refused(comp(None, three, 0, 5, one, 0, 2, 0, two, three, None, None, totals), "may not alias")
    refused(comp(None, None, 0, 5, one, 0, 2, 0, two, None, None, None, totals), "null context")
    refused(comp(None, None, 0, 0, None, 0, 0, 1, None, None, None, None, totals), "null context")       # an empty mesh needs no buffers
    assert list(totals) == [7] * 8

    def sel(nv, nf, keep, colors, channels, out_v, out_f, out_c, cnt, text, verts=one, faces=one):
        refused(select(None, verts, 0, nv, faces, 0, nf, keep, colors, channels, out_v, out_f, out_c, None, None, None, cnt), text)

    sel(-1, 1, three, None, 3, two, two, None, counts, "negative count")
    sel(5, 2 ** 31, three, None, 3, two, two, None, counts, "at most 2^31 - 1")
    sel(5, 2, three, None, 3, two, two, None, None, "null argument")
    sel(5, 2, three, one, 2, two, two, two, counts, "channels must be 1 or 3")
    sel(5, 2, three, None, 3, two, two, None, counts, "null buffer", verts=None)
    sel(5, 2, None, None, 3, two, two, None, counts, "null buffer")
    sel(5, 2, three, None, 3, None, two, None, counts, "null buffer")
    sel(5, 2, three, one, 3, two, two, None, counts, "null buffer")
    sel(5, 2, three, None, 3, one, two, None, counts, "may not alias")
    sel(5, 2, two, None, 3, two, two, None, counts, "may not alias")
    sel(5, 2, three, None, 3, two, two, None, counts, "null context")
    sel(0, 0, None, None, 3, None, None, None, counts, "null context", verts=None, faces=None)
    assert list(counts) == [7, 7]


# =====================================================================================================================
# GPU
# =====================================================================================================================

def on_device(pb3d, name, conn, measured):
    V, F = case(name)
    if measured:
        lab, stats, vlab = pb3d.mesh_components(F, vertices=V, connectivity=conn, return_vertex_labels=True)
    else:
        lab, stats, vlab = pb3d.mesh_components(F, len(V), connectivity=conn, return_vertex_labels=True)
    t = pb3d.mesh_topology(F, len(V))
    totals = {k: t[k] for k in mr.TOTALS}
    ref = want(name, "edge", measured)["totals"]
    assert t["euler"] == ref["vertices"] - ref["edges"] + ref["faces"] and t["closed"] == (ref["unbalanced_edges"] == 0)
    assert t["edge_manifold"] == (ref["nonmanifold_edges"] == 0)
    assert t["watertight"] == (ref["unbalanced_edges"] == 0 and ref["nonmanifold_edges"] == 0 and ref["boundary_edges"] == 0)
    totals["components"] = len(stats["faces"])                                  # mesh_topology counts by edge; the stats name this rule's
    assert conn != "edge" or t["components"] == len(stats["faces"])
    return dict(face_labels=lab, vertex_labels=vlab, stats=stats, totals=totals)


def check(pb3d, names):
    for name in names:
        for conn in CONNECTIVITIES:
            for measured in (True, False):
                same_result(on_device(pb3d, name, conn, measured), want(name, conn, measured), (name, conn, measured))


@gpu
def test_hand_made_on_the_device(pb3d_gpu):
    check(pb3d_gpu, HAND + ["ranked"])
    for face, loops in (([[0, 0, 1]], 1), ([[2, 2, 2]], 3)):
        assert pb3d_gpu.mesh_topology(np.array(face, np.int32), 4)["loops"] == loops


@gpu
@pytest.mark.parametrize("name", SEAMS)
def test_sort_tile_seams(pb3d_gpu, name):
    check(pb3d_gpu, [name])
    if name == "book":
        t = pb3d_gpu.mesh_topology(case(name)[1], len(case(name)[0]))
        assert (t["nonmanifold_edges"], t["unbalanced_edges"], t["boundary_edges"]) == (1, 1 + 2 * 4097, 2 * 4097) and not t["closed"]


@gpu
@pytest.mark.parametrize("name", SUMS)
def test_block_seams_of_the_sums(pb3d_gpu, name):
    V, F = case(name)
    for conn in CONNECTIVITIES:
        _, stats = pb3d_gpu.mesh_components(F, vertices=V, connectivity=conn)
        ref = want(name, conn)["stats"]
        for part in ("area", "volume"):
            assert stats[part].tobytes() == ref[part].tobytes(), (name, conn, part, stats[part], ref[part])


@gpu
@pytest.mark.parametrize("name", MANY + ["folded"])
def test_many_components(pb3d_gpu, name):
    check(pb3d_gpu, [name])


@gpu
def test_numbering_follows_the_faces(pb3d_gpu):
    check(pb3d_gpu, PERMUTED)
    V, F = case("fragments")
    plain, _ = pb3d_gpu.mesh_components(F, len(V))
    rev, _ = pb3d_gpu.mesh_components(case("faces_reversed")[1], len(V))
    moved, _ = pb3d_gpu.mesh_components(case("vertices_reversed")[1], len(V))
    assert np.array_equal(moved, plain) and rev[0] == 0 and not np.array_equal(rev[::-1], plain)
    order = {}
    renamed = np.array([order.setdefault(l, len(order)) for l in plain[::-1].tolist()], np.int32)
    assert np.array_equal(rev, renamed)


@gpu
def test_dtypes_and_indices(pb3d_gpu):
    check(pb3d_gpu, TYPED)
    V, F = case("unreferenced")
    lab, stats, vlab = pb3d_gpu.mesh_components(F, len(V), return_vertex_labels=True)
    named = np.zeros(len(V), bool)
    named[F.reshape(-1)] = True
    assert (vlab[~named] == -1).all() and (vlab[named] >= 0).all() and pb3d_gpu.mesh_topology(F, len(V))["vertices"] == named.sum() < len(V)


OUT_FILL = 0xA5


@gpu
def test_bad_index_writes_nothing(pb3d_gpu):
    L = pb3d_gpu._lib
    lib, ctx = L.load(), L.ctx()
    V, F = case("fragments")
    nv, nf = len(V), len(F)
    d_v = pb3d_gpu.device.from_numpy(V)
    outs = [pb3d_gpu.device.DeviceBuffer(n) for n in (nf * 4, nv * 4, nf * 40, nf * 16)]
    souts = [pb3d_gpu.device.DeviceBuffer(n) for n in (nv * 12, nf * 24, nv * 4, nv * 4, nf * 4)]
    d_keep = pb3d_gpu.device.from_numpy(np.ones(nf, np.uint8))
    try:
        for fdt in (np.int32, np.int64):
            for bad in (nv, -nv - 1):
                G = F.astype(fdt)
                G[nf - 1, 2] = bad
                for fn in (lambda: pb3d_gpu.mesh_components(G, vertices=V), lambda: pb3d_gpu.mesh_topology(G, nv),
                           lambda: pb3d_gpu.select_faces(V, G, np.ones(nf, bool)), lambda: pb3d_gpu.keep_mesh_components(V, G, k=1)):
                    with pytest.raises(IndexError, match="out of bounds"):
                        fn()
                d_f = pb3d_gpu.device.from_numpy(G)
                try:
                    for b in outs + souts:
                        b.upload(np.full(b.nbytes, OUT_FILL, np.uint8))
                    totals = (C.c_int64 * 8)(*([-3] * 8))
                    counts = (C.c_int64 * 2)(-3, -3)
                    p = [C.c_void_p(b.ptr) for b in outs]
                    q = [C.c_void_p(b.ptr) for b in souts]
                    rc = lib.pb3d_mesh_components_resident(ctx, C.c_void_p(d_v.ptr), 0, nv, C.c_void_p(d_f.ptr), int(fdt == np.int64), nf, 0, *p, totals)
                    assert rc == -6 and b"index out of bounds" in lib.pb3d_last_error() and list(totals) == [-3] * 8
                    rc = lib.pb3d_mesh_select_faces_resident(ctx, C.c_void_p(d_v.ptr), 0, nv, C.c_void_p(d_f.ptr), int(fdt == np.int64), nf,
                                                             C.c_void_p(d_keep.ptr), None, 3, q[0], q[1], None, q[2], q[3], q[4], counts)
                    assert rc == -6 and b"index out of bounds" in lib.pb3d_last_error() and list(counts) == [-3, -3]
                    for b in outs + souts:
                        assert (b.download((b.nbytes,)) == OUT_FILL).all(), (fdt, bad, "an output was written")
                finally:
                    d_f.free()
    finally:
        for b in [d_v, d_keep] + outs + souts:
            b.free()


ALL = dict(return_index=True, return_inverse=True, return_face_index=True)


@gpu
def test_select_faces(pb3d_gpu):
    V, F, colors = sr.colored_mesh()
    rng = np.random.default_rng(23)
    for cols in (colors, np.ascontiguousarray(colors[:, 2:]), None):
        for keep in (rng.random(len(F)) < 0.4, np.ones(len(F), bool), np.zeros(len(F), np.int8), (rng.random(len(F)) < 0.5) * 7):
            got = pb3d_gpu.select_faces(V, F, keep, colors=cols, **ALL)
            got = got if cols is not None else (got[0], got[1], None, *got[2:])
            same_mesh(got, mr.select(V, F, keep, cols), ("colored", None if cols is None else cols.shape, int(np.count_nonzero(keep))))
    got = pb3d_gpu.select_faces(V, F, np.ones(len(F), bool))
    assert got[0].tobytes() == V.tobytes() and got[1].tobytes() == F.tobytes()                 # no unreferenced vertex: the input arrays
    # degenerate and repeated faces stay when flagged; non-finite vertices are copied byte for byte
    W = V.copy()
    W[5] = (np.nan, np.inf, -0.0)
    G = np.concatenate([F[:40], [[5, 5, 6], [7, 7, 7]], F[:3], F[10:12][:, [1, 2, 0]]]).astype(np.int32)
    keep = np.ones(len(G), bool)
    keep[::3] = False
    keep[40:] = True
    for vdt, fdt in ((np.float32, np.int32), (np.float64, np.int64)):
        same_mesh(pb3d_gpu.select_faces(W.astype(vdt), G.astype(fdt), keep, **ALL)[:2], mr.select(W.astype(vdt), G.astype(fdt), keep)[:2], (vdt, fdt))
    got = pb3d_gpu.select_faces(W, G, keep, **ALL)
    ref = mr.select(W, G, keep)
    same_mesh((got[0], got[1], None, *got[2:]), ref, "degenerate")
    assert len(got[1]) == int(keep.sum()) and np.array_equal(got[4], np.flatnonzero(keep))


RANKINGS = ("faces", "area", "volume")


def on_device_keep(pb3d, V, F, colors=None, **how):
    got = pb3d.keep_mesh_components(V, F, colors=colors, return_labels=True, **how)
    return got if colors is not None else (got[0], got[1], None, *got[2:])


def same_keep(got, ref, what):
    same_mesh(got[:3], ref[:3], what)
    assert got[3].dtype == np.int32 and np.array_equal(got[3], ref[3]) and got[4].dtype == np.intp and np.array_equal(got[4], ref[4]), what


@gpu
def test_keep_mesh_components(pb3d_gpu):
    V, F = case("fragments")
    for conn in CONNECTIVITIES:
        for how in (dict(k=1), dict(k=3), dict(min_faces=9), dict(closed_only=True), dict(k=100), dict(min_faces=9, k=2, rank_by="area"),
                    dict(min_area=3.0), dict()):
            same_keep(on_device_keep(pb3d_gpu, V, F, connectivity=conn, **how), mr.keep_components(V, F, connectivity=conn, **how), (conn, how))
    largest = pb3d_gpu.keep_mesh_components(V, F, k=1)
    lab, stats = pb3d_gpu.mesh_components(largest[1], vertices=largest[0])
    assert len(stats["faces"]) == 1 and stats["faces"][0] == 4088 == len(largest[1]) and (lab == 0).all()
    # two identical tetrahedra: the tie goes to the first
    T = np.concatenate([mr.TET, mr.TET + 4]).astype(np.int32)
    P = np.concatenate([mr.TET_VERTS, mr.TET_VERTS])
    for rank_by in RANKINGS:
        got = on_device_keep(pb3d_gpu, P, T, k=1, rank_by=rank_by)
        assert np.array_equal(got[1], mr.TET) and got[4].tolist() == [0]
    # three rankings, three answers
    V3, F3 = case("ranked")
    cols = (np.arange(36, dtype=np.uint8).reshape(12, 3) * 7)
    picks = {}
    for rank_by in RANKINGS:
        got = on_device_keep(pb3d_gpu, V3, F3, colors=cols, k=1, rank_by=rank_by)
        same_keep(got, mr.keep_components(V3, F3, cols, k=1, rank_by=rank_by), rank_by)
        picks[rank_by] = got[4].tolist()
    assert picks == dict(faces=[0], area=[1], volume=[2])
    same_keep(on_device_keep(pb3d_gpu, V3, F3, k=2, rank_by="volume"), mr.keep_components(V3, F3, k=2, rank_by="volume"), "k=2 by volume")


@gpu
def test_kept_mesh_voxelizes_like_the_restatement(pb3d_gpu):
    V, F = case("fragments")
    for how in (dict(k=1), dict(closed_only=True, min_faces=9)):
        verts, faces = pb3d_gpu.keep_mesh_components(V, F, **how)
        ref = mr.keep_components(V, F, **how)
        assert pb3d_gpu.mesh_topology(faces, len(verts))["closed"]
        got = pb3d_gpu.voxelize_mesh(verts, faces, (16, 16, 16))
        assert got.any() and np.array_equal(got, pb3d_gpu.voxelize_mesh(ref[0], ref[1], (16, 16, 16)))
        assert np.array_equal(got, pb3d_gpu.voxelize_mesh(V, F[np.isin(ref[3], ref[4])], (16, 16, 16)))


def arena(pb3d, array, off):
    """the array at byte `off` of a buffer of its own: (buffer, address)"""
    a = np.ascontiguousarray(array)
    buf = pb3d.device.DeviceBuffer(a.nbytes + 64)
    buf.upload(a, off)
    return buf, buf.at(off)


@gpu
def test_resident_twins_and_byte_offsets(pb3d_gpu):
    """the resident forms on buffers that start 4 and 12 bytes (8 and 24 for the 8-byte types) behind an allocation give the bytes of
    the NumPy forms"""
    for name, conn in (("fragments", "edge"), ("f64i64", "vertex"), ("book", "edge")):
        V, F = case(name)
        V, F = np.ascontiguousarray(V), np.ascontiguousarray(F)
        nv, nf = len(V), len(F)
        ref = want(name, conn)
        kw = dict(verts_f64=V.dtype == np.float64, faces_i64=F.dtype == np.int64)
        for ov, of in ((0, 0), (V.dtype.itemsize, 3 * F.dtype.itemsize), (3 * V.dtype.itemsize, F.dtype.itemsize)):
            (bv, pv), (bf, pf) = arena(pb3d_gpu, V, ov), arena(pb3d_gpu, F, of)
            held = [bv, bf]
            try:
                d_lab, d_vlab, d_counts, d_meas, t = pb3d_gpu.mesh_components_resident(pf, nf, nv, pv, conn, **kw)
                held += [d_lab, d_vlab, d_counts, d_meas]
                nc = t["components"]
                stats = {k: a for k, a in zip(mr.COUNTS, d_counts.download((5, nc), np.int64))}
                stats.update({k: a for k, a in zip(("area", "volume"), d_meas.download((2, nc), np.float64))})
                t["components"] = nc
                same_result(dict(face_labels=d_lab.download((nf,), np.int32), vertex_labels=d_vlab.download((nv,), np.int32), stats=stats,
                                 totals={k: t[k] for k in mr.TOTALS}), ref, (name, conn, ov, of))
                assert {k: pb3d_gpu.mesh_topology_resident(pf, nf, nv, kw["faces_i64"])[k] for k in mr.TOTALS if k != "components"} \
                    == {k: x for k, x in ref["totals"].items() if k != "components"}
                keep = np.random.default_rng(nf).random(nf) < 0.5
                bk, pk = arena(pb3d_gpu, keep.view(np.uint8), 1)
                held.append(bk)
                *bufs, (n, m) = pb3d_gpu.select_faces_resident(pv, nv, pf, nf, pk, **kw)
                held += [b for b in bufs if b is not None]
                want_mesh = mr.select(V, F, keep)
                same_mesh((bufs[0].download((n, 3), V.dtype), bufs[1].download((m, 3), F.dtype), None, bufs[3].download((n,), np.int32).astype(np.intp),
                           bufs[4].download((nv,), np.int32).astype(np.intp), bufs[5].download((m,), np.int32).astype(np.intp)), want_mesh,
                          (name, "select", ov, of))
                (*bufs, (n, m)), d_lab2, chosen = pb3d_gpu.keep_mesh_components_resident(pv, nv, pf, nf, k=2, rank_by="area", connectivity=conn, **kw)
                held += [b for b in bufs if b is not None] + [d_lab2]
                kept = mr.keep_components(V, F, connectivity=conn, k=2, rank_by="area")
                assert np.array_equal(chosen, kept[4]) and np.array_equal(d_lab2.download((nf,), np.int32), kept[3])
                assert bufs[0].download((n, 3), V.dtype).tobytes() == kept[0].tobytes() and np.array_equal(bufs[1].download((m, 3), F.dtype), kept[1])
            finally:
                for b in held:
                    b.free()


@gpu
def test_runs_twice_alike_and_host_waits(pb3d_gpu):
    V, F = case("fragments")
    d_v, d_f = pb3d_gpu.device.from_numpy(V), pb3d_gpu.device.from_numpy(F)
    held = [d_v, d_f]
    try:
        runs = []
        for i in range(3):
            before = pb3d_gpu.device.sync_count()
            d_lab, d_vlab, d_counts, d_meas, t = pb3d_gpu.mesh_components_resident(d_f, len(F), len(V), d_v)
            assert i == 0 or pb3d_gpu.device.sync_count() - before == 2         # warm: the index check and the totals
            held += [d_lab, d_vlab, d_counts, d_meas]
            nc = t["components"]
            runs.append((t, d_lab.download((len(F),), np.int32).tobytes(), d_counts.download((5, nc), np.int64).tobytes(),
                         d_meas.download((2, nc), np.float64).tobytes()))
        assert runs[0] == runs[1] == runs[2]
    finally:
        for b in held:
            b.free()
