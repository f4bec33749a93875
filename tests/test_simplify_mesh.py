"""simplify_mesh and compact_mesh (pb3d/simplify.py, csrc/simplify.hip) against the NumPy restatement of tests/simplify_restate.py, and
that restatement against a plain per-face Python loop.  Every comparison is np.array_equal (vertices by their bytes): include/pb3d.h
states the result to the bit, so there is no tolerance anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import simplify_restate as sr
from pb3d import compact_mesh, simplify_mesh  # noqa: F401  (without the feature nothing in this file can run)

gpu = pytest.mark.gpu

DUPLICATES = ("drop", "keep")
FOLDED_SIZES = (2.0, 3.0, 4.0)


# ---- the cases: name -> (vertices, faces, voxel_size or None for compact_mesh, colors or None) -------------------------------------------
def _negative(F, nv, seed=4):
    F = F.copy()
    F[np.random.default_rng(seed).random(F.shape) < 0.5] -= nv
    return F


@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, arg = name.partition("/")
    if kind == "folded":
        return (*sr.folded_mesh(), float(arg), None)
    if kind == "ball":
        return (*sr.ball_mesh(), None if arg == "compact" else float(arg), None)
    if kind == "repeats":
        nf, _, how = arg.partition("/")
        return (*sr.repeats_mesh(int(nf)), 0.5 if how == "clustered" else None, None)
    if kind == "sheet":
        return (*sr.sheet_mesh(int(arg)), sr.SHEET_VOXEL, None)
    V, F = sr.folded_mesh()
    if kind == "f64i64":
        return V.astype(np.float64), F.astype(np.int64), float(arg), None
    if kind == "uint16":
        return V.astype(np.float16), F.astype(np.uint16), float(arg), None
    if kind == "negative":
        return V, _negative(F, len(V)), float(arg), None
    if kind == "unreferenced":
        return (*sr.with_unreferenced(V, F), float(arg), None)
    if kind == "reversed":
        return np.ascontiguousarray(V[::-1]), (len(V) - 1 - F).astype(F.dtype), float(arg), None
    assert kind == "colors"
    V, F, colors = sr.colored_mesh()
    if arg == "label":                                                          # one byte a vertex, as a label volume gives
        return V, F, 2.5, np.ascontiguousarray(colors[:, 2:])
    return V, F, None if arg == "compact" else float(arg), colors


CASES = ([f"folded/{vs}" for vs in FOLDED_SIZES] + ["ball/0.4", "ball/2.0", "ball/100.0", "ball/compact"]
         + [f"repeats/{nf}" for nf in sr.REPEAT_SIZES] + [f"repeats/{nf}/clustered" for nf in sr.REPEAT_SIZES]
         + [f"sheet/{side}" for side in sr.SHEET_SIDES]
         + ["f64i64/3.0", "uint16/3.0", "negative/3.0", "unreferenced/3.0", "reversed/3.0", "colors/2.0", "colors/compact", "colors/label"])
FIRST_TOO = ("folded/3.0", "ball/0.4", "f64i64/3.0", "unreferenced/3.0", "colors/2.0")      # the cases that also run with reduce = first


@functools.lru_cache(maxsize=None)
def want(name, duplicate_faces="drop", reduce="centroid"):
    """the restatement of a case, computed once and shared"""
    V, F, vs, colors = case(name)
    got = sr.restate(V, F, vs, None, reduce, duplicate_faces, colors)
    for a in got:
        if a is not None:
            a.setflags(write=False)
    return got


def settings(name):
    return [(d, r) for d in DUPLICATES for r in (("centroid", "first") if name in FIRST_TOO else ("centroid",))]


def same(got, ref, what):
    for g, w, part in zip(got, ref, sr.PARTS):
        assert (g is None) == (w is None), (what, part)
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g.view(np.uint8) if part == "vertices" else g, w.view(np.uint8) if part == "vertices" else w):
            bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
            raise AssertionError((what, part, "first differing row", int(bad[0]), "rows differing", len(bad), "of", len(g)))


# =====================================================================================================================
# CPU: the restatement against a loop, its invariants, the pinned counts; exports; validation
# =====================================================================================================================

@pytest.mark.parametrize("name", CASES)
def test_restatement_is_the_loop(name):
    V, F, _, colors = case(name)
    for dup, reduce in settings(name):
        same(want(name, dup, reduce), sr.loop(V, F, case(name)[2], None, reduce, dup, colors), (name, dup, reduce))


@pytest.mark.parametrize("name", CASES)
def test_restatement_invariants(name):
    V, F, _, colors = case(name)
    for dup, reduce in settings(name):
        verts, faces, cols, index, inverse, face_index = want(name, dup, reduce)
        n, m = len(verts), len(faces)
        assert verts.shape == (n, 3) and faces.shape == (m, 3) and index.shape == (n,) and inverse.shape == (len(V),) and face_index.shape == (m,)
        assert (np.diff(face_index) > 0).all() and (np.diff(index) > 0).all()
        assert np.array_equal(inverse[index], np.arange(n))
        assert m == 0 or (faces.min() >= 0 and faces.max() < n)
        assert np.array_equal(np.unique(faces), np.arange(n))                   # every output vertex is referenced
        assert (inverse >= -1).all() and (inverse < n).all()
        assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
        wrapped = np.where(F < 0, F + len(V), F)
        assert np.array_equal(inverse[wrapped[face_index]], faces)              # the caller's corner order
        assert (cols is None) == (colors is None) and (cols is None or np.array_equal(cols, colors[index]))
        if dup == "drop":
            k = np.argmin(faces, axis=1)
            rot = np.stack([faces[np.arange(m), (k + a) % 3] for a in range(3)], axis=1)
            assert len(np.unique(rot, axis=0)) == m


def test_pinned_counts():
    V, F = sr.folded_mesh()
    assert V.shape == (4570, 3) and F.shape == (10648, 3) and V.dtype == np.float32 and F.dtype == np.int32 and sr.edge_balanced(F)
    for vs, n, m_drop, m_keep in ((2.0, 507, 2235, 2256), (3.0, 212, 1084, 1142), (4.0, 110, 642, 718)):
        drop, keep = want(f"folded/{vs}", "drop"), want(f"folded/{vs}", "keep")
        assert (len(drop[0]), len(drop[1]), len(keep[0]), len(keep[1])) == (n, m_drop, n, m_keep)
        assert sr.edge_balanced(keep[1]) and not sr.edge_balanced(drop[1])      # keep stays closed; drop opens the folded parts
        assert np.array_equal(drop[0].view(np.uint8), keep[0].view(np.uint8)) and set(drop[5].tolist()) < set(keep[5].tolist())
    V, F = sr.ball_mesh()
    assert V.shape == (1536, 3) and F.shape == (3068, 3) and sr.edge_balanced(F)
    assert (len(want("ball/2.0")[0]), len(want("ball/2.0")[1])) == (341, 678)
    assert (len(want("ball/100.0")[0]), len(want("ball/100.0")[1])) == (0, 0) and (want("ball/100.0")[4] == -1).all()


def test_ball_of_single_vertex_clusters():
    """below the half-voxel lattice's spacing every vertex is its own cluster: simplify_mesh is compact_mesh, and with reduce = first
    (centroids of one float32 vertex are that vertex too) the input comes back byte for byte"""
    V, F = sr.ball_mesh()
    for dup in DUPLICATES:
        for reduce in ("centroid", "first"):
            got = want("ball/0.4", dup, reduce)
            same(got, want("ball/compact", dup), ("ball", dup, reduce))
            assert got[0].tobytes() == V.tobytes() and got[1].tobytes() == F.tobytes()
            assert np.array_equal(got[3], np.arange(len(V))) and np.array_equal(got[5], np.arange(len(F)))


def by_hand(name, got):
    """what the hand-made faces of sr.repeats_mesh must come to"""
    V, F, _, _ = case(name)
    nf = len(F)
    verts, faces, _, index, inverse, face_index = got["drop"]
    kept = face_index.tolist()
    assert kept[0] == 0 and sr.MIRROR_AT in kept and sr.ROTATION_AT not in kept and nf - 1 not in kept, name
    a, b, c = (int(inverse[v]) for v in sr.RESERVED)
    assert faces[0].tolist() == [a, b, c] and faces[kept.index(sr.MIRROR_AT)].tolist() == [a, c, b], name      # their own corner order
    assert int((np.sort(faces, axis=1) == sorted((a, b, c))).all(axis=1).sum()) == 2, name
    keep_index = got["keep"][5].tolist()
    assert {0, sr.MIRROR_AT, sr.ROTATION_AT, nf - 1} <= set(keep_index) and len(keep_index) == nf, name
    assert len(kept) < nf - 2, name                                              # the random triples repeat too


@pytest.mark.parametrize("nf", sr.REPEAT_SIZES)
def test_repeats_by_hand(nf):
    for name in (f"repeats/{nf}", f"repeats/{nf}/clustered"):
        by_hand(name, {dup: want(name, dup) for dup in DUPLICATES})
    same(want(f"repeats/{nf}/clustered"), want(f"repeats/{nf}"), nf)             # one vertex per cluster: the same mesh


def test_sheet_cases_reach_every_pass_count():
    for side, passes in zip(sr.SHEET_SIDES, (1, 2, 2, 3)):
        V, F = sr.sheet_mesh(side)
        clusters = side * side                                                  # keys 0 .. clusters: the collapsed faces' key is the last
        assert len(np.unique(want(f"sheet/{side}", "keep")[4])) == clusters and (clusters.bit_length() + 7) // 8 == passes
        drop, keep = want(f"sheet/{side}", "drop"), want(f"sheet/{side}", "keep")
        square = 2 * (side - 1) ** 2
        assert len(keep[1]) == len(F) and len(drop[1]) == square + len(range(0, min(300, square), 7))      # the mirror images stay
        assert (drop[5][:square] == np.arange(square)).all()


def test_indices_dtypes_and_order():
    base = want("folded/3.0")
    same(want("negative/3.0"), base, "negative")
    wide = want("f64i64/3.0")
    assert wide[0].dtype == np.float64 and wide[1].dtype == np.int64 and np.array_equal(wide[1], base[1])
    small = want("uint16/3.0")
    assert small[0].dtype == np.float64 and small[1].dtype == np.int64
    # unreferenced vertices: they join clusters and centroids, and the clusters made only of them vanish
    V, F, vs, _ = case("unreferenced/3.0")
    verts, faces, _, index, inverse, face_index = want("unreferenced/3.0")
    named = np.zeros(len(V), bool)
    named[F.reshape(-1)] = True
    assert int((~named).sum()) == 1524
    joined = np.unique(inverse[~named & (inverse >= 0)])
    assert len(joined) > 50 and int((inverse[~named] == -1).sum()) > 500
    origin = V.min(axis=0).astype(np.float64) - 1.5                             # one grid for both: the faces that stay are the same
    plain, moved = sr.restate(V[named], np.cumsum(named)[F] - 1, vs, origin=origin), sr.restate(V, F, vs, origin=origin)
    assert len(plain[0]) == len(moved[0]) and np.array_equal(plain[5], moved[5])
    assert len({r.tobytes() for r in moved[0]} - {r.tobytes() for r in plain[0]}) > 50     # ... and the centroids are not
    # reversed vertex order: the same partition, another numbering
    fwd, rev = want("folded/3.0"), want("reversed/3.0")
    assert len(fwd[0]) == len(rev[0]) and len(fwd[1]) == len(rev[1]) and not np.array_equal(fwd[1], rev[1])
    pairs = np.unique(np.stack([fwd[4], rev[4][::-1]], 1), axis=0)
    assert len(pairs) == len(np.unique(fwd[4])) == len(np.unique(rev[4]))
    for bad in (len(V), -len(V) - 1):
        G = F.copy()
        G[len(G) // 2, 1] = bad
        for fn in (sr.restate, sr.loop):
            with pytest.raises(IndexError):
                fn(V, G, vs)


def test_colours_name_a_vertex_of_the_cluster():
    V, F, colors = sr.colored_mesh()
    assert len(np.unique(colors, axis=0)) == 267                                 # of some 280 occupied voxels: the colours tell them apart
    for name in ("colors/2.0", "colors/compact", "colors/label"):
        for dup in DUPLICATES:
            verts, faces, cols, index, inverse, _ = want(name, dup)
            given = case(name)[3]
            assert cols.dtype == np.uint8 and cols.shape == (len(verts), given.shape[1]) and np.array_equal(cols, given[index])
            for k in range(0, len(verts), 7):
                assert cols[k].tolist() in given[inverse == k].tolist()


def test_exports():
    import pb3d
    for n in ("simplify_mesh", "simplify_mesh_resident", "compact_mesh", "compact_mesh_resident"):
        assert callable(getattr(pb3d, n)) and n in pb3d.simplify.__all__
    for s in ("pb3d_mesh_simplify_resident", "pb3d_mesh_compact_resident", "pb3d_simplify_last"):
        assert s in pb3d._lib.EXPORTED_SYMBOLS


def test_validation_needs_no_device():
    import pb3d
    V = np.zeros((4, 3))
    F = np.array([[0, 1, 2]])
    for bad in (np.nan, np.inf, -np.inf):
        p = V.copy()
        p[3, 1] = bad                                                           # a vertex no face names
        with pytest.raises(ValueError, match="NaN or infinity"):
            pb3d.simplify_mesh(p, F, 0.1)
    for vs in (0.0, -1.0, np.nan, np.inf):
        for fn in (lambda: pb3d.simplify_mesh(V, F, vs), lambda: pb3d.simplify_mesh_resident(None, 4, None, 1, vs)):
            with pytest.raises(ValueError, match="voxel_size must be finite and > 0"):
                fn()
    for origin in ((0.0, np.nan, 0.0), (0.0, 0.0), 1.0):
        for fn in (lambda: pb3d.simplify_mesh(V, F, 0.1, origin=origin), lambda: pb3d.simplify_mesh_resident(None, 4, None, 1, 0.1, origin=origin)):
            with pytest.raises(ValueError, match="origin must be three finite values"):
                fn()
    for reduce in ("mean", None, 0):
        for fn in (lambda: pb3d.simplify_mesh(V, F, 0.1, reduce=reduce), lambda: pb3d.simplify_mesh_resident(None, 4, None, 1, 0.1, reduce=reduce)):
            with pytest.raises(ValueError, match="reduce must be 'centroid' or 'first'"):
                fn()
    for dup in ("merge", None, 0, True):
        for fn in (lambda: pb3d.simplify_mesh(V, F, 0.1, duplicate_faces=dup), lambda: pb3d.compact_mesh(V, F, duplicate_faces=dup),
                   lambda: pb3d.simplify_mesh_resident(None, 4, None, 1, 0.1, duplicate_faces=dup),
                   lambda: pb3d.compact_mesh_resident(None, 4, None, 1, duplicate_faces=dup)):
            with pytest.raises(ValueError, match="duplicate_faces must be 'drop' or 'keep'"):
                fn()
    for fn in (lambda c: pb3d.simplify_mesh(V, F, 0.1, colors=c), lambda c: pb3d.compact_mesh(V, F, colors=c)):
        with pytest.raises(TypeError, match="uint8"):
            fn(np.zeros((4, 3), np.float32))
        for shape in ((4,), (4, 2), (3, 3), (4, 3, 1)):
            with pytest.raises(ValueError, match="colors must have shape"):
                fn(np.zeros(shape, np.uint8))
    for fn in (lambda: pb3d.simplify_mesh_resident(None, 4, None, 1, 0.1, channels=2), lambda: pb3d.compact_mesh_resident(None, 4, None, 1, channels=0)):
        with pytest.raises(ValueError, match="channels must be 1 or 3"):
            fn()
    for fn in (lambda v, f: pb3d.simplify_mesh(v, f, 0.1), pb3d.compact_mesh):
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
    for fn in (lambda: pb3d.simplify_mesh_resident(None, 2 ** 31, None, 1, 0.1), lambda: pb3d.compact_mesh_resident(None, 2 ** 31, None, 1)):
        with pytest.raises(ValueError, match="at most 2\\^31 - 1 vertices"):
            fn()


def test_no_faces_needs_no_device():
    import pb3d
    for vdt, fdt in ((np.float32, np.int32), (np.float64, np.int64), (np.int16, np.uint8)):
        V, F = np.ones((5, 3), vdt), np.zeros((0, 3), fdt)
        for got in (pb3d.simplify_mesh(V, F, 0.1, colors=np.zeros((5, 1), np.uint8), return_index=True, return_inverse=True, return_face_index=True),
                    pb3d.compact_mesh(V, F, colors=np.zeros((5, 1), np.uint8), return_index=True, return_inverse=True, return_face_index=True)):
            same(got, sr.restate(V, F, 0.1, colors=np.zeros((5, 1), np.uint8)), (vdt, fdt))
        assert len(pb3d.simplify_mesh(V, F, 0.1)) == 2 and len(pb3d.compact_mesh(V, F, return_inverse=True)) == 3
    same(pb3d.compact_mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int32), return_index=True, return_inverse=True, return_face_index=True)[:2],
         sr.restate(np.zeros((0, 3)), np.zeros((0, 3), np.int32))[:2], "nothing")


def test_cabi_refusals_need_no_device():
    import pb3d
    lib = pb3d._lib.load()
    one, two = C.c_void_p(256), C.c_void_p(512)
    counts = (C.c_int64 * 2)(7, 7)
    simplify, compact = lib.pb3d_mesh_simplify_resident, lib.pb3d_mesh_compact_resident

    def refused(rc, text):
        assert rc == -1 and text in lib.pb3d_last_error().decode(), (rc, lib.pb3d_last_error())

    def both(nv, nf, dup, colors, channels, out_v, out_f, out_c, cnt, text, verts=one, faces=one):
        refused(simplify(None, verts, 0, nv, faces, 0, nf, 0.5, None, 0, dup, colors, channels, out_v, out_f, out_c, None, None, None, cnt), text)
        refused(compact(None, verts, 0, nv, faces, 0, nf, dup, colors, channels, out_v, out_f, out_c, None, None, None, cnt), text)

    both(-1, 1, 0, None, 3, two, two, None, counts, "negative count")
    both(5, 2 ** 31, 0, None, 3, two, two, None, counts, "at most 2^31 - 1")
    both(5, 2, 2, None, 3, two, two, None, counts, "duplicate_faces must be 0 (drop) or 1 (keep)")
    both(5, 2, 0, None, 3, two, two, None, None, "null argument")
    both(5, 2, 0, one, 2, two, two, two, counts, "channels must be 1 or 3")
    both(5, 2, 0, None, 3, two, two, None, counts, "null buffer", verts=None)
    both(5, 2, 0, None, 3, None, two, None, counts, "null buffer")
    both(5, 2, 0, one, 3, two, two, None, counts, "null buffer")                # colours in, no room for colours out
    both(5, 2, 0, None, 3, one, two, None, counts, "may not alias")
    both(5, 2, 0, None, 3, two, two, None, counts, "null context")
    both(0, 0, 1, None, 3, None, None, None, counts, "null context", verts=None, faces=None)        # an empty mesh needs no buffers
    for vs in (0.0, -0.5, float("nan"), float("inf")):
        refused(simplify(None, one, 0, 5, one, 0, 2, vs, None, 0, 0, None, 3, two, two, None, None, None, None, counts), "voxel_size must be finite and > 0")
    o = (C.c_double * 3)(0.0, float("nan"), 0.0)
    refused(simplify(None, one, 0, 5, one, 0, 2, 0.5, o, 0, 0, None, 3, two, two, None, None, None, None, counts), "origin must be finite")
    refused(simplify(None, one, 0, 5, one, 0, 2, 0.5, None, 2, 0, None, 3, two, two, None, None, None, None, counts), "reduce must be 0 (centroid) or 1 (first)")
    refused(lib.pb3d_simplify_last(None, counts, None), "null argument")
    assert list(counts) == [7, 7]                                               # a refusal writes nothing


# =====================================================================================================================
# GPU
# =====================================================================================================================

ALL = dict(return_index=True, return_inverse=True, return_face_index=True)


def via_numpy(pb3d, name, dup, reduce):
    V, F, vs, colors = case(name)
    if vs is None:
        got = pb3d.compact_mesh(V, F, duplicate_faces=dup, colors=colors, **ALL)
    else:
        got = pb3d.simplify_mesh(V, F, case(name)[2], reduce=reduce, duplicate_faces=dup, colors=colors, **ALL)
    return got if colors is not None else (got[0], got[1], None, *got[2:])


def download(bufs, counts, nv, vdt, fdt, channels):
    """the buffers of a resident form in the NumPy form's types"""
    n, m = counts
    return (bufs[0].download((n, 3), vdt), bufs[1].download((m, 3), fdt), bufs[2].download((n, channels)) if bufs[2] is not None else None,
            bufs[3].download((n,), np.int32).astype(np.intp), bufs[4].download((nv,), np.int32).astype(np.intp),
            bufs[5].download((m,), np.int32).astype(np.intp))


def via_resident(pb3d, name, dup, reduce):
    V, F, vs, colors = case(name)
    V, F = np.ascontiguousarray(V), np.ascontiguousarray(F)
    assert V.dtype in (np.float32, np.float64) and F.dtype in (np.int32, np.int64)
    held = [pb3d.device.from_numpy(V), pb3d.device.from_numpy(F)] + ([pb3d.device.from_numpy(colors)] if colors is not None else [])
    try:
        kw = dict(duplicate_faces=dup, d_colors=held[2] if colors is not None else None, channels=colors.shape[1] if colors is not None else 3,
                  verts_f64=V.dtype == np.float64, faces_i64=F.dtype == np.int64)
        if vs is None:
            *bufs, counts = pb3d.compact_mesh_resident(held[0], len(V), held[1], len(F), **kw)
        else:
            *bufs, counts = pb3d.simplify_mesh_resident(held[0], len(V), held[1], len(F), case(name)[2], reduce=reduce, **kw)
        held += [b for b in bufs if b is not None]
        return download(bufs, counts, len(V), V.dtype, F.dtype, kw["channels"])
    finally:
        for b in held:
            b.free()


@gpu
@pytest.mark.parametrize("name", CASES)
def test_device_is_the_restatement(pb3d_gpu, name):
    resident = name != "uint16/3.0"                                             # the resident forms take the four dtypes of the kernels
    for dup, reduce in settings(name):
        same(via_numpy(pb3d_gpu, name, dup, reduce), want(name, dup, reduce), (name, dup, reduce, "numpy"))
        if resident and reduce == "centroid":
            same(via_resident(pb3d_gpu, name, dup, reduce), want(name, dup, reduce), (name, dup, reduce, "resident"))


@gpu
@pytest.mark.parametrize("vs", FOLDED_SIZES)
def test_keep_stays_closed(pb3d_gpu, vs):
    """the edge balance of the device's own output: kept under duplicate_faces = keep, lost under drop where the thin parts fold"""
    V, F = sr.folded_mesh()
    verts, faces = pb3d_gpu.simplify_mesh(V, F, vs, duplicate_faces="keep")
    assert sr.edge_balanced(F) and sr.edge_balanced(faces) and len(faces) == len(want(f"folded/{vs}", "keep")[1])
    verts, faces = pb3d_gpu.simplify_mesh(V, F, vs, duplicate_faces="drop")
    assert not sr.edge_balanced(faces) and len(faces) == len(want(f"folded/{vs}", "drop")[1])


@gpu
def test_ball(pb3d_gpu):
    V, F = sr.ball_mesh()
    for dup in DUPLICATES:
        compact = pb3d_gpu.compact_mesh(V, F, duplicate_faces=dup, **ALL)
        for reduce in ("centroid", "first"):
            got = pb3d_gpu.simplify_mesh(V, F, 0.4, reduce=reduce, duplicate_faces=dup, **ALL)
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, compact))
            assert got[0].tobytes() == V.tobytes() and got[1].tobytes() == F.tobytes()
        verts, faces, inverse = pb3d_gpu.simplify_mesh(V, F, 100.0, duplicate_faces=dup, return_inverse=True)
        assert verts.shape == (0, 3) and faces.shape == (0, 3) and verts.dtype == np.float32 and faces.dtype == np.int32 and (inverse == -1).all()
    assert len(pb3d_gpu.simplify_mesh(V, F, 2.0)[0]) == 341 and len(pb3d_gpu.simplify_mesh(V, F, 2.0)[1]) == 678


@gpu
@pytest.mark.parametrize("nf", sr.REPEAT_SIZES)
def test_repeats_on_the_device(pb3d_gpu, nf):
    for name in (f"repeats/{nf}", f"repeats/{nf}/clustered"):
        by_hand(name, {dup: via_numpy(pb3d_gpu, name, dup, "centroid") for dup in DUPLICATES})


OUT_FILL = 0xA5


@gpu
def test_bad_index_writes_nothing(pb3d_gpu):
    """an index == nv and an index < -nv, in int32 and int64 faces: the library's index error (IndexError in Python) and no output byte
    touched; so for a face list with no vertices at all"""
    L = pb3d_gpu._lib
    lib, ctx = L.load(), L.ctx()
    V, F = sr.ball_mesh()
    nv, nf = len(V), len(F)
    d_v = pb3d_gpu.device.from_numpy(V)
    outs = [pb3d_gpu.device.DeviceBuffer(n) for n in (nv * 12, nf * 24, nv * 4, nv * 4, nf * 4)]
    try:
        for fdt in (np.int32, np.int64):
            for bad in (nv, -nv - 1):
                G = F.astype(fdt)
                G[nf - 1, 2] = bad
                for fn in (lambda: pb3d_gpu.simplify_mesh(V, G, 2.0), lambda: pb3d_gpu.compact_mesh(V, G)):
                    with pytest.raises(IndexError, match="out of bounds"):
                        fn()
                d_f = pb3d_gpu.device.from_numpy(G)
                try:
                    for entry in ("simplify", "compact"):
                        for b in outs:
                            b.upload(np.full(b.nbytes, OUT_FILL, np.uint8))
                        counts = (C.c_int64 * 2)(-3, -3)
                        ptrs = [C.c_void_p(b.ptr) for b in outs]
                        head = (ctx, C.c_void_p(d_v.ptr), 0, nv, C.c_void_p(d_f.ptr), int(fdt == np.int64), nf)
                        tail = (0, None, 3, ptrs[0], ptrs[1], None, ptrs[2], ptrs[3], ptrs[4], counts)
                        rc = (lib.pb3d_mesh_simplify_resident(*head, 2.0, None, 0, *tail) if entry == "simplify"
                              else lib.pb3d_mesh_compact_resident(*head, *tail))
                        assert rc == -6 and b"index out of bounds" in lib.pb3d_last_error(), (entry, fdt, bad, rc)
                        assert list(counts) == [-3, -3]
                        for b in outs:
                            assert (b.download((b.nbytes,)) == OUT_FILL).all(), (entry, fdt, bad, "an output was written")
                finally:
                    d_f.free()
        counts = (C.c_int64 * 2)(-3, -3)
        d_f = pb3d_gpu.device.from_numpy(F)
        try:
            rc = lib.pb3d_mesh_compact_resident(ctx, None, 0, 0, C.c_void_p(d_f.ptr), 0, nf, 0, None, 3, None, None, None, None, None, None, counts)
            assert rc == -6 and list(counts) == [-3, -3]
        finally:
            d_f.free()
    finally:
        for b in [d_v] + outs:
            b.free()


@gpu
def test_colours_on_the_device(pb3d_gpu):
    """index_grid's colours name a vertex's lattice voxel: the device's meshify gives the mesh and the bytes, and every output colour is
    the colour of the cluster's first vertex -- a vertex of that cluster"""
    import meshify_cases as mc
    V, F, colors = sr.colored_mesh()
    occ = np.zeros((10, 10, 10), bool)
    occ[1:9, 1:9, 1:9] = np.random.default_rng(17).random((8, 8, 8)) < 0.55
    grid = np.ascontiguousarray(mc.index_grid(occ))
    d_grid = pb3d_gpu.device.from_numpy(grid)
    try:
        (dv, df, dn, dc), (n, m) = pb3d_gpu.device.meshify(d_grid, grid.shape, download=False)
        held = [dv, df, dn, dc]
        try:
            assert np.array_equal(dv.download((n, 3), np.float32), V) and np.array_equal(df.download((m, 3), np.int32), F)
            assert np.array_equal(dc.download((n, 3)), colors)
            for dup in DUPLICATES:
                *bufs, counts = pb3d_gpu.simplify_mesh_resident(dv, n, df, m, 2.0, duplicate_faces=dup, d_colors=dc, channels=3)
                held += bufs
                got = download(bufs, counts, n, np.float32, np.int32, 3)
                same(got, want("colors/2.0", dup), ("meshify buffers", dup))
                assert np.array_equal(got[2], colors[got[3]])
                for k in range(len(got[0])):
                    assert got[2][k].tolist() in colors[got[4] == k].tolist()
        finally:
            for b in held:
                b.free()
    finally:
        d_grid.free()


@gpu
def test_composition(pb3d_gpu):
    """what comes out is a mesh the other mesh entries take: adjacency and one smoothing step raise no index error, every vertex has a
    neighbour, and voxelize_mesh takes the keep output"""
    V, F = sr.folded_mesh()
    for dup in DUPLICATES:
        verts, faces = pb3d_gpu.simplify_mesh(V, F, 2.0, duplicate_faces=dup)
        starts, neighbours = pb3d_gpu.mesh_vertex_adjacency(faces, len(verts))
        assert (np.diff(starts) >= 2).all() and neighbours.max() == len(verts) - 1
        smooth = pb3d_gpu.smooth_mesh(verts, faces, iterations=1)
        assert smooth.shape == verts.shape and smooth.dtype == verts.dtype and np.isfinite(smooth).all()
    verts, faces = pb3d_gpu.simplify_mesh(V, F, 2.0, duplicate_faces="keep")
    solid = pb3d_gpu.voxelize_mesh(verts, faces, (16, 16, 16))
    assert solid.shape == (16, 16, 16) and solid.any()


@gpu
def test_resident_runs_twice_alike(pb3d_gpu):
    """straight from meshify(download=False)'s buffers (float32 vertices, int32 faces, n x 3 bytes); two runs give equal bytes"""
    V, F = sr.folded_mesh()
    mask = np.zeros((16, 16, 16), np.uint8)
    mask[1:15, 1:15, 1:15] = np.random.default_rng(3).random((14, 14, 14)) < 0.5
    grid = np.ascontiguousarray(np.repeat(mask[..., None] * 200, 3, axis=-1).astype(np.uint8))
    d_grid = pb3d_gpu.device.from_numpy(grid)
    held = [d_grid]
    try:
        (dv, df, dn, dc), (n, m) = pb3d_gpu.device.meshify(d_grid, grid.shape, download=False)
        held += [dv, df, dn, dc]
        assert (n, m) == (len(V), len(F))
        Vd, Fd, Cd = dv.download((n, 3), np.float32), df.download((m, 3), np.int32), dc.download((n, 3))
        for dup in DUPLICATES:
            runs = []
            for rep in range(2):
                *bufs, counts = pb3d_gpu.simplify_mesh_resident(dv, n, df, m, 3.0, duplicate_faces=dup, d_colors=dc, channels=3)
                held += bufs
                runs.append(download(bufs, counts, n, np.float32, np.int32, 3))
            assert [a.tobytes() for a in runs[0]] == [a.tobytes() for a in runs[1]]
            same(runs[0], sr.restate(Vd, Fd, 3.0, None, "centroid", dup, Cd), ("meshify", dup))
    finally:
        for b in held:
            b.free()


@gpu
def test_host_waits_and_last(pb3d_gpu):
    """once the scratch is warm: the index check, voxel_downsample's two and the read-back of the two counts for simplify_mesh, the
    index check and the read-back for compact_mesh; nf = 0 waits for nothing.  pb3d_simplify_last has the counts, and the pass times
    only under the knob"""
    L = pb3d_gpu._lib
    lib, ctx = L.load(), L.ctx()
    V, F = sr.ball_mesh()
    nv, nf = len(V), len(F)
    held = [pb3d_gpu.device.from_numpy(V), pb3d_gpu.device.from_numpy(F)]
    last, ms = (C.c_int64 * 3)(), (C.c_double * 5)()
    try:
        for dup in DUPLICATES:
            for rep in range(2):
                before = pb3d_gpu.device.sync_count()
                *bufs, counts = pb3d_gpu.simplify_mesh_resident(held[0], nv, held[1], nf, 2.0, duplicate_faces=dup)
                waits = pb3d_gpu.device.sync_count() - before
                held += [b for b in bufs if b is not None]
            assert waits == 4 and counts == (341, 678), (dup, waits, counts)
            L.check(lib.pb3d_simplify_last(ctx, last, None))
            assert last[1] == 341 and last[2] == 678 and last[0] == len(np.unique(dr_inverse(V, 2.0)))
            assert lib.pb3d_simplify_last(ctx, last, ms) == -1 and b"simplify_timing" in lib.pb3d_last_error()
            for rep in range(2):
                before = pb3d_gpu.device.sync_count()
                *bufs, counts = pb3d_gpu.compact_mesh_resident(held[0], nv, held[1], nf, duplicate_faces=dup)
                waits = pb3d_gpu.device.sync_count() - before
                held += [b for b in bufs if b is not None]
            assert waits == 2 and counts == (nv, nf), (dup, waits, counts)
            L.check(lib.pb3d_simplify_last(ctx, last, None))
            assert list(last) == [nv, nv, nf]
        before = pb3d_gpu.device.sync_count()
        *bufs, counts = pb3d_gpu.simplify_mesh_resident(held[0], nv, None, 0, 2.0)
        held += [b for b in bufs if b is not None]
        assert counts == (0, 0) and pb3d_gpu.device.sync_count() == before
        assert (bufs[4].download((nv,), np.int32) == -1).all()
        L.set_tuning("simplify_timing", 1)
        try:
            *bufs, counts = pb3d_gpu.simplify_mesh_resident(held[0], nv, held[1], nf, 2.0)
            held += [b for b in bufs if b is not None]
            L.check(lib.pb3d_simplify_last(ctx, last, ms))
            assert counts == (341, 678) and all(t >= 0.0 for t in ms) and sum(ms) > 0.0
        finally:
            L.set_tuning("simplify_timing", 0)
    finally:
        for b in held:
            b.free()


def dr_inverse(V, voxel_size):
    import downsample_restate as dr
    return dr.restate(V, voxel_size)[2]
