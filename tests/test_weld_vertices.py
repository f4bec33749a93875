"""weld_vertices (pb3d/weld.py, csrc/weld.hip) against the NumPy restatement of tests/weld_restate.py, that restatement against a plain
dictionary loop, and the chain soup -> weld_vertices -> mesh_topology -> orient_mesh.  Every comparison is by bytes: include/pb3d.h
states the result to the bit, so there is no tolerance anywhere."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import mesh_restate as me
import meshcomp_restate as mc
import orient_restate as orr
import simplify_restate as sr
import voxelize_restate as vr
import weld_restate as wr
from pb3d import weld_vertices  # noqa: F401  (without the feature nothing in this file can run)

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEAM_SIZES = (2047, 2048, 2049, 4097)           # vertices: the sort's tile is 2048 pairs


@functools.lru_cache(maxsize=None)
def mc_mesh():
    v, f, _ = me.marching_cubes_binary(vr.random_mask((12, 10, 11), 0.35, 3))
    return sr._frozen(v, f)


# ---- the cases: name -> (vertices, faces or None, colors or None) ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, arg = name.partition("/")
    if kind == "soup":
        V, F = wr.soup(*(mc_mesh() if arg == "mc" else mc.fragments_mesh()))
        return V, F, None
    if kind == "distinct":
        return wr.distinct(int(arg)), None, None
    if kind == "equal":
        return wr.all_equal(int(arg)), None, None
    if kind == "zeros":
        return wr.zero_pair(), np.array([[0, 1, 2], [3, 4, -1], [-5, 2, 3]], np.int32), None
    if kind == "subnormals":
        return wr.subnormals(np.float32 if arg == "32" else np.float64), None, None
    if kind == "words":
        return wr.word_neighbours(), None, None
    if kind == "float16":                                                       # becomes float64: equality is float64's, which is float16's
        return wr.soup(*mc_mesh())[0].astype(np.float16), None, None
    if kind == "integer":
        return (np.arange(3 * 700).reshape(700, 3) % 11).astype(np.int16), None, None
    V, F = wr.soup(*mc_mesh())
    if kind == "colors":
        c = np.random.default_rng(6).integers(0, 256, (len(V), int(arg)), dtype=np.uint8)
        return V, F, c
    if kind == "unreferenced":                                                  # duplicates no face names, in front and behind
        extra = np.concatenate([V[5:9], [[9.5, 9.5, 9.5]], V[:2]])
        return np.concatenate([extra[:3], V, extra[3:]]).astype(V.dtype), (F + 3).astype(np.int32), None
    if kind == "int64":
        return V.astype(np.float64) * np.pi, F.astype(np.int64), None
    if kind == "uint16":
        return V[:3 * 2000], F[:2000].astype(np.uint16), None
    assert kind == "negative"
    G = F.astype(np.int64)
    G[np.random.default_rng(4).random(G.shape) < 0.5] -= len(V)
    return V.astype(np.float64), G, None


SOUPS = ["soup/mc", "soup/fragments"]
SEAMS = [f"{k}/{n}" for n in SEAM_SIZES for k in ("distinct", "equal")]
BITS = ["zeros", "subnormals/32", "subnormals/64", "words", "float16", "integer"]
EXTRAS = ["colors/1", "colors/3", "unreferenced", "int64", "uint16", "negative"]
CASES = SOUPS + SEAMS + BITS + EXTRAS


@functools.lru_cache(maxsize=None)
def want(name):
    r = wr.restate(*case(name))
    for a in r.values():
        if a is not None:
            a.setflags(write=False)
    return r


def same_result(got, ref, what):
    assert list(got) == list(ref)
    for part in ref:
        g, w = got[part], ref[part]
        assert (g is None) == (w is None), (what, part)
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1)).any(1))
            raise AssertionError((what, part, "first differing row", int(bad[0]), g[bad[0]], w[bad[0]], "differing", len(bad), "of", len(g)))


def on_device(pb3d, name):
    V, F, c = case(name)
    out = list(pb3d.weld_vertices(V, F, c, return_index=True, return_inverse=True, return_counts=True))
    verts = out.pop(0)
    faces = out.pop(0) if F is not None else None
    colors = out.pop(0) if c is not None else None
    index, inverse, counts = out
    return dict(vertices=verts, faces=faces, colors=colors, index=index, inverse=inverse, counts=counts)


# =====================================================================================================================
# CPU
# =====================================================================================================================

@pytest.mark.parametrize("name", CASES)
def test_restatement_is_the_loop(name):
    same_result(want(name), wr.loop(*case(name)), name)


@pytest.mark.parametrize("name", CASES)
def test_restatement_invariants(name):
    V, F, c = case(name)
    r = want(name)
    W = np.asarray(V, np.float32 if np.asarray(V).dtype == np.float32 else np.float64)
    m = len(r["vertices"])
    assert (np.diff(r["index"]) > 0).all() and r["counts"].sum() == len(W) and (r["counts"] >= 1).all()      # first appearance
    assert np.array_equal(r["inverse"][r["index"]], np.arange(m)) and (r["index"][r["inverse"]] <= np.arange(len(W))).all()
    assert (r["vertices"][r["inverse"]] == W).all() and r["vertices"].tobytes() == W[r["index"]].tobytes()
    assert len(np.unique(r["vertices"] + W.dtype.type(0), axis=0)) == m         # no two output rows are equal
    if F is not None:
        assert r["faces"].dtype == F.dtype and r["faces"].min() >= 0 and (r["vertices"][r["faces"]] == W[F]).all()
    again = wr.restate(r["vertices"], r["faces"], r["colors"])                  # welding a welded mesh changes nothing
    assert again["vertices"].tobytes() == r["vertices"].tobytes() and np.array_equal(again["index"], np.arange(m))
    assert F is None or np.array_equal(again["faces"], r["faces"])


def test_pinned_facts():
    r = want("zeros")
    assert r["index"].tolist() == [0, 1, 4] and r["inverse"].tolist() == [0, 1, 0, 0, 2] and r["counts"].tolist() == [3, 1, 1]
    assert np.signbit(r["vertices"][0]).tolist() == [True, False, False] and r["faces"].tolist() == [[0, 1, 0], [0, 2, 2], [0, 0, 0]]
    assert len(want("subnormals/32")["vertices"]) == len(want("subnormals/64")["vertices"]) == 5
    assert len(want("words")["vertices"]) == 16 and want("words")["counts"].tolist() == [3 if i % 3 == 0 else 2 for i in range(16)]
    V, F = mc_mesh()
    r = want("soup/mc")
    assert (len(V), len(F), len(r["vertices"])) == (1079, 2462, 1079) and r["counts"].sum() == 3 * 2462
    assert mc.restate(r["faces"], 1079)["totals"] == mc.restate(F, 1079)["totals"]                  # the soup welds back to the mesh's topology
    assert mc.restate(case("soup/mc")[1], 3 * 2462)["totals"]["components"] == 2462
    r = want("soup/fragments")
    assert len(r["vertices"]) == 2608 and mc.restate(r["faces"], 2608)["totals"]["components"] == 43
    for n in SEAM_SIZES:
        assert len(want(f"distinct/{n}")["vertices"]) == n and want(f"equal/{n}")["counts"].tolist() == [n]
    assert len(want("unreferenced")["vertices"]) == 1080


def test_exports():
    import pb3d
    for n in ("weld_vertices", "weld_vertices_resident"):
        assert callable(getattr(pb3d, n)) and n in pb3d.weld.__all__
    header = open(os.path.join(ROOT, "include", "pb3d.h")).read()
    assert "pb3d_weld_vertices_resident" in pb3d._lib.EXPORTED_SYMBOLS and re.search(r"^int\s+pb3d_weld_vertices_resident\s*\(", header, re.M)


def test_validation_needs_no_device():
    import pb3d
    V = np.zeros((4, 3))
    F = np.array([[0, 1, 2]])
    for bad in (np.nan, np.inf, -np.inf):
        p = V.copy()
        p[3, 1] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            pb3d.weld_vertices(p)
        with pytest.raises(ValueError, match="NaN or infinity"):
            pb3d.weld_vertices(p, F)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        pb3d.weld_vertices(np.zeros((4, 2)), F)
    with pytest.raises(TypeError):
        pb3d.weld_vertices(np.zeros((4, 3), complex))
    with pytest.raises(ValueError, match=r"\(m, 3\)"):
        pb3d.weld_vertices(V, np.zeros((2, 4), np.int32))
    with pytest.raises(IndexError):
        pb3d.weld_vertices(V, np.zeros((1, 3)))                                 # float indices
    with pytest.raises(IndexError):
        pb3d.weld_vertices(np.zeros((0, 3)), F)                                 # no vertex, one face
    with pytest.raises(IndexError):
        pb3d.weld_vertices(V, np.array([[0, 1, 4]], np.uint32))
    for c in (np.zeros((4, 2), np.uint8), np.zeros((3, 3), np.uint8), np.zeros(4, np.uint8)):
        with pytest.raises(ValueError, match="colors must have shape"):
            pb3d.weld_vertices(V, F, c)
    with pytest.raises(TypeError):
        pb3d.weld_vertices(V, F, np.zeros((4, 3)))
    with pytest.raises(ValueError, match="channels must be 1 or 3"):
        pb3d.weld_vertices_resident(None, 4, channels=2)
    with pytest.raises(ValueError, match="at most 2\\^31 - 1 vertices"):
        pb3d.weld_vertices_resident(None, 2 ** 31)
    with pytest.raises(ValueError, match="faces"):
        pb3d.weld_vertices_resident(None, 4, None, 2 ** 31 // 3 + 1)


def test_empty_inputs_need_no_device():
    import pb3d
    for vdt, fdt in ((np.float32, np.int32), (np.float64, np.int64), (np.int16, np.uint8)):
        V, F, c = np.zeros((0, 3), vdt), np.zeros((0, 3), fdt), np.zeros((0, 1), np.uint8)
        out = pb3d.weld_vertices(V, F, c, return_index=True, return_inverse=True, return_counts=True)
        same_result(dict(zip(("vertices", "faces", "colors", "index", "inverse", "counts"), out)), wr.restate(V, F, c), (vdt, fdt))
        got = pb3d.weld_vertices(V)
        assert isinstance(got, np.ndarray) and got.shape == (0, 3) and got.dtype == (vdt if vdt == np.float32 else np.float64)
        assert len(pb3d.weld_vertices(V, F)) == 2 and len(pb3d.weld_vertices(V, return_counts=True)) == 2


def test_cabi_refusals_need_no_device():
    import pb3d
    lib = pb3d._lib.load()
    one, two, three, four, five = (C.c_void_p(256 * k) for k in range(1, 6))
    m = C.c_int64(7)
    weld = lib.pb3d_weld_vertices_resident

    def refused(rc, text):
        assert rc == -1 and text in lib.pb3d_last_error().decode(), (rc, lib.pb3d_last_error())

    def call(nv, nf, text, verts=one, faces=two, colors=None, channels=3, out_v=three, out_f=four, out_c=None, index=None, inverse=None, counts=None,
             classes=C.byref(m)):
        refused(weld(None, verts, 0, nv, faces, 0, nf, colors, channels, out_v, out_f, out_c, index, inverse, counts, classes), text)

    call(-1, 1, "negative count")
    call(5, -1, "negative count")
    call(2 ** 31, 1, "at most 2^31 - 1 vertices")
    call(5, (2 ** 31 - 1) // 3 + 1, "(2^31 - 1) / 3 faces")
    call(5, 2, "null argument", classes=None)
    call(5, 2, "channels must be 1 or 3", colors=five, channels=2, out_c=five)
    call(5, 2, "null buffer", verts=None)
    call(5, 2, "null buffer", out_v=None)
    call(5, 2, "null buffer", faces=None)
    call(5, 2, "null buffer", out_f=None)
    call(5, 2, "null buffer", colors=five)                                      # colours in, none out
    call(5, 2, "null buffer", out_c=five)
    call(5, 2, "may not alias", out_v=one)
    call(5, 2, "may not alias", out_f=two)
    call(5, 2, "may not alias", index=one)
    call(5, 2, "may not alias", inverse=two)
    call(5, 2, "may not alias", colors=five, out_c=C.c_void_p(2048), counts=five)
    call(5, 2, "null context")
    call(5, 0, "null context", faces=None, out_f=None)                           # a cloud needs no faces
    call(0, 0, "null context", verts=None, faces=None, out_v=None, out_f=None)  # nothing needs no buffers
    assert m.value == 7


# =====================================================================================================================
# GPU
# =====================================================================================================================

@gpu
@pytest.mark.parametrize("name", SOUPS)
def test_soups(pb3d_gpu, name):
    same_result(on_device(pb3d_gpu, name), want(name), name)


@gpu
@pytest.mark.parametrize("name", SEAMS)
def test_sort_tile_seams(pb3d_gpu, name):
    same_result(on_device(pb3d_gpu, name), want(name), name)


@gpu
@pytest.mark.parametrize("name", BITS)
def test_equality_is_ieee_equality(pb3d_gpu, name):
    same_result(on_device(pb3d_gpu, name), want(name), name)


@gpu
@pytest.mark.parametrize("name", EXTRAS)
def test_colours_unreferenced_and_index_dtypes(pb3d_gpu, name):
    same_result(on_device(pb3d_gpu, name), want(name), name)
    V, F, c = case(name)
    out = pb3d_gpu.weld_vertices(V, F, c)
    assert len(out) == (3 if c is not None else 2) and out[0].tobytes() == want(name)["vertices"].tobytes() and out[1].dtype == F.dtype


@gpu
def test_return_forms(pb3d_gpu):
    V = case("zeros")[0]
    got = pb3d_gpu.weld_vertices(V)
    assert isinstance(got, np.ndarray) and got.tobytes() == want("zeros")["vertices"].tobytes()
    verts, counts = pb3d_gpu.weld_vertices(V, return_counts=True)
    assert counts.dtype == np.int64 and counts.tolist() == [3, 1, 1]
    verts, faces, inverse = pb3d_gpu.weld_vertices(V, np.zeros((0, 3), np.int16), return_inverse=True)
    assert faces.shape == (0, 3) and faces.dtype == np.int16 and inverse.dtype == np.int32 and inverse.tolist() == [0, 1, 0, 0, 2]


@gpu
def test_bad_index_is_refused(pb3d_gpu):
    V, F, _ = case("soup/mc")
    for bad in (len(V), -len(V) - 1):
        G = F.copy()
        G[len(G) // 2, 1] = bad
        with pytest.raises(IndexError):
            pb3d_gpu.weld_vertices(V, G)
    same_result(on_device(pb3d_gpu, "soup/mc"), want("soup/mc"), "after a refusal")


@gpu
def test_soup_welds_back_and_orients(pb3d_gpu):
    """soup -> weld_vertices -> mesh_topology equals the original mesh's totals; -> orient_mesh after random pre-swaps -> closed"""
    for name, (V, F) in (("soup/mc", mc_mesh()), ("soup/fragments", mc.fragments_mesh())):
        S, SF, _ = case(name)
        same_result(on_device(pb3d_gpu, name), want(name), name)
        assert pb3d_gpu.mesh_topology(SF, len(S))["components"] == len(F)                  # the soup: one component per face
        W, WF = pb3d_gpu.weld_vertices(S, SF)
        t = pb3d_gpu.mesh_topology(WF, len(W))
        assert t == pb3d_gpu.mesh_topology(F, len(V)) and t["closed"]
        G = orr.preswapped(WF, 8)[0]
        assert not pb3d_gpu.mesh_topology(G, len(W))["closed"]
        out, stats, totals = pb3d_gpu.orient_mesh(W, G, "negative", return_stats=True)
        ref = orr.restate(G, len(W), W, "negative")
        assert np.array_equal(out, ref["faces"]) and totals == ref["totals"] and stats["volume"].tobytes() == ref["stats"]["volume"].tobytes()
        assert pb3d_gpu.mesh_topology(out, len(W))["closed"] and stats["orientable"].all()
