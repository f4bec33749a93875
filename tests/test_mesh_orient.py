"""mesh_orientation and orient_mesh (pb3d/orient.py, csrc/orient.hip on csrc/meshcomp.hip's front half) against the NumPy / SciPy
restatement of tests/orient_restate.py, and that restatement against a plain breadth-first walk.  Every comparison is np.array_equal
(floats by their bytes): include/pb3d.h states the result to the bit, so there is no tolerance anywhere."""
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
from pb3d import mesh_orientation, orient_mesh  # noqa: F401  (without the feature nothing in this file can run)

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNS = (None, "positive", "negative")
SEAM_STRIPS = (682, 683, 1366, 4097)            # 3 m = 2046, 2049, 4098 and 12291 records: the sort's tile is 2048 pairs
SUM_STRIPS = (255, 256, 257, 513, 65537)        # faces: the sums' block is 256; 65 537: a face-adjacency path that long


@functools.lru_cache(maxsize=None)
def mc_mesh():
    """the marching-cubes mesh of random_mask((12, 10, 11), 0.35, 3): 1079 vertices, 2462 faces, 16 patches"""
    mask = vr.random_mask((12, 10, 11), 0.35, 3)
    v, f, _ = me.marching_cubes_binary(mask)
    return sr._frozen(v, f) + (mask,)


def box_mesh(cavity):
    mask = np.zeros((6, 5, 5), bool)
    mask[1:5, 1:4, 1:4] = True                  # the 4 x 3 x 3 box
    if cavity:
        mask[2:4, 2, 2] = False
    v, f, _ = me.marching_cubes_binary(mask)
    return v, f


# ---- the cases: name -> (vertices, faces) ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, arg = name.partition("/")
    hand = dict(tets_vertex=mc.tets_sharing_vertex, tets_edge=mc.tets_sharing_edge, flipped=mc.tet_with_flipped_face, open=mc.open_triangle,
                loops=mc.loop_faces, book=mc.book, fragments=mc.fragments_mesh, folded=sr.folded_mesh, fan=orr.fan,
                ball=lambda: sr.ball_mesh()[:2], box=lambda: box_mesh(False), box_cavity=lambda: box_mesh(True),
                uv_sphere=lambda: vr.uv_sphere((0.3, -0.2, 0.1), 2.5), mc=lambda: mc_mesh()[:2])
    if kind == "rp2":
        return mc._irrational(6, 6.0).astype(np.float32) + np.eye(6, 3, dtype=np.float32), orr.PROJECTIVE_PLANE
    if kind in ("mobius", "band"):
        return orr.band(int(arg), kind == "mobius")
    if kind == "strip":                                                         # a seeded random half of the faces wound the other way
        V, F = mc.strip(int(arg))
        return V, orr.preswapped(F, int(arg))[0]
    if kind == "swapped":                                                       # swapped/<case>
        V, F = case(arg)
        return V, orr.preswapped(F, 11)[0]
    if kind in hand:
        V, F = hand[kind]()[:2]
        return np.asarray(V), np.asarray(F)
    V, F = mc.fragments_mesh()
    G = orr.preswapped(F, 5)[0]
    if kind == "faces_reversed":
        return V, np.ascontiguousarray(G[::-1])
    if kind == "vertices_reversed":
        return np.ascontiguousarray(V[::-1]), (len(V) - 1 - G).astype(G.dtype)
    if kind == "f64i64":
        return V.astype(np.float64) * np.pi, G.astype(np.int64)
    if kind == "uint16":
        return V.astype(np.float64), G.astype(np.uint16)
    assert kind == "negative"
    G = G.astype(np.int64)
    G[np.random.default_rng(4).random(G.shape) < 0.5] -= len(V)
    return V.astype(np.float64), G


HAND = ["rp2", "mobius/3", "mobius/5", "mobius/8", "band/5", "tets_vertex", "tets_edge", "flipped", "open", "loops", "box", "box_cavity"]
SEAMS = [f"strip/{m}" for m in SEAM_STRIPS] + ["book"]
SUMS = [f"strip/{m}" for m in SUM_STRIPS]
SOLIDS = ["fragments", "folded", "ball", "uv_sphere", "box", "swapped/fragments", "swapped/folded", "swapped/ball", "swapped/uv_sphere", "swapped/mc"]
PERMUTED = ["faces_reversed", "vertices_reversed"]
TYPED = ["f64i64", "uint16", "negative"]
CASES = HAND + SEAMS + SUMS + ["fan"] + SOLIDS + PERMUTED + TYPED


@functools.lru_cache(maxsize=None)
def want(name, sign=None, measured=True):
    """the restatement of a case, computed once and shared"""
    V, F = case(name)
    r = orr.restate(F, len(V), V if measured else None, sign)
    for a in [r["flip"], r["patch"], r["faces"], *r["stats"].values()]:
        a.setflags(write=False)
    return r


def same_result(got, ref, what):
    assert got["totals"] == ref["totals"], (what, got["totals"], ref["totals"])
    for part in ("flip", "patch", "faces"):
        g, w = got[part], ref[part]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, part, "first differing face", int(np.flatnonzero((g != w).reshape(len(g), -1).any(1))[0]))
    assert set(got["stats"]) == set(ref["stats"]), (what, list(got["stats"]))
    for part, w in ref["stats"].items():
        g = got["stats"][part]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, g.shape)
        if not np.array_equal(g.view(np.uint8), w.view(np.uint8)):
            bad = np.flatnonzero(g != w)
            raise AssertionError((what, part, "first differing patch", int(bad[0]), g[bad[0]], w[bad[0]], "differing", len(bad), "of", len(g)))


# =====================================================================================================================
# CPU: the restatement against a walk, its invariants, the pinned facts; exports; validation
# =====================================================================================================================

@pytest.mark.parametrize("name", CASES)
def test_restatement_is_the_walk(name):
    V, F = case(name)
    for sign in SIGNS:
        same_result(want(name, sign), orr.loop(F, len(V), V, sign), (name, sign))
    same_result(want(name, None, False), orr.loop(F, len(V)), (name, "no vertices"))


@pytest.mark.parametrize("name", CASES)
def test_restatement_invariants(name):
    V, F = case(name)
    for sign in SIGNS:
        r = want(name, sign)
        st, t, patch = r["stats"], r["totals"], r["patch"]
        ids, first = np.unique(patch, return_index=True)
        assert np.array_equal(ids, np.arange(t["patches"])) and (np.diff(first) > 0).all() and first[0] == 0      # numbered by smallest face
        assert st["faces"].sum() == len(F) and st["pair_edges"].sum() == t["pair_edges"] and st["boundary_edges"].sum() == t["boundary_edges"]
        assert st["disagreeing_edges"].sum() == t["disagreeing_edges"] and st["flipped_faces"].sum() == t["flipped_faces"] == r["flip"].sum()
        assert st["orientable"].sum() == t["orientable_patches"] and st["inverted"].sum() == t["inverted_patches"]
        assert not (st["inverted"] & ~st["orientable"]).any() and not (st["inverted"] & (st["boundary_edges"] > 0)).any()
        assert (st["flipped_faces"][~st["orientable"]] == 0).all() and (sign is not None or not st["inverted"].any())
        ref = mc.restate(F, len(V))["totals"]
        assert t["boundary_edges"] == ref["boundary_edges"] and t["nonmanifold_edges"] == ref["nonmanifold_edges"]
        assert (r["faces"][:, 0] == np.asarray(F)[:, 0]).all()                   # the first corner stays
        if sign is not None:
            decided = st["orientable"] & (st["boundary_edges"] == 0)
            assert ((st["volume"][decided] >= 0) if sign == "positive" else (st["volume"][decided] <= 0)).all()
        # orienting the output flips nothing, and no pair edge of an orientable patch disagrees any more
        again = orr.restate(r["faces"], len(V), V, sign)
        assert again["totals"]["flipped_faces"] == 0 and np.array_equal(again["patch"], patch)
        assert (again["stats"]["disagreeing_edges"][st["orientable"]] == 0).all()
        assert np.array_equal(again["stats"]["volume"].view(np.uint64), st["volume"].view(np.uint64))


def test_pinned_facts():
    t = want("rp2")["totals"]
    assert (t["patches"], t["orientable_patches"], t["pair_edges"], t["boundary_edges"], t["flipped_faces"]) == (1, 0, 15, 0, 0)
    for k in (3, 5, 8):
        t = want(f"mobius/{k}")["totals"]
        assert (t["patches"], t["orientable_patches"], t["boundary_edges"], t["flipped_faces"]) == (1, 0, 2 * k, 0)
    t = want("band/5")["totals"]
    assert (t["patches"], t["orientable_patches"], t["boundary_edges"]) == (1, 1, 10)
    t = want("flipped")["totals"]
    assert (t["patches"], t["disagreeing_edges"], t["flipped_faces"]) == (1, 3, 1) and want("flipped")["flip"].tolist() == [0, 0, 1, 0]
    assert want("tets_edge")["totals"]["patches"] == 2 and want("tets_vertex")["totals"]["patches"] == 2
    assert want("tets_edge")["stats"]["nonmanifold_records"].tolist() == [2, 2] and want("tets_edge")["totals"]["nonmanifold_edges"] == 1
    assert want("book")["totals"]["patches"] == 4097
    V, F = case("fragments")
    assert len(F) == 5352 and mc.restate(F, len(V))["totals"]["components"] == 43
    t = want("fragments")["totals"]
    assert (t["patches"], t["orientable_patches"]) == (59, 59)
    assert len(case("folded")[1]) == 10648 and want("folded")["totals"]["patches"] == 15
    for name in ("swapped/fragments", "swapped/folded"):
        V, F = case(name)
        assert mc.restate(F, len(V))["totals"]["unbalanced_edges"] > 0
        assert mc.restate(want(name)["faces"], len(V))["totals"]["unbalanced_edges"] == 0
    V, F, _ = mc_mesh()
    assert (len(V), len(F), want("swapped/mc")["totals"]["patches"]) == (1079, 2462, 16)


def test_our_own_shells_are_negative():
    """in their own frame marching-cubes shells have negative V and their cavities positive (pb3d/orient.py's docstring)"""
    assert want("box")["stats"]["volume"].tolist() == [-(4 * 3 * 3 - 13.0 / 3.0)] == [-31.666666666666668]
    v = want("box_cavity")["stats"]["volume"]
    assert v[0] == -31.666666666666668 and v[1] == 2.0 / 3.0 and len(v) == 2
    r = want("box_cavity", "negative")
    assert r["stats"]["inverted"].tolist() == [False, True] and (r["stats"]["volume"] < 0).all()     # per patch: the cavity ends negative too


def test_restated_sign_rule_does_not_depend_on_the_input_winding():
    for name in ("fragments", "ball", "mc"):
        V, F = case(name)
        for sign in ("positive", "negative"):
            ref = want(name, sign)
            decided = (ref["stats"]["orientable"] & (ref["stats"]["boundary_edges"] == 0) & (ref["stats"]["volume"] != 0))[ref["patch"]]     # V == 0 decides nothing
            for seed in (1, 2):
                r = orr.restate(orr.preswapped(F, seed)[0], len(V), V, sign)
                assert np.array_equal(r["faces"][decided], ref["faces"][decided]), (name, sign, seed)


def test_exports():
    import pb3d
    for n in ("mesh_orientation", "orient_mesh", "mesh_orientation_resident", "orient_mesh_resident"):
        assert callable(getattr(pb3d, n)) and n in pb3d.orient.__all__
    header = open(os.path.join(ROOT, "include", "pb3d.h")).read()
    assert "pb3d_mesh_orient_resident" in pb3d._lib.EXPORTED_SYMBOLS and re.search(r"^int\s+pb3d_mesh_orient_resident\s*\(", header, re.M)
    assert "negative" in pb3d.orient.__doc__.lower() and "-31.666" in pb3d.orient.__doc__


def test_validation_needs_no_device():
    import pb3d
    V = np.zeros((4, 3))
    F = np.array([[0, 1, 2]])
    for sign in ("outward", 1, True, "Positive"):
        for fn in (lambda: pb3d.mesh_orientation(F, vertices=V, volume_sign=sign), lambda: pb3d.orient_mesh(V, F, volume_sign=sign),
                   lambda: pb3d.mesh_orientation_resident(None, 1, 4, None, sign), lambda: pb3d.orient_mesh_resident(None, 4, None, 1, sign)):
            with pytest.raises(ValueError, match="volume_sign must be None, 'positive' or 'negative'"):
                fn()
    for fn in (lambda: pb3d.mesh_orientation(F, 4, volume_sign="positive"), lambda: pb3d.mesh_orientation_resident(None, 1, 4, None, "negative")):
        with pytest.raises(ValueError, match="volume_sign needs the vertices"):
            fn()
    for bad in (np.nan, np.inf, -np.inf):
        p = V.copy()
        p[3, 1] = bad                                                           # a vertex no face names
        for fn in (lambda: pb3d.mesh_orientation(F, vertices=p), lambda: pb3d.orient_mesh(p, F)):
            with pytest.raises(ValueError, match="NaN or infinity"):
                fn()
    with pytest.raises(ValueError, match="n_vertices"):
        pb3d.mesh_orientation(F, 5, vertices=V)
    for fn in (lambda v, f: pb3d.mesh_orientation(f, vertices=v), pb3d.orient_mesh):
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
        pb3d.mesh_orientation(F, 0)
    with pytest.raises(ValueError, match="at most 2\\^31 - 1 vertices"):
        pb3d.mesh_orientation_resident(None, 1, 2 ** 31)
    with pytest.raises(ValueError, match="faces"):
        pb3d.mesh_orientation_resident(None, 2 ** 31, 4)


def test_empty_inputs_need_no_device():
    import pb3d
    for vdt, fdt in ((np.float32, np.int32), (np.float64, np.int64), (np.int16, np.uint8)):
        V, F = np.ones((5, 3), vdt), np.zeros((0, 3), fdt)
        for sign in SIGNS:
            flip, patch, stats, totals = pb3d.mesh_orientation(F, vertices=V, volume_sign=sign)
            out, flip2, patch2, stats2, totals2 = pb3d.orient_mesh(V, F, sign, return_flips=True, return_patches=True, return_stats=True)
            ref = orr.restate(F, 5, V, sign)
            same_result(dict(flip=flip, patch=patch, faces=out, stats=stats, totals=totals), ref, (vdt, fdt, sign))
            same_result(dict(flip=flip2, patch=patch2, faces=out, stats=stats2, totals=totals2), ref, (vdt, fdt, sign))
        flip, patch, stats, totals = pb3d.mesh_orientation(F, 5)
        assert "volume" not in stats and totals == dict.fromkeys(orr.TOTALS, 0)
        assert pb3d.orient_mesh(V, F).shape == (0, 3) and pb3d.orient_mesh(V, F).dtype == fdt
    assert pb3d.mesh_orientation(np.zeros((0, 3), np.int32))[0].shape == (0,)


def test_cabi_refusals_need_no_device():
    import pb3d
    lib = pb3d._lib.load()
    one, two, three, four, five = (C.c_void_p(256 * k) for k in range(1, 6))
    totals = (C.c_int64 * 8)(*([7] * 8))
    orient = lib.pb3d_mesh_orient_resident

    def refused(rc, text):
        assert rc == -1 and text in lib.pb3d_last_error().decode(), (rc, lib.pb3d_last_error())

    refused(orient(None, None, 0, -1, one, 0, 1, 0, two, three, None, four, None, totals), "negative count")
    refused(orient(None, None, 0, 5, one, 0, -1, 0, two, three, None, four, None, totals), "negative count")
    refused(orient(None, None, 0, 2 ** 31, one, 0, 1, 0, two, three, None, four, None, totals), "at most 2^31 - 1 vertices")
    refused(orient(None, None, 0, 5, one, 0, (2 ** 31 - 1) // 6 + 1, 0, two, three, None, four, None, totals), "(2^31 - 1) / 6 faces")
    for sign in (-1, 3):
        refused(orient(None, five, 0, 5, one, 0, 2, sign, two, three, None, four, None, totals), "volume_sign must be 0 (keep), 1 (positive) or 2 (negative)")
    refused(orient(None, None, 0, 5, one, 0, 2, 0, two, three, None, four, None, None), "null argument")
    for sign in (1, 2):
        refused(orient(None, None, 0, 5, one, 0, 2, sign, two, three, None, four, None, totals), "the sign rule needs the vertices")
    refused(orient(None, None, 0, 5, one, 0, 2, 0, two, three, None, four, five, totals), "the volumes need the vertices")
    refused(orient(None, None, 0, 5, None, 0, 2, 0, two, three, None, four, None, totals), "null buffer")
    refused(orient(None, None, 0, 5, one, 0, 2, 0, None, three, None, four, None, totals), "null buffer")
    refused(orient(None, None, 0, 5, one, 0, 2, 0, two, None, None, four, None, totals), "null buffer")
    refused(orient(None, None, 0, 5, one, 0, 2, 0, two, three, None, None, None, totals), "null buffer")
    refused(orient(None, None, 0, 5, one, 0, 2, 0, one, three, None, four, None, totals), "may not alias")
    refused(orient(None, None, 0, 5, one, 0, 2, 0, two, three, one, four, None, totals), "may not alias")
    refused(orient(None, five, 0, 5, one, 0, 2, 0, two, three, None, five, None, totals), "may not alias")
    refused(orient(None, None, 0, 5, one, 0, 2, 0, two, three, None, four, None, totals), "null context")
    refused(orient(None, None, 0, 0, None, 0, 0, 0, None, None, None, None, None, totals), "null context")      # an empty mesh needs no buffers
    assert list(totals) == [7] * 8


# =====================================================================================================================
# GPU
# =====================================================================================================================

def on_device(pb3d, name, sign, measured=True):
    V, F = case(name)
    out, flip, patch, stats, totals = pb3d.orient_mesh(V, F, sign, return_flips=True, return_patches=True, return_stats=True)
    if measured:
        flip2, patch2, stats2, totals2 = pb3d.mesh_orientation(F, vertices=V, volume_sign=sign)
    else:
        flip2, patch2, stats2, totals2 = pb3d.mesh_orientation(F, len(V))
        stats = {k: v for k, v in stats.items() if k != "volume"}
    assert np.array_equal(flip, flip2) and np.array_equal(patch, patch2) and totals == totals2 and set(stats) == set(stats2)
    assert all(np.array_equal(stats[k].view(np.uint8), stats2[k].view(np.uint8)) for k in stats)
    return dict(flip=flip, patch=patch, faces=out, stats=stats, totals=totals)


def check(pb3d, names, signs=SIGNS):
    for name in names:
        for sign in signs:
            same_result(on_device(pb3d, name, sign), want(name, sign), (name, sign))
        same_result(on_device(pb3d, name, None, False), want(name, None, False), (name, "no vertices"))


@gpu
def test_hand_made_on_the_device(pb3d_gpu):
    check(pb3d_gpu, HAND)


@gpu
@pytest.mark.parametrize("name", SEAMS)
def test_sort_tile_seams(pb3d_gpu, name):
    check(pb3d_gpu, [name], (None,))


@gpu
@pytest.mark.parametrize("name", SUMS)
def test_block_seams_and_forest_depth(pb3d_gpu, name):
    check(pb3d_gpu, [name], (None,))


@gpu
def test_fan_round_one_vertex(pb3d_gpu):
    check(pb3d_gpu, ["fan"], (None, "negative"))


@gpu
@pytest.mark.parametrize("name", SOLIDS)
def test_solids_under_every_sign(pb3d_gpu, name):
    check(pb3d_gpu, [name])


@gpu
def test_numbering_follows_the_faces(pb3d_gpu):
    check(pb3d_gpu, PERMUTED, (None, "positive"))


@gpu
def test_dtypes_and_indices(pb3d_gpu):
    check(pb3d_gpu, TYPED, (None, "positive"))
    for name in TYPED:
        V, F = case(name)
        out, flip = pb3d_gpu.orient_mesh(V, F, return_flips=True)
        assert out.dtype == F.dtype and flip.any() and not flip.all()
        assert out[flip == 0].tobytes() == F[flip == 0].tobytes() and out[flip == 1].tobytes() == F[flip == 1][:, [0, 2, 1]].tobytes()


@gpu
def test_a_second_pass_flips_nothing(pb3d_gpu):
    for name in ("swapped/fragments", "swapped/mc", "mobius/5", "strip/4097"):
        V, F = case(name)
        for sign in SIGNS:
            same_result(on_device(pb3d_gpu, name, sign), want(name, sign), (name, sign))
            out, stats, _ = pb3d_gpu.orient_mesh(V, F, sign, return_stats=True)
            again, flip, stats2, totals2 = pb3d_gpu.orient_mesh(V, out, sign, return_flips=True, return_stats=True)
            assert not flip.any() and totals2["flipped_faces"] == 0 and np.array_equal(again, out), (name, sign)
            assert (stats2["disagreeing_edges"][stats["orientable"]] == 0).all(), (name, sign)


@gpu
def test_sign_rule_does_not_depend_on_the_input_winding(pb3d_gpu):
    for name in ("fragments", "ball", "mc"):
        V, F = case(name)
        for sign in ("positive", "negative"):
            same_result(on_device(pb3d_gpu, name, sign), want(name, sign), (name, sign))
            ref = want(name, sign)
            decided = (ref["stats"]["orientable"] & (ref["stats"]["boundary_edges"] == 0) & (ref["stats"]["volume"] != 0))[ref["patch"]]     # V == 0 decides nothing
            for seed in (1, 2):
                out = pb3d_gpu.orient_mesh(V, orr.preswapped(F, seed)[0], sign)
                assert out[decided].tobytes() == ref["faces"][decided].tobytes(), (name, sign, seed)


@gpu
def test_marching_cubes_mesh_closes_again(pb3d_gpu):
    V, F, mask = mc_mesh()
    G = case("swapped/mc")[1]
    assert not pb3d_gpu.mesh_topology(G, len(V))["closed"]
    for sign in SIGNS:
        same_result(on_device(pb3d_gpu, "swapped/mc", sign), want("swapped/mc", sign), sign)
        out = pb3d_gpu.orient_mesh(V, G, sign)
        assert pb3d_gpu.mesh_topology(out, len(V))["closed"]
        assert np.array_equal(pb3d_gpu.voxelize_mesh(V, out, mask.shape) != 0, mask)


@gpu
def test_volume_is_mesh_components_volume(pb3d_gpu):
    for name in ("swapped/ball", "swapped/uv_sphere"):
        V, F = case(name)
        for sign in SIGNS:
            same_result(on_device(pb3d_gpu, name, sign), want(name, sign), (name, sign))
            out, stats, totals = pb3d_gpu.orient_mesh(V, F, sign, return_stats=True)
            _, comp = pb3d_gpu.mesh_components(out, vertices=V)
            assert totals["patches"] == len(comp["volume"]) == 1 and stats["volume"].tobytes() == comp["volume"].tobytes(), (name, sign)


@gpu
def test_bad_index_is_refused(pb3d_gpu):
    V, F = case("fragments")
    for bad in (len(V), -len(V) - 1):
        G = F.copy()
        G[len(G) // 2, 1] = bad
        with pytest.raises(IndexError):
            pb3d_gpu.orient_mesh(V, G)
        with pytest.raises(IndexError):
            pb3d_gpu.mesh_orientation(G, len(V))
    same_result(on_device(pb3d_gpu, "fragments", None), want("fragments"), "after a refusal")
