"""The deformation restatement (tests/deform_restate.py) against the committed closures' results (tests/golden/deform_edges.*, written by
tools/gen_golden_deform.py), and the conditions that keep tests/test_deform_edges.py from being vacuous: the tie cases hold ties, the
sign(0) cases hold points on the centre, each plausible wrong arithmetic (deform_restate.VARIANTS) changes the result of a committed
case, and the batch lists reach nvalid = 0, 7n and values between.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import deform_restate as dr


@pytest.fixture(scope="module")
def fixtures():
    return dr.load()


def _saved(sc):
    return {p: {"deform": d} for p, d in sc["saved"].items()}


def test_committed_cases_are_the_constructed_ones(fixtures):
    """the fixtures hold the inputs deform_restate constructs (so a change of a construction needs the generator run again)"""
    clouds, scenes = fixtures
    built = dr.cloud_cases()
    assert list(clouds) == list(built)
    for name, c in built.items():
        got = clouds[name][0]
        assert np.array_equal(got["pts"], c["pts"]) and got["pts"].dtype == np.float32, name
        assert (got["image_shape"], got["voxel_shape"], got["deform"], got["kind"]) == (c["image_shape"], c["voxel_shape"], c["deform"], c["kind"]), name
    built = dr.scenes()
    assert list(scenes) == list(built)
    for name, s in built.items():
        got = scenes[name][0]
        assert np.array_equal(got["grid"], s["grid"]) and np.array_equal(got["image"], s["image"]) and got["saved"] == s["saved"], name
        assert list(got["labels"].items()) == list(s["labels"].items()), name
        for k, v in s["cam"].items():
            assert np.array_equal(got["cam"][k], v) and np.asarray(got["cam"][k]).dtype == np.asarray(v).dtype, (name, k)


def test_restatement_equals_closures(fixtures):
    clouds, scenes = fixtures
    for name, (c, rows) in clouds.items():
        got = dr.deform_coords(c["pts"], c["image_shape"], c["voxel_shape"], c["deform"])
        assert got.dtype == np.int64 and np.array_equal(got, rows), name
    for name, (sc, parts, out) in scenes.items():
        shape, ishape = sc["grid"].shape[:3], sc["image"].shape[:2]
        assert set(parts) == set(sc["saved"]) and set(parts) <= set(sc["labels"])
        for part, (rows, iou) in parts.items():
            pts, _ = dr.part_points(sc["grid"], sc["labels"], part)
            assert np.array_equal(dr.deform_coords(pts, ishape, shape, sc["saved"][part]), rows), (name, part)
            inter, uni, nv = dr.iou_counts(pts, shape, sc["saved"][part], sc["image"], sc["cam"], sc["labels"][part])
            assert dr.iou(inter, uni) == iou, (name, part)
            assert nv == dr.nvalid(pts, ishape, shape, sc["saved"][part])
            assert (nv == 0) == (len(dr.deform_part(sc["grid"], sc["labels"], part, sc["saved"][part], ishape)[0]) == 0)
        assert np.array_equal(dr.build_deformed_grid(sc["grid"], sc["labels"], _saved(sc), ishape), out), name


def test_oracle_equals_restatement(fixtures, oracle):
    """the C oracle other tests compare with is pinned on the same cases"""
    clouds, scenes = fixtures
    for name, (c, rows) in clouds.items():
        assert np.array_equal(oracle.deform_coords(c["pts"], c["image_shape"], c["voxel_shape"], c["deform"]), rows), name
    for name, (sc, parts, out) in scenes.items():
        ishape = sc["image"].shape[:2]
        for part, (rows, iou) in parts.items():
            cd, cols = oracle.deform_part(sc["grid"], sc["labels"], part, sc["saved"][part], ishape)
            want, wcols = dr.deform_part(sc["grid"], sc["labels"], part, sc["saved"][part], ishape)
            assert np.array_equal(cd, want) and np.array_equal(cols, wcols), (name, part)
            assert oracle.evaluate_part_deform(sc["grid"], sc["labels"], part, sc["saved"][part], sc["image"], sc["cam"])[1] == iou, (name, part)
        assert np.array_equal(oracle.build_deformed_grid(sc["grid"], sc["labels"], _saved(sc), ishape), out), name


def test_cases_reach_their_edges(fixtures):
    clouds, scenes = fixtures
    kinds = {}
    for name, (c, rows) in clouds.items():
        v, cen = dr.values(c["pts"], [dr.scalars(c["image_shape"], c["voxel_shape"], c["deform"])])
        kinds.setdefault(c["kind"], []).append(name)
        x0, z0 = bool((cen[..., 0] == 0).any()), bool((cen[..., 2] == 0).any())
        if c["kind"] == "tie":
            assert dr.half_count(v) > 0, name
        if c["kind"] == "sign0":
            want = {"sign0_x_n3": (True, False), "sign0_z_n3": (False, True), "sign0_none_n3": (False, False)}.get(name, (True, True))
            assert (x0, z0) == want, name
            assert c["deform"]["shift_xz"] != 0
        if c["kind"] == "mean":
            n = len(c["pts"])
            assert any(Fraction(float(s) / n) != Fraction(int(s), n) for s in c["pts"].astype(np.float64).sum(axis=0)), name       # sum / n is rounded
        if c["kind"] == "f32":
            assert np.abs(c["pts"]).max() > (1 << 21) - 64 and np.abs(c["pts"]).max() < (1 << 22)
    assert {k: len(v) for k, v in kinds.items()} == {"tie": 12, "sign0": 6, "fma": 3, "f32": 1, "mean": 2, "dup": 4, "bounds": 7}
    ties = [c for c, _ in clouds.values() if c["kind"] == "tie"]
    assert {len(c["pts"]) for c in ties} == {2, 4, 8, 64}
    assert any((c["pts"].mean(axis=0) < 0).all() for c in ties) and any((c["pts"].mean(axis=0) > 0).all() for c in ties)
    neg = even = odd = 0
    for c in ties:
        v, _ = dr.values(c["pts"], [dr.scalars(c["image_shape"], c["voxel_shape"], c["deform"])])
        t = v[np.abs(v - np.trunc(v)) == 0.5]
        neg += int((t < 0).sum()); even += int((np.floor(t) % 2 == 0).sum()); odd += int((np.floor(t) % 2 == 1).sum())
    assert neg > 0 and even > 0 and odd > 0
    assert len(clouds["sign0_n1"][0]["pts"]) == 1
    assert len(np.unique(clouds["dup_rows"][0]["pts"], axis=0)) < len(clouds["dup_rows"][0]["pts"])
    assert len(clouds["dup_half"][1]) * 3 < len(clouds["dup_half"][0]["pts"])
    assert clouds["far_shift_y"][1][:, 1].max() < -90000 and (clouds["negative"][1] < 0).any()
    # bounds: rows at -1, 0, A - 1 and A of every axis
    c, rows = clouds["bounds_identity"]
    for a, A in zip((0, 1, 2), c["voxel_shape"][::-1]):
        assert set(np.unique(rows[:, a])) == {-1, 0, A - 1, A}
    assert len(set(c["voxel_shape"])) == 3
    # scenes: overlap, a part that leaves the grid, a part that is never saved, an order that differs from the order of insertion
    sc, parts, out = scenes["order"]
    ishape = sc["image"].shape[:2]
    sets = {p: {tuple(r) for r in dr.deform_part(sc["grid"], sc["labels"], p, sc["saved"][p], ishape)[0]} for p in sc["saved"]}
    assert sets["dome"] & sets["plinth"] and sets["plinth"] & sets["windows"] and sets["dome"] & sets["windows"]
    assert not sets["chhatris"] and "main_door" in sc["labels"] and "main_door" not in sc["saved"]
    assert len(dr.part_points(sc["grid"], sc["labels"], "main_door")[0]) > 0
    rev = dr.build_deformed_grid(sc["grid"], dict(reversed(list(sc["labels"].items()))), _saved(sc), ishape)
    assert not np.array_equal(rev, out)                                     # the order of part_labels decides the overlap


def _outputs(clouds, scenes, variant):
    """everything the restatement computes on the committed cases, with one detail of the arithmetic switched"""
    res = {}
    for name, (c, _) in clouds.items():
        res[name] = dr.deform_coords(c["pts"], c["image_shape"], c["voxel_shape"], c["deform"], variant)
    for name, (sc, parts, _) in scenes.items():
        ishape = sc["image"].shape[:2]
        res[name + "/grid"] = dr.build_deformed_grid(sc["grid"], sc["labels"], _saved(sc), ishape, variant)
        for part in parts:
            pts, _ = dr.part_points(sc["grid"], sc["labels"], part)
            res[f"{name}/{part}/iou"] = np.array(dr.iou_counts(pts, sc["grid"].shape[:3], sc["saved"][part], sc["image"], sc["cam"], sc["labels"][part], variant))
    return res


def test_every_variant_changes_a_committed_case(fixtures):
    clouds, scenes = fixtures
    right = _outputs(clouds, scenes, None)
    changed = {}
    for variant in dr.VARIANTS:
        wrong = _outputs(clouds, scenes, variant)
        changed[variant] = [k for k in right if not np.array_equal(right[k], wrong[k])]
        assert changed[variant], variant
    # the cases built for one variant are caught by it
    assert {"fma_x", "fma_y", "fma_z"} <= set(changed["fma"])
    assert "f32_near_2p21" in changed["float32"]
    assert {"sign0_x_n3", "sign0_z_n3", "sign0_xz_n3", "sign0_n1", "sign0/grid"} <= set(changed["sign0_plus"])
    assert "sign0_none_n3" not in changed["sign0_plus"]
    assert sum(k.startswith("tie_") for k in changed["half_away"]) >= 6 and "ties/grid" in changed["half_away"]
    assert {"mean_n7", "ties/grid"} <= set(changed["one_centre"])
    print({v: len(c) for v, c in changed.items()})


def test_batch_lists_reach_every_nvalid(fixtures):
    """across the tuple lists the GPU test sends: nvalid 0, 7n and values strictly between; the lattice is distinct"""
    clouds, _ = fixtures
    zero = full = between = 0
    for name, (c, _) in clouds.items():
        sc = dr.mixed_batch(c)
        nv = dr.in_bounds(dr.rounded(c["pts"], sc), dr.batch_bounds(c)).sum(axis=1)
        n7 = 7 * len(c["pts"])
        zero += int((nv == 0).sum()); full += int((nv == n7).sum()); between += int(((nv > 0) & (nv < n7)).sum())
        assert nv[7] == 0, name                                              # the tuple that puts the whole part outside
    assert zero > 30 and full > 30 and between > 30, (zero, full, between)
    sc = dr.lattice(8197, {0: dr.TIE_SC[0], 8191: dr.TIE_SC[1], 8192: dr.TIE_SC[2], 8196: dr.TIE_SC[3]})
    pts = clouds["tie_n8_m0"][0]["pts"]
    v, _ = dr.values(pts, sc[[0, 8191, 8192, 8196]])
    assert all(dr.half_count(x) > 0 for x in v)
    nv = dr.in_bounds(dr.rounded(pts, sc), (16, 16, 16)).sum(axis=1)
    assert (nv == 0).any() and (nv == 56).any() and ((nv > 0) & (nv < 56)).any() and len(np.unique(nv)) > 20


def test_batched_restatement_equals_one_tuple_at_a_time(fixtures):
    """iou_counts_sc over a list, dense and sparse, is iou_counts_sc of every tuple alone"""
    clouds, _ = fixtures
    rng = np.random.default_rng(3)
    for name in ("tie_n8_m0", "sign0_xz_n5", "bounds_stretch", "fma_x"):
        c = clouds[name][0]
        A = dr.batch_bounds(c)
        H, W = c["image_shape"]
        colour = (190, 0, 255)
        image = np.where(rng.random((H, W, 1)) < 0.4, np.uint8(colour), np.uint8((1, 220, 5))).astype(np.uint8)
        sc = dr.mixed_batch(c)
        for dtype in (np.float32, np.float64):
            cam = dr.front_camera(A, H, W, dtype)
            whole = dr.iou_counts_sc(c["pts"], A, sc, image, cam, colour)
            sparse = dr.iou_counts_sc(c["pts"], A, sc, image, cam, colour, dense=False)
            for k in range(len(sc)):
                one = dr.iou_counts_sc(c["pts"], A, sc[k:k + 1], image, cam, colour)
                assert [int(w[k]) for w in whole] == [int(o[0]) for o in one] == [int(s[k]) for s in sparse], (name, k)
            assert len({tuple(int(w[k]) for w in whole) for k in range(len(sc))}) > 5, name
