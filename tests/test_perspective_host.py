"""perspective_carve without a device: the NumPy restatement against every committed fixture, the mask bit layout, the refusals of
pb3d_perspective_carve_resident (all made before the context is looked at, so a null context reaches them) and the Python layer's
ValueErrors (all raised before anything is uploaded)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import perspective_restate as pr

EINVAL = -1


def test_restatement_reproduces_synthetic_fixtures():
    cases = pr.load_synthetic()
    assert set(cases) == set(pr.synthetic_cases())
    for name, (case, want, removed) in cases.items():
        got, rem = pr.carve(case["grid"], case["views"], case["colors"], case["outside"])
        assert got.dtype == np.uint8 and np.array_equal(got, want), name
        assert rem.dtype == np.int64 and np.array_equal(rem, removed), name
        other = ~pr.subject(case["grid"], case["colors"])
        assert np.array_equal(want[other], case["grid"][other]), name


def test_fixture_inputs_are_the_generator_cases():
    """the committed inputs are what perspective_restate.synthetic_cases builds: dtypes of masks and camera values included"""
    fix = pr.load_synthetic()
    for name, case in pr.synthetic_cases().items():
        f = fix[name][0]
        assert np.array_equal(f["grid"], case["grid"]) and f["outside"] == case["outside"], name
        assert len(f["views"]) == len(case["views"])
        for (fm, fc), (m, c) in zip(f["views"], case["views"]):
            assert fm.dtype == np.asarray(m).dtype and np.array_equal(fm, m), name
            for k in c:
                assert type(fc[k]) is type(c[k]) and np.array_equal(np.asarray(fc[k]), np.asarray(c[k])), (name, k)
                assert np.asarray(fc[k]).dtype == np.asarray(c[k]).dtype, (name, k)


def test_restatement_reproduces_stored_monument_fixture():
    from pb3d.config import PART_COLORS
    meta = json.load(open(os.path.join(pr.GOLDEN, "pcarve_charminar.json")))
    grid, views = pr.stored_case(meta["monument"])
    assert list(grid.shape) == meta["shape"]
    bg = np.array(PART_COLORS["background"], np.uint8)
    views = [(np.any(m != bg, axis=-1), c) for m, c in views]
    with np.load(os.path.join(pr.GOLDEN, "pcarve_charminar.npz")) as z:
        for run, rec in meta["runs"].items():
            out, removed = pr.carve(grid, views, rec["colors"], rec["outside"])
            assert removed.tolist() == rec["removed"], run
            assert pr.sha(out) == rec["sha256"], run
            assert np.array_equal(pr.keep_bits(out), z[f"{run}/keep_bits"]), run
            # the generator's condition: every view removes, and the carve leaves, at least 1 % of the subject voxels
            assert min(rec["removed"]) >= 0.01 * rec["subject"] and rec["left"] >= 0.01 * rec["subject"], run


def test_half_even_case_has_ties():
    """the rounding case does put pixels on .5: odd x - cam_x at depth 4 with f = 2"""
    case = pr.load_synthetic()["half_even"][0]
    cam = case["views"][0][1]
    pts, _ = pr.points_of(pr.subject(case["grid"]))
    d = pts[pts[:, 2] == 0] - cam["cam_pos"]
    u = d[:, 0] / d[:, 2] * cam["f"] + cam["cx"]
    v = -(d[:, 1] / d[:, 2]) * cam["f"] + cam["cy"]
    assert (d[:, 2] == 4).all() and ((u % 1) == 0.5).sum() > 50 and ((v % 1) == 0.5).sum() > 50


def test_pack_mask_bits_layout():
    from pb3d.perspective import pack_mask_bits
    rng = np.random.default_rng(5)
    for H, W in ((1, 1), (3, 31), (2, 32), (5, 33), (4, 64), (7, 97)):
        m = rng.random((H, W)) < 0.5
        bits = pack_mask_bits(m)
        assert bits.dtype == np.uint32 and bits.shape == (H, (W + 31) // 32)
        assert np.array_equal(bits, pr.pack_bits(m))
        for v in range(H):
            for u in range(W):
                assert ((int(bits[v, u >> 5]) >> (u & 31)) & 1) == int(m[v, u])
        # any dtype, any non-zero value, and (H, W, 3) set where any channel is
        assert np.array_equal(pack_mask_bits((m * 254).astype(np.uint8)), bits)
        assert np.array_equal(pack_mask_bits(np.where(m, -0.5, 0.0)), bits)
        rgb = np.zeros((H, W, 3), np.uint8)
        rgb[m, rng.integers(0, 3, int(m.sum()))] = 3
        assert np.array_equal(pack_mask_bits(rgb), bits)
    one = np.zeros((1, 40), bool); one[0, 33] = True
    assert pack_mask_bits(one).tolist() == [[0, 2]]
    for bad in (np.zeros(5), np.zeros((2, 3, 4)), np.zeros((0, 4)), np.zeros((4, 0, 3))):
        with pytest.raises(ValueError):
            pack_mask_bits(bad)


def _view(L, **kw):
    v = L.CarveView()
    v.R[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]; v.cam[:] = [0, 0, -10]
    v.f, v.cx, v.cy = 5.0, 4.0, 4.0
    v.prec[:] = kw.get("prec", [0, 0, 0, 0])
    v.Himg, v.Wimg = kw.get("H", 8), kw.get("W", 8)
    v.d_maskbits = kw.get("mask", 0x1000)          # never dereferenced: every call below is refused first
    return v


def test_entry_refusals_need_no_context():
    import pb3d
    L = pb3d._lib
    lib = L.load()
    grid = C.c_void_p(0x2000)
    cols = np.array([[1, 2, 3], [0, 0, 0]], np.uint8)
    many = np.full((32, 3), 9, np.uint8)

    def call(d_grid=grid, shape=(4, 4, 4), Cc=3, colors=None, ncolors=0, views=(), nviews=None, null_views=False):
        arr = (L.CarveView * max(1, len(views)))(*views)
        n = len(views) if nviews is None else nviews
        rc = lib.pb3d_perspective_carve_resident(None, d_grid, shape[0], shape[1], shape[2], Cc, None if colors is None else L.p_u8(colors), ncolors,
                                                 None if null_views else C.cast(arr, C.c_void_p), n, 0, grid, None)
        return rc, lib.pb3d_last_error().decode()

    good = [_view(L)]
    for what, kw, text in (
            ("C", dict(Cc=2, views=good), "C must be 1"),
            ("negative shape", dict(shape=(4, -1, 4), views=good), "bad grid shape"),
            ("null grid", dict(d_grid=None, views=good), "null grid"),
            ("too many colours", dict(colors=many, ncolors=32, views=good), "at most 31 colours"),
            ("black colour", dict(colors=cols, ncolors=2, views=good), "colour 1 is black"),
            ("black label", dict(Cc=1, colors=np.array([3, 0], np.uint8), ncolors=2, views=good), "colour 1 is black"),
            ("negative views", dict(nviews=-1), "-1 views"),
            ("null views", dict(views=good, null_views=True), "null view table"),
            ("Himg", dict(views=[_view(L, H=0)]), "view 0 has a 0 x 8 mask"),
            ("Wimg", dict(views=[_view(L), _view(L, W=-3)]), "view 1 has a 8 x -3 mask"),
            ("null mask", dict(views=[_view(L, mask=None)]), "view 0 has a null mask"),
            ("bad prec", dict(views=[_view(L, prec=[0, 2, 0, 0])]), "prec[1] must be 0 or 1"),
            ("narrowing prec", dict(views=[_view(L, prec=[1, 0, 1, 1])]), "precision may only widen"),
            ("narrowing shift", dict(views=[_view(L, prec=[0, 1, 0, 1])]), "precision may only widen")):
        rc, err = call(**kw)
        assert rc == EINVAL and text in err, (what, rc, err)
    # nothing left to refuse: the null context is what is reported, with views and without
    for kw in (dict(views=good), dict(), dict(shape=(0, 4, 4), d_grid=None, views=good), dict(Cc=1, colors=np.array([3], np.uint8), ncolors=1, views=good * 9)):
        rc, err = call(**kw)
        assert rc == EINVAL and "pb3d_perspective_carve: null context" in err, (kw, rc, err)


def test_python_value_errors_before_any_upload():
    """no device is touched: these run on a machine without one"""
    import pb3d
    cam = {"cam_pos": np.array([0, 0, -9], np.float32), "target": np.zeros(3, np.float32), "f": 4.0, "cx": 2.0, "cy": 2.0}
    g = np.zeros((3, 4, 5, 3), np.uint8)
    ok = [(np.ones((4, 4), bool), cam)]
    for grid in (np.zeros((3, 4), np.uint8), np.zeros((3, 4, 5, 4), np.uint8), np.zeros((3, 4, 5, 3, 1), np.uint8)):
        with pytest.raises(ValueError, match="voxel_grid must be"):
            pb3d.perspective_carve(grid, ok)
    for mask in (np.ones(4), np.ones((4, 4, 2)), np.ones((2, 3, 3, 3)), np.ones((0, 4))):
        with pytest.raises(ValueError, match="mask"):
            pb3d.perspective_carve(g, [(mask, cam)])
    with pytest.raises(ValueError, match="outside"):
        pb3d.perspective_carve(g, ok, outside="drop")
    with pytest.raises(ValueError, match="black"):
        pb3d.perspective_carve(g, ok, colors=[(1, 2, 3), (0, 0, 0)])
    with pytest.raises(ValueError, match="label 0"):
        pb3d.perspective_carve(g[..., 0], ok, colors=[0])
    with pytest.raises(ValueError, match="at most 31"):
        pb3d.perspective_carve(g, ok, colors=[(k + 1, 0, 0) for k in range(32)])
    with pytest.raises(ValueError, match="empty"):
        pb3d.perspective_carve(g, ok, colors=[])
    with pytest.raises(ValueError, match="uint8 values"):
        pb3d.perspective_carve(g, ok, colors=[(256, 0, 0)])
    for kw in (dict(outside="drop"), dict(colors=[(0, 0, 0)]), dict(colors=[]), dict(colors=[(k + 1, 0, 0) for k in range(32)])):
        with pytest.raises(ValueError):
            pb3d.perspective_carve_resident(None, (3, 4, 5, 3), ok, **kw)
