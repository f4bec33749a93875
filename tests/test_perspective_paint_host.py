"""perspective_paint without a device: the NumPy restatement against every committed fixture, the refusals of
pb3d_perspective_paint_resident (all made before the context is looked at, so a null context reaches them) and the Python layer's
ValueErrors (all raised before anything is uploaded)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import paint_restate as pt
import perspective_restate as pr

EINVAL = -1


def test_restatement_reproduces_synthetic_fixtures():
    cases = pt.load_synthetic()
    assert set(cases) == set(pt.synthetic_cases())
    later_skipped = later_fresh = 0
    for name, (case, want, decided) in cases.items():
        trace = []
        got, dec = pt.paint(case["grid"], case["views"], case["colors"], case["skip"], case["eps"], case["zbufs"], trace)
        assert got.dtype == np.uint8 and np.array_equal(got, want), name
        assert dec.dtype == np.int64 and np.array_equal(dec, decided), name
        sel = pr.subject(case["grid"], case["colors"])
        assert np.array_equal(want[~sel], case["grid"][~sel]) and np.array_equal(pr.subject(want), pr.subject(case["grid"])), name
        # the generator's conditions: every view decides, and the call leaves undecided, at least 5 % of the subject voxels
        n = int(sel.sum())
        assert decided.min() >= 0.05 * n and n - decided.sum() >= 0.05 * n, (name, n, decided)
        before = np.zeros(n, bool)
        for k, (seen, paints, _, _) in enumerate(trace):
            if k:
                later_skipped += int((paints & before).sum()); later_fresh += int((paints & ~before).sum())
            before |= seen
    assert later_skipped > 0 and later_fresh > 0


def test_fixture_inputs_are_the_generator_cases():
    """the committed inputs are what paint_restate.synthetic_cases builds: the dtypes of camera values and eps included"""
    fix = pt.load_synthetic()
    for name, case in pt.synthetic_cases().items():
        f = fix[name][0]
        assert np.array_equal(f["grid"], case["grid"]) and f["colors"] == case["colors"] and f["skip"] == case["skip"], name
        assert type(f["eps"]) is type(case["eps"]) and f["eps"] == case["eps"], name
        assert (f["zbufs"] is None) == (case["zbufs"] is None) and len(f["views"]) == len(case["views"]), name
        if case["zbufs"] is not None:
            assert all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(f["zbufs"], case["zbufs"])), name
        for (fm, fc), (m, c) in zip(f["views"], case["views"]):
            assert fm.dtype == np.uint8 and np.array_equal(fm, m), name
            for k in c:
                assert type(fc[k]) is type(c[k]) and np.array_equal(np.asarray(fc[k]), np.asarray(c[k])), (name, k)
                assert np.asarray(fc[k]).dtype == np.asarray(c[k]).dtype, (name, k)


def test_cases_reach_what_they_are_named_for():
    from pb3d.projection_utils import camera_args
    cases = pt.load_synthetic()
    prec = lambda cam: list(camera_args(np.zeros((1, 3), np.float32), cam["cam_pos"], cam["target"], cam["f"], cam["cx"], cam["cy"])[4])  # noqa: E731
    flags = {name: [prec(cam)[0] for _, cam in case["views"]] for name, (case, _, _) in cases.items()}
    assert flags["walk_rgb_70x9x13"] == [0, 0] and flags["walk_lab_12x10x16"] == [1, 0] and flags["walk_rgb_5x7x16"] == [0, 1]
    assert len(flags["views8"]) == 8 and 0 < sum(flags["views8"]) < 8
    assert len({im.shape[:2] for im, _ in cases["views8"][0]["views"]}) == 8
    assert {type(c["eps"]) for c, _, _ in cases.values()} == {float, np.float64}
    assert cases["walk_rgb_70x9x13"][0]["grid"].shape == (70, 9, 13, 3) and cases["walk_lab_12x10x16"][0]["grid"].shape == (12, 10, 16)
    # the skip list and the supplied z-buffers decide the result
    on, off, other = cases["skip_on"], cases["skip_off"], cases["zbuf_other"]
    assert np.array_equal(on[0]["grid"], off[0]["grid"]) and not np.array_equal(on[1], off[1])
    bg = np.asarray(pt.BACKGROUND, np.uint8)
    assert (off[1] == bg).all(axis=-1).any() and not (on[1] == bg).all(axis=-1).any()
    own, _ = pt.paint(other[0]["grid"], other[0]["views"], None, other[0]["skip"])
    assert not np.array_equal(own, other[1])


def test_restatement_reproduces_stored_monument_fixture():
    meta = json.load(open(os.path.join(pt.GOLDEN, "ppaint_charminar.json")))
    grid, views = pt.stored_case(meta["monument"])
    assert list(grid.shape) == meta["shape"]
    out, decided = pt.paint(grid, views, None, [tuple(c) for c in meta["skip"]], pt.eps_from_record(meta["eps"]))
    assert decided.tolist() == meta["decided"] and min(meta["decided"]) >= 1000
    assert pt.sha(out) == meta["sha256"]
    at, vals = pt.changed_sample(grid, out)
    with np.load(os.path.join(pt.GOLDEN, "ppaint_charminar.npz")) as z:
        assert np.array_equal(at, z["sample/index"]) and np.array_equal(vals, z["sample/value"])


def _view(L, **kw):
    v = L.PaintView()
    v.R[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]; v.cam[:] = [0, 0, -10]
    v.f, v.cx, v.cy = 5.0, 4.0, 4.0
    v.prec[:] = kw.get("prec", [0, 0, 0, 0])
    v.Himg, v.Wimg = kw.get("H", 8), kw.get("W", 8)
    v.d_image = kw.get("image", 0x1000)             # never dereferenced: every call below is refused first
    v.d_zbuf = kw.get("zbuf", 0x3000)
    return v


def test_entry_refusals_need_no_context():
    import pb3d
    L = pb3d._lib
    lib = L.load()
    grid = C.c_void_p(0x200000)
    cols = np.array([[1, 2, 3], [0, 0, 0]], np.uint8)
    many = np.full((32, 3), 9, np.uint8)
    nine = np.full((9, 3), 9, np.uint8)

    def call(d_grid=grid, shape=(4, 4, 4), Cc=3, colors=None, ncolors=0, views=(), nviews=None, null_views=False, skip=None, nskip=0,
             eps_f32=0, out=grid):
        arr = (L.PaintView * max(1, len(views)))(*views)
        n = len(views) if nviews is None else nviews
        rc = lib.pb3d_perspective_paint_resident(None, d_grid, shape[0], shape[1], shape[2], Cc, None if colors is None else L.p_u8(colors), ncolors,
                                                 None if null_views else C.cast(arr, C.c_void_p), n, None if skip is None else L.p_u8(skip), nskip,
                                                 1e-3, eps_f32, out, None)
        return rc, lib.pb3d_last_error().decode()

    good = [_view(L)]
    for what, kw, text in (
            ("C", dict(Cc=2, views=good), "C must be 1"),
            ("negative shape", dict(shape=(4, -1, 4), views=good), "bad grid shape"),
            ("null grid", dict(d_grid=None, views=good), "null grid"),
            ("too many colours", dict(colors=many, ncolors=32, views=good), "at most 31 colours"),
            ("black colour", dict(colors=cols, ncolors=2, views=good), "colour 1 is black"),
            ("black label", dict(Cc=1, colors=np.array([3, 0], np.uint8), ncolors=2, views=good), "colour 1 is black"),
            ("long axis", dict(shape=((1 << 24) + 1, 1, 1), views=good), "longer than 2^24"),
            ("negative views", dict(nviews=-1), "0 to 8 views, got -1"),
            ("nine views", dict(views=good * 9), "0 to 8 views, got 9"),
            ("null views", dict(views=good, null_views=True), "null view table"),
            ("nine skip colours", dict(views=good, skip=nine, nskip=9), "at most 8 skip colours, got 9"),
            ("negative skip", dict(views=good, nskip=-1), "at most 8 skip colours, got -1"),
            ("null skip", dict(views=good, nskip=2), "null skip table"),
            ("eps_f32", dict(views=good, eps_f32=2), "eps_f32 must be 0 or 1"),
            ("Himg", dict(views=[_view(L, H=0)]), "view 0 has a 0 x 8 image"),
            ("Wimg", dict(views=[_view(L), _view(L, W=-3)]), "view 1 has a 8 x -3 image"),
            ("null image", dict(views=[_view(L, image=None)]), "view 0 has a null image"),
            ("null z-buffer", dict(views=[_view(L), _view(L, zbuf=None)]), "view 1 has a null z-buffer"),
            ("bad prec", dict(views=[_view(L, prec=[0, 2, 0, 0])]), "prec[1] must be 0 or 1"),
            ("narrowing prec", dict(views=[_view(L, prec=[1, 0, 1, 1])]), "precision may only widen"),
            ("null output", dict(views=good, out=None), "null output"),
            ("partial overlap", dict(views=good, out=C.c_void_p(0x200000 + 7)), "overlaps the grid in part"),
            ("partial overlap below", dict(views=good, out=C.c_void_p(0x200000 - 4 * 4 * 4 * 3 + 1)), "overlaps the grid in part")):
        rc, err = call(**kw)
        assert rc == EINVAL and text in err, (what, rc, err)
    # nothing left to refuse: the null context is what is reported, with views and without, in place and beside the grid
    for kw in (dict(views=good), dict(), dict(shape=(0, 4, 4), d_grid=None, views=good), dict(views=good * 8, skip=nine, nskip=8),
               dict(views=good, out=C.c_void_p(0x200000 + 4 * 4 * 4 * 3)), dict(views=good, out=C.c_void_p(0x200000 - 4 * 4 * 4 * 3)),
               dict(Cc=1, colors=np.array([3], np.uint8), ncolors=1, views=good, eps_f32=1)):
        rc, err = call(**kw)
        assert rc == EINVAL and "pb3d_perspective_paint: null context" in err, (kw, rc, err)


def test_python_value_errors_before_any_upload():
    """no device is touched: these run on a machine without one"""
    import pb3d
    cam = {"cam_pos": np.array([0, 0, -9], np.float32), "target": np.zeros(3, np.float32), "f": 4.0, "cx": 2.0, "cy": 2.0}
    g = np.zeros((3, 4, 5, 3), np.uint8)
    rgb, lab = np.ones((4, 6, 3), np.uint8), np.ones((4, 6), np.uint8)
    ok = [(rgb, cam)]
    for grid in (np.zeros((3, 4), np.uint8), np.zeros((3, 4, 5, 4), np.uint8), np.zeros((3, 4, 5, 3, 1), np.uint8)):
        with pytest.raises(ValueError, match="voxel_grid must be"):
            pb3d.perspective_paint(grid, ok)
    with pytest.raises(ValueError, match="at most 8 views, got 9"):
        pb3d.perspective_paint(g, ok * 9)
    for image in (lab, np.ones(4, np.uint8), np.ones((4, 6, 2), np.uint8), np.ones((2, 3, 3, 3), np.uint8)):       # rank / channels
        with pytest.raises(ValueError, match="image of a view is"):
            pb3d.perspective_paint(g, [(image, cam)])
    for image in (rgb, np.ones((4, 6, 1), np.uint8)):
        with pytest.raises(ValueError, match="image of a view is"):
            pb3d.perspective_paint(g[..., 0], [(image, cam)])
    for image in (np.ones((0, 6, 3), np.uint8), np.ones((4, 0, 3), np.uint8)):                                      # empty
        with pytest.raises(ValueError, match="at least one pixel"):
            pb3d.perspective_paint(g, [(image, cam)])
    with pytest.raises(ValueError, match="at least one pixel"):
        pb3d.perspective_paint(g[..., 0], [(np.ones((0, 6), np.uint8), cam)])
    with pytest.raises(ValueError, match="black"):
        pb3d.perspective_paint(g, ok, colors=[(1, 2, 3), (0, 0, 0)])
    with pytest.raises(ValueError, match="label 0"):
        pb3d.perspective_paint(g[..., 0], [(lab, cam)], colors=[0])
    with pytest.raises(ValueError, match="at most 31"):
        pb3d.perspective_paint(g, ok, colors=[(k + 1, 0, 0) for k in range(32)])
    with pytest.raises(ValueError, match="empty"):
        pb3d.perspective_paint(g, ok, colors=[])
    with pytest.raises(ValueError, match="at most 8 skip colours, got 9"):
        pb3d.perspective_paint(g, ok, skip=[(k + 1, 0, 0) for k in range(9)])
    with pytest.raises(ValueError, match="uint8 values"):
        pb3d.perspective_paint(g, ok, skip=[(256, 0, 0)])
    for zb in (np.zeros((6, 4), np.float32), np.zeros((4, 5), np.float32), np.zeros(24, np.float32), np.zeros((4, 6, 1), np.float32)):
        with pytest.raises(ValueError, match="z-buffer of view 0"):
            pb3d.perspective_paint(g, ok, zbufs=[zb])
    with pytest.raises(ValueError, match="1 views but 2 z-buffers"):
        pb3d.perspective_paint(g, ok, zbufs=[np.zeros((4, 6), np.float32)] * 2)
    for kw in (dict(colors=[(0, 0, 0)]), dict(colors=[]), dict(colors=[(k + 1, 0, 0) for k in range(32)]), dict(skip=[(9, 9, 9)] * 9)):
        with pytest.raises(ValueError):
            pb3d.perspective_paint_resident(None, (3, 4, 5, 3), ok, [None], **kw)
    with pytest.raises(ValueError, match="at most 8 views"):
        pb3d.perspective_paint_resident(None, (3, 4, 5, 3), ok * 9, [None] * 9)
    with pytest.raises(ValueError, match="image of a view is"):
        pb3d.perspective_paint_resident(None, (3, 4, 5, 1), ok, [None])
    with pytest.raises(ValueError, match="1 views but 0 z-buffers"):
        pb3d.perspective_paint_resident(None, (3, 4, 5, 3), ok, [])
