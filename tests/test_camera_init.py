"""Notebook 2's bbox camera init and keypoint fit (reference utils/camera_estimation.py:56-170): pb3d_grid_bounds_resident against
np.where, the host scalar half against dicts captured from the reference (tools/gen_golden_overlays.py: values AND dtypes, they decide
the projection's promotion later), and optimize_camera_with_keypoints against the reference's recorded result.x, bit for bit."""
import ctypes as C
import io
import json
import os
import types
from contextlib import redirect_stdout

import numpy as np
import pytest

import overlay_restate as ovr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRIDS = [(1, 1, 1), (3, 2, 5), (65, 3, 9), (70, 5, 41), (13, 7, 64)]


def fixture():
    return json.load(open(os.path.join(GOLDEN, "overlay_init_fit.json")))


def unhex(rec):
    """a recorded camera value with its dtype: 'py' a Python float, else a NumPy scalar or (3,) array"""
    v = [float.fromhex(h) for h in rec["hex"]]
    if rec["dtype"] == "py":
        return v[0]
    a = np.array(v, np.float64).astype(rec["dtype"])
    return a if len(v) > 1 else a[0]


def same_value(got, rec):
    want = unhex(rec)
    if rec["dtype"] == "py":
        return type(got) is float and got == want
    return isinstance(got, (np.ndarray, np.generic)) and got.dtype == np.dtype(rec["dtype"]) and np.shape(got) == np.shape(want) \
        and np.array_equal(np.asarray(got), np.asarray(want))


def quiet(fn, *a, **k):
    so = io.StringIO()
    with redirect_stdout(so):
        r = fn(*a, **k)
    return r, so.getvalue()


def init_cases():
    return [(mon, view, parts) for mon, views in fixture().items() for view, rec in views.items() for parts in rec["inits"]]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_fixture_covers_both_monuments_views_and_an_empty_selection():
    fx = fixture()
    assert set(fx) == {"Akbar", "Bibi"} and all(set(v) == {"front", "drone"} for v in fx.values())
    recs = [r for v in fx.values() for w in v.values() for r in w["inits"].values()]
    assert any("error" in r for r in recs) and sum("params" in r for r in recs) >= 8
    assert sum(w["fit"] is not None for v in fx.values() for w in v.values()) >= 2


@pytest.mark.parametrize("mon,view,parts", init_cases())
def test_scalar_half_equals_reference(mon, view, parts):
    from pb3d.camera_estimation import bbox_init_from_bounds
    rec = fixture()[mon][view]["inits"][parts]
    if "error" in rec:                                  # no voxel of the parts: grid_bounds reports count 0 and no bounds
        with pytest.raises(ValueError) as e:
            bbox_init_from_bounds(None, None, None, None, 8, 8, 30)
        assert str(e.value) == rec["error"]
        return
    x0, y0, x1, y1 = rec["img_bbox"]
    got, out = quiet(bbox_init_from_bounds, rec["lo"], rec["hi"], np.array([x0, y0]), np.array([x1, y1]), rec["H"], rec["W"], 30)
    assert list(got) == ["cam_pos", "target", "f", "cx", "cy"]
    for k in got:
        assert same_value(got[k], rec["params"][k]), (k, got[k], rec["params"][k])
    assert got["cam_pos"].dtype == np.float64 and got["target"].dtype == np.float32
    assert out == rec["prints"]


def fit_cases():
    return [(mon, view, loss) for mon, views in fixture().items() for view, rec in views.items() if rec["fit"] for loss in ("L2", "L1")]


@pytest.mark.parametrize("mon,view,loss", fit_cases())
def test_keypoint_fit_equals_recorded_x(mon, view, loss):
    from scipy.optimize import minimize
    from pb3d.camera_estimation import optimize_camera_with_keypoints
    rec = fixture()[mon][view]
    fit = rec["fit"]
    vk = {k: np.array([float.fromhex(h) for h in fit["voxel_kps"][k]]) for k in fit["voxel_kps"]}
    ik = {k: tuple(float.fromhex(h) for h in fit["image_kps"][k]) for k in fit["keys"]}
    init = {k: unhex(v) for k, v in rec["inits"][fit["init"]]["params"].items()}
    keep_v = {k: v.copy() for k, v in vk.items()}; keep_i = dict(ik); keep_init = {k: np.array(v, copy=True) for k, v in init.items()}
    image = np.zeros((rec["inits"][fit["init"]]["H"], rec["inits"][fit["init"]]["W"], 3), np.uint8)       # only its shape is read
    got, out = quiet(optimize_camera_with_keypoints, vk, ik, image, init, loss_type=loss, minimize=minimize)
    x = np.array(list(got["cam_pos"]) + list(got["target"]) + [got["f"], got["cx"], got["cy"]], np.float64)
    want = np.array([float.fromhex(h) for h in fit["x"][loss]])
    assert np.array_equal(x.view(np.uint64), want.view(np.uint64)), (x, want)
    assert list(got) == ["cam_pos", "target", "f", "cx", "cy"] and got["cam_pos"].dtype == np.float64
    assert "Optimized Camera Parameters" in out and "Final Reprojection Loss" in out
    assert all(np.array_equal(vk[k], keep_v[k]) for k in vk) and ik == keep_i
    assert all(np.array_equal(init[k], keep_init[k]) for k in init)


def test_fit_needs_a_minimiser_and_takes_the_installed_one(monkeypatch):
    from scipy.optimize import minimize
    from pb3d import camera_estimation as ce
    monkeypatch.setattr(ce, "_REF", {})         # whatever an earlier pb3d.install() left is put back afterwards
    args = ({"a_top": np.array([1.0, 2.0, 3.0])}, {"a_top": (4.0, 5.0)}, np.zeros((8, 8, 3), np.uint8),
            {"cam_pos": np.array([4.0, 4.0, -60.0]), "target": np.array([4.0, 4.0, 4.0], np.float32), "f": 50.0, "cx": 4.0, "cy": 4.0})
    with pytest.raises(TypeError, match="minimize="):
        ce.optimize_camera_with_keypoints(*args)
    ce._REF["minimize"] = minimize              # what pb3d.install() leaves from the reference package
    a, _ = quiet(ce.optimize_camera_with_keypoints, *args)
    ce._REF.clear()
    b, _ = quiet(ce.optimize_camera_with_keypoints, *args, minimize=minimize)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_exported():
    import pb3d
    from pb3d import camera_estimation as ce
    for n in ("auto_compute_initial_params_matching_bbox", "bbox_init_from_bounds", "optimize_camera_with_keypoints",
              "projection_overlays", "visualize_voxel_projection_iou"):
        assert n in ce.__all__ and getattr(pb3d, n) is getattr(ce, n)
    for n in ("grid_bounds", "grid_hit_bits"):          # module-level building blocks, no package surface
        assert callable(getattr(ce, n)) and n not in ce.__all__ and not hasattr(pb3d, n)
    for n in ("auto_compute_initial_params_matching_bbox", "optimize_camera_with_keypoints", "visualize_voxel_projection_iou"):
        assert n in pb3d._PATCH["camera_estimation"]
    for n in ("pb3d_grid_bounds_resident", "pb3d_grid_hit_bits_resident", "pb3d_overlay_compose_resident"):
        assert n in pb3d._lib.EXPORTED_SYMBOLS


def test_bounds_entry_refuses_bad_arguments():
    from pb3d import _lib
    lib = _lib.load()
    fake, out = C.c_void_p(0x1000), C.c_void_p(0x2000)
    black = np.zeros(3, np.uint8)
    many = np.ones((32, 3), np.uint8)

    def call(grid=fake, shape=(4, 4, 4), Cc=3, cols=None, n=0, o=out):
        return lib.pb3d_grid_bounds_resident(None, grid, *shape, Cc, None if cols is None else _lib.p_u8(cols), n, o)

    for kw, msg in (({"Cc": 2}, b"C must be"), ({"shape": (-1, 4, 4)}, b"bad grid shape"), ({"grid": None}, b"null grid"),
                    ({"cols": black, "n": 1}, b"black"), ({"cols": many, "n": 32}, b"at most 31"), ({"n": 1}, b"null colour table"),
                    ({"o": None}, b"null context"), ({}, b"null context")):
        assert call(**kw) == -1, kw
        assert msg in lib.pb3d_last_error(), (kw, lib.pb3d_last_error())


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def bounds_grid(shape, Cc, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(1, 4, shape + ((3,) if Cc == 3 else ()), dtype=np.uint8) * (rng.random(shape + ((1,) if Cc == 3 else ())) < 0.3)
    return np.ascontiguousarray(g.astype(np.uint8))


def check_bounds(pb3d, grid, colours, resident=None):
    n, lo, hi = pb3d.camera_estimation.grid_bounds(grid if resident is None else resident, colours)
    wn, wlo, whi = ovr.bounds(grid, colours or [])
    assert n == wn, (grid.shape, colours)
    if wn:
        assert lo.dtype == np.int64 and np.array_equal(lo, wlo) and np.array_equal(hi, whi), (grid.shape, colours, lo, hi, wlo, whi)
    else:
        assert lo is None and hi is None


@pytest.mark.gpu
@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("shape", GRIDS)
def test_bounds_against_np_where(pb3d_gpu, shape, Cc):
    one = [7] if Cc == 1 else [(7, 8, 9)]
    two = [7, 200] if Cc == 1 else [(7, 8, 9), (0, 0, 200)]
    far = tuple(s - 1 for s in shape)
    for corner in ((0, 0, 0), far):                     # one voxel at the origin / at the far corner, among other colours
        g = bounds_grid(shape, Cc, 1)
        g[corner] = one[0]
        check_bounds(pb3d_gpu, g, one)
    g = bounds_grid(shape, Cc, 2)
    g[far] = two[1]; g[0, 0, shape[2] // 2] = two[0]
    check_bounds(pb3d_gpu, g, two)                      # two colours
    check_bounds(pb3d_gpu, g, None)                     # any non-zero voxel
    check_bounds(pb3d_gpu, bounds_grid(shape, Cc, 3), one)      # empty selection: count 0
    check_bounds(pb3d_gpu, np.zeros_like(g), None)


@pytest.mark.gpu
def test_bounds_on_an_odd_byte_offset(pb3d_gpu):
    from pb3d import device as dev
    shape = (70, 5, 64)                                 # A2 % 4 == 0: only the base address forbids the dword loads
    g = bounds_grid(shape, 3, 4)
    g[69, 4, 63] = (7, 8, 9)
    d = dev.DeviceBuffer(g.nbytes + 8)
    try:
        for off in (1, 3):
            d.upload(g, byte_offset=off)
            check_bounds(pb3d_gpu, g, [(7, 8, 9)], dev.DeviceGrid(types.SimpleNamespace(ptr=d.ptr + off), g.shape))
    finally:
        d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("mon", ["Akbar", "Bibi"])
def test_init_end_to_end(pb3d_gpu, mon):
    from pb3d import eval_helpers_intra as ev
    fx = fixture()[mon]
    from pb3d import device as dev
    grid_np = np.load(os.path.join(GOLDEN, f"stored_{mon}_voxel_grid.npz"))["voxel_grid"]
    grid = dev.DeviceGrid(dev.from_numpy(grid_np), grid_np.shape)           # uploaded once for every selection and view
    try:
        _init_cases(pb3d_gpu, mon, fx, grid, grid_np)
    finally:
        grid.free()


def _init_cases(pb3d_gpu, mon, fx, grid, grid_np):
    from pb3d import eval_helpers_intra as ev
    for view, rec in fx.items():
        image, _ = quiet(lambda: np.ascontiguousarray(ev.resize_mask_to_voxel_grid(ev.load_mask(os.path.join(GOLDEN, f"data_{mon}_{view}_mask.png")), grid_np)[:, :, :3]))
        for parts, want in rec["inits"].items():
            names = parts.split(",")
            if "error" in want:
                with pytest.raises(ValueError) as e:
                    pb3d_gpu.auto_compute_initial_params_matching_bbox(grid, image, pb3d_gpu.PART_COLORS, names)
                assert str(e.value) == want["error"]
                continue
            got, out = quiet(pb3d_gpu.auto_compute_initial_params_matching_bbox, grid, image, pb3d_gpu.PART_COLORS, names, fov_deg=30)
            for k in got:
                assert same_value(got[k], want["params"][k]), (mon, view, parts, k)
            assert out == want["prints"]
            n, lo, hi = pb3d_gpu.camera_estimation.grid_bounds(grid, [pb3d_gpu.PART_COLORS[p] for p in names])
            assert n == want["count"] and list(lo) == want["lo"] and list(hi) == want["hi"]
