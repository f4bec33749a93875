"""Notebook 2's projection-IoU overlays (reference utils/camera_estimation.py:346-477) on the device: pb3d_grid_hit_bits_resident and
pb3d_overlay_compose_resident (csrc/overlay.hip) against images captured from the reference's own function (tools/gen_golden_overlays.py),
against the NumPy restatement of tests/overlay_restate.py, and against the per-part route the sweep replaces
(get_voxel_points_by_parts + project_colored_voxels, then all(proj == colour)).  Every comparison is np.array_equal: the blend is
exact, so there is no tolerance anywhere."""
import hashlib
import io
import json
import os
import types
from contextlib import redirect_stdout

import numpy as np
import pytest

import overlay_restate as ovr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("part_on_whole", "whole_on_whole", "whole_on_whole_color")
GRIDS = [(1, 1, 1), (3, 2, 5), (65, 3, 9), (70, 5, 41), (13, 7, 64)]
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def synth_meta():
    return json.load(open(os.path.join(GOLDEN, "overlay_synth.json")))


def load_case(name):
    meta = synth_meta()[name]
    with np.load(os.path.join(GOLDEN, "overlay_synth.npz"), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files if k.startswith(name + "/")}
    cam = {}
    for k, rec in meta["cam"].items():
        v = [float.fromhex(h) for h in rec["hex"]]
        cam[k] = v[0] if rec["dtype"] == "py" else np.array(v).astype(rec["dtype"])
    pc = {k: tuple(v) for k, v in meta["part_colors"].items()}
    return meta, arrays, pc, cam


def expected(meta, arrays, name, mode):
    m = meta["modes"][mode]
    return [(t, arrays[f"{name}/{mode}/{i}"], None if h is None else float.fromhex(h)) for i, (t, h) in enumerate(zip(m["titles"], m["iou"]))]


def same_overlays(got, want):
    assert [t for t, _, _ in got] == [t for t, _, _ in want]
    for (t, v, i), (_, wv, wi) in zip(got, want):
        assert v.dtype == np.uint8 and v.shape == wv.shape and np.array_equal(v, wv), t
        assert (i is None and wi is None) or float(i) == wi, (t, i, wi)


def stored_mask(mon, view, grid):
    from pb3d import eval_helpers_intra as ev
    with redirect_stdout(io.StringIO()):
        return np.ascontiguousarray(ev.resize_mask_to_voxel_grid(ev.load_mask(os.path.join(GOLDEN, f"data_{mon}_{view}_mask.png")), grid)[:, :, :3])


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_fixtures_exist():
    meta = synth_meta()
    assert set(meta) == {"borders", "pal33", "black", "twins"}
    for f in ("overlay_synth.npz", "overlay_synth.json", "overlay_akbar.json", "overlay_init_fit.json"):
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 256 * 1024
    assert len(meta["pal33"]["modes"]["part_on_whole"]["titles"]) == 33             # the absent and the out-of-range part are skipped
    assert "void | IoU" in meta["black"]["modes"]["part_on_whole"]["titles"][1]
    ak = json.load(open(os.path.join(GOLDEN, "overlay_akbar.json")))
    assert len(ak["cameras"]) == 5 and all(set(c) == set(MODES) for c in ak["cameras"].values())


@pytest.mark.parametrize("name", ["borders", "pal33", "black", "twins"])
def test_fixture_equals_restatement(name):
    meta, arrays, pc, cam = load_case(name)
    cases = ovr.synthetic_cases()[name]
    assert np.array_equal(cases[0], arrays[f"{name}/grid"]) and np.array_equal(cases[2], arrays[f"{name}/image"]) and cases[1] == pc
    for mode in MODES:
        got, outlines = ovr.overlays(arrays[f"{name}/grid"], pc, arrays[f"{name}/image"], cam, mode)
        same_overlays(got, expected(meta, arrays, name, mode))
        assert outlines == meta["modes"][mode]["outline_pixels"]
    assert meta["part_on_part"] == "name 'proj_f' is not defined"
    with pytest.raises(NameError, match="name 'proj_f' is not defined"):
        ovr.overlays(arrays[f"{name}/grid"], pc, arrays[f"{name}/image"], cam, "part_on_part")


def test_borders_case_reaches_all_four_borders():
    meta, arrays, pc, cam = load_case("borders")
    img = arrays["borders/image"]
    H, W = img.shape[:2]
    both = np.all(img == pc["slab"], -1) & ovr.hit_mask(ovr.points_of(ovr.part_mask(arrays["borders/grid"], pc["slab"])), cam, H, W)
    assert both[0].any() and both[-1].any() and both[:, 0].any() and both[:, -1].any() and not both.all()
    assert meta["modes"]["part_on_whole"]["outline_pixels"][0] > 0


def test_blend_and_dilation_are_the_library_expressions():
    from scipy.ndimage import binary_dilation
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    assert np.array_equal(ovr.blend(a, b), (0.7 * a.astype(np.float64) + 0.3 * b.astype(np.float64)).astype(np.uint8))
    rng = np.random.default_rng(0)
    for shape in ((1, 1), (1, 9), (7, 1), (13, 17)):
        m = rng.random(shape) < 0.3
        assert np.array_equal(ovr.dilate4(m), binary_dilation(m))
    assert np.array_equal(ovr.dilate4(np.ones((3, 4), bool)), np.ones((3, 4), bool))


def test_compose_entry_refuses_bad_arguments():
    import ctypes as C
    from pb3d import _lib
    lib = _lib.load()
    p = C.c_void_p(0x1000)
    cols = np.ones((40, 3), np.uint8)
    bg = np.zeros(3, np.uint8)

    def call(nplanes=1, nparts=2, mode=0, H=4, W=4, colors=cols):
        return lib.pb3d_overlay_compose_resident(None, p, nplanes, p, H, W, None if colors is None else _lib.p_u8(colors), nparts, _lib.p_u8(bg), None,
                                            mode, p, p)

    for kw, msg in (({"mode": 3}, b"mode is 0, 1 or 2"), ({"mode": -1}, b"mode is 0, 1 or 2"), ({"nparts": 249, "nplanes": 9}, b"at most 248"),
                    ({"nparts": 32}, b"take 2 bit planes"), ({"nplanes": 2}, b"take 1 bit planes"), ({"colors": None}, b"null colour table"),
                    ({"H": -1}, b"bad argument"), ({}, b"null context")):
        assert call(**kw) == -1, kw
        assert msg in lib.pb3d_last_error(), (kw, lib.pb3d_last_error())
    assert lib.pb3d_grid_hit_bits_resident(None, p, 1 << 25, 1, 1, 1, _lib.p_u8(cols), 1, None, None, 1.0, 0.0, 0.0, None, 4, 4, p) == -1
    assert b"2^24" in lib.pb3d_last_error()


# ---- GPU: hit bits -----------------------------------------------------------------------------------------------------------------
def cameras(shape, H, W):
    A0, A1, A2 = shape
    c = np.array([(A2 - 1) / 2, (A1 - 1) / 2, (A0 - 1) / 2])
    d = 3.0 * max(shape)
    f32 = ovr.front_camera(shape, H, W, 0.7)
    slider = {"cam_pos": c + [4.0, -3.0, -d], "target": c + [0.5, 0.25, 0.0], "f": 0.9 * d, "cx": W / 2 + 0.25, "cy": H / 2 - 0.75}
    promoted = dict(f32, f=np.float64(f32["f"]))                    # float32 camera, float64 focal length: the later stages widen
    inside = {"cam_pos": c.astype(np.float32), "target": (c + [0.1, 0.2, 5.0]).astype(np.float32), "f": 0.5 * max(H, W), "cx": W / 2,
              "cy": H / 2}                                          # voxels behind the camera: Z is clamped to 1e-8
    # looking away: every Z is clamped to 1e-8, and off the optical axis (no voxel has X = Y = 0) X / Z leaves any image
    away = {"cam_pos": (c + [0.37, 0.41, -d]).astype(np.float32), "target": (c + [0.37, 0.41, -2 * d]).astype(np.float32), "f": 0.7 * d,
            "cx": W / 2, "cy": H / 2}
    return {"f32": f32, "slider": slider, "promoted": promoted, "inside": inside, "away": away}


def per_part_route(pb3d, grid, colours, cam, H, W):
    bits = np.zeros((H, W), np.uint32)
    for k, c in enumerate(colours):
        pts, col = pb3d.get_voxel_points_by_parts(grid, {"p": tuple(int(v) for v in c)}, ["p"])
        if len(pts):
            proj = pb3d.project_colored_voxels(pts, col, cam["cam_pos"], cam["target"], cam["f"], cam["cx"], cam["cy"], H, W)
            bits |= np.all(proj == np.asarray(c, np.uint8), axis=-1).astype(np.uint32) << np.uint32(k)
    return bits


@pytest.mark.gpu
@pytest.mark.parametrize("shape", GRIDS)
def test_hit_bits_grids_colour_counts_images_cameras(pb3d_gpu, shape):
    case = 0
    for ncol in (1, 10, 31):
        cols = ovr.palette(ncol, 20 + ncol)
        grid = ovr.random_grid(shape, cols + ovr.palette(2, 99), 0.6, sum(shape) + ncol)        # two more colours that are no bit
        for (H, W) in ((1, 1), (5, 7), (33, 29)):
            for cname, cam in cameras(shape, H, W).items():
                got = pb3d_gpu.camera_estimation.grid_hit_bits(grid, cols, cam, H, W)
                want = ovr.hit_bits(grid, cols, cam, H, W)
                assert got.dtype == np.uint32 and np.array_equal(got, want), (shape, ncol, H, W, cname)
                if cname == "away":
                    assert not got.any()
                if case % 5 == 0:                                   # the route the sweep replaces, on a fifth of the cases
                    assert np.array_equal(got, per_part_route(pb3d_gpu, grid, cols, cam, H, W)), (shape, ncol, H, W, cname)
                case += 1
    labels = np.ascontiguousarray(ovr.random_grid(shape, [(k, 0, 0) for k in range(1, 9)], 0.6, 5)[..., 0])     # C = 1
    cam = cameras(shape, 33, 29)["slider"]
    assert np.array_equal(pb3d_gpu.camera_estimation.grid_hit_bits(labels, [3, 8, 1], cam, 33, 29), ovr.hit_bits(labels, [3, 8, 1], cam, 33, 29))


@pytest.mark.gpu
def test_hit_bits_akbar_cameras_and_odd_offset(pb3d_gpu):
    from pb3d import device as dev
    from pb3d import eval_helpers_intra as ev
    PC = pb3d_gpu.PART_COLORS
    grid = np.load(os.path.join(GOLDEN, "stored_Akbar_voxel_grid.npz"))["voxel_grid"]
    cols = list(PC.values())
    d = dev.DeviceBuffer(grid.nbytes + 4)
    d.upload(grid, byte_offset=1)
    odd = dev.DeviceGrid(types.SimpleNamespace(ptr=d.ptr + 1), grid.shape)
    try:
        for stage, view in (("init", "front"), ("init", "drone"), ("kp", "front"), ("final", "front"), ("final", "drone")):
            cam = ev.load_camera_json(os.path.join(GOLDEN, f"stored_Akbar_camera_params_{stage}.json"), view)
            H, W = stored_mask("Akbar", view, grid).shape[:2]
            got = pb3d_gpu.camera_estimation.grid_hit_bits(grid, cols, cam, H, W)
            assert np.array_equal(got, ovr.hit_bits(grid, cols, cam, H, W)), (stage, view)
            assert np.array_equal(got, pb3d_gpu.camera_estimation.grid_hit_bits(odd, cols, cam, H, W)), (stage, view)
            if stage == "final":
                assert np.array_equal(got, per_part_route(pb3d_gpu, grid, cols, cam, H, W)), (stage, view)
    finally:
        d.free()


# ---- GPU: composition --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["borders", "pal33", "black", "twins"])
def test_composition_equals_fixtures(pb3d_gpu, name):
    from pb3d import device as dev
    meta, arrays, pc, cam = load_case(name)
    grid, image = arrays[f"{name}/grid"], arrays[f"{name}/image"]
    keep_g, keep_i = grid.copy(), image.copy()
    for mode in MODES:
        same_overlays(pb3d_gpu.projection_overlays(grid, pc, image, cam, mode), expected(meta, arrays, name, mode))
    assert np.array_equal(grid, keep_g) and np.array_equal(image, keep_i)
    resident = dev.DeviceGrid(dev.from_numpy(grid), grid.shape)
    try:
        same_overlays(pb3d_gpu.projection_overlays(resident, pc, image, cam, "part_on_whole"), expected(meta, arrays, name, "part_on_whole"))
    finally:
        resident.free()
    with pytest.raises(NameError, match="name 'proj_f' is not defined"):
        pb3d_gpu.projection_overlays(grid, pc, image, cam, "part_on_part")
    assert pb3d_gpu.projection_overlays(np.zeros_like(grid), pc if name != "black" else {"a": pc["a"]}, image, cam, "part_on_part") == []
    assert pb3d_gpu.projection_overlays(grid, pc, image, cam, "no_such_mode") == []


# ---- GPU: end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_akbar_digests_and_ious(pb3d_gpu):
    from pb3d import eval_helpers_intra as ev
    PC = pb3d_gpu.PART_COLORS
    grid = np.load(os.path.join(GOLDEN, "stored_Akbar_voxel_grid.npz"))["voxel_grid"]
    dig = json.load(open(os.path.join(GOLDEN, "overlay_akbar.json")))
    assert dig["shape"] == list(grid.shape)
    for key, rec in dig["cameras"].items():
        stage, view = key.split("_")
        cam = ev.load_camera_json(os.path.join(GOLDEN, f"stored_Akbar_camera_params_{stage}.json"), view)
        image = stored_mask("Akbar", view, grid)
        per, combined = pb3d_gpu.projection_iou_by_part(grid, PC, image, cam)
        for mode in MODES:
            got = pb3d_gpu.projection_overlays(grid, PC, image, cam, mode)
            assert [t for t, _, _ in got] == rec[mode]["titles"], (key, mode)
            assert [sha(v) for _, v, _ in got] == rec[mode]["sha256"], (key, mode)
            assert [None if i is None else float(i).hex() for _, _, i in got] == rec[mode]["iou"], (key, mode)
            if mode == "part_on_whole":
                assert {t.split(" | ")[0]: i for t, _, i in got} == per, key
            if mode == "whole_on_whole":
                assert got[0][2] == combined, key
