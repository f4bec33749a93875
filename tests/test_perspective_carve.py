"""perspective_carve on the device (csrc/pcarve.hip) against the committed fixtures of tests/golden/pcarve_*: every comparison is exact
equality of grids, counts, digests and keep bits.  The fixtures come from tests/perspective_restate.py, which the generator ties to
the reference's project_colored_voxels and tests/test_perspective_host.py re-runs on the CPU.

Shapes are the smallest that reach each path of the kernel: A0 = 70 crosses the 64-step chunk of the walk, A2 = 13 is ragged (byte
loads and stores), A2 = 16 on an aligned buffer moves whole dwords (C = 1: one, C = 3: three per lane), the same rows at an odd base
fall back to bytes; nine views need a second, in-place launch behind the first eight."""
import json
import os

import numpy as np
import pytest

import perspective_restate as pr

gpu = pytest.mark.gpu
GUARD = 256


@pytest.fixture(scope="module")
def cases():
    return pr.load_synthetic()


def run(pb3d, case, views=None, **kw):
    return pb3d.perspective_carve(case["grid"], case["views"] if views is None else views, colors=case["colors"], outside=case["outside"],
                                  return_counts=True, **kw)


def check(pb3d, cases, name):
    case, want, removed = cases[name]
    got, rem = run(pb3d, case)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), name
    assert rem.dtype == np.int64 and np.array_equal(rem, removed), (name, rem, removed)
    assert np.array_equal(pb3d.perspective_carve(case["grid"], case["views"], colors=case["colors"], outside=case["outside"]), want), name
    return case, want, removed


def resident(pb3d, case, want, removed, off_in, off_out):
    """the resident entry on windows into guarded arenas (tests/test_pointer_offsets.py): off_out None = in place"""
    dev = pb3d.device
    grid = case["grid"]
    shape = grid.shape if grid.ndim == 4 else grid.shape + (1,)
    n = grid.nbytes

    def arena(off, fill, payload=None):
        host = np.full(GUARD + off + n + GUARD, fill, np.uint8)
        if payload is not None:
            host[GUARD + off:GUARD + off + n] = payload.reshape(-1)
        return dev.from_numpy(host), host

    a_in, h_in = arena(off_in, 0xFF, grid)
    a_out, h_out = (a_in, h_in) if off_out is None else arena(off_out, 0xA5)
    off_o = off_in if off_out is None else off_out
    d_rem = dev.DeviceBuffer(8 * len(case["views"]) + 16)
    try:
        d_rem.upload(np.full(len(case["views"]) + 2, -7, np.int64))
        pb3d.perspective_carve_resident(a_in.at(GUARD + off_in), shape, case["views"], colors=case["colors"], outside=case["outside"],
                                        out=None if off_out is None else a_out.at(GUARD + off_out), d_removed=d_rem.at(8))
        got = a_out.download((h_out.size,))
        rem = d_rem.download((len(case["views"]) + 2,), np.int64)
        what = (grid.shape, off_in, off_out)
        assert np.array_equal(got[:GUARD + off_o], h_out[:GUARD + off_o]) and np.array_equal(got[GUARD + off_o + n:], h_out[GUARD + off_o + n:]), (what, "guard")
        assert np.array_equal(got[GUARD + off_o:GUARD + off_o + n].reshape(want.shape), want), what
        assert rem[0] == -7 and rem[-1] == -7 and np.array_equal(rem[1:-1], removed), (what, rem)
        if off_out is not None:
            assert np.array_equal(a_in.download((h_in.size,)), h_in), (what, "the input changed")
    finally:
        for b in {id(a_in): a_in, id(a_out): a_out, id(d_rem): d_rem}.values():
            b.free()


@gpu
def test_walk_edges(pb3d_gpu, cases):
    for name in ("walk_rgb_70x9x13", "walk_lab_12x10x16", "walk_rgb_5x7x16"):
        case, want, removed = check(pb3d_gpu, cases, name)
        assert removed.min() > 0
        resident(pb3d_gpu, case, want, removed, 0, None)
        resident(pb3d_gpu, case, want, removed, 0, 0)


@gpu
def test_odd_byte_offsets(pb3d_gpu, cases):
    """rows of whole dwords (A2 = 16) whose base is not 4-byte aligned, in either buffer or both"""
    for name in ("walk_rgb_5x7x16", "walk_lab_12x10x16"):
        case, want, removed = cases[name]
        for off_in, off_out in ((1, None), (3, None), (4, None), (1, 0), (0, 1), (3, 2), (2, 2), (4, 64)):
            resident(pb3d_gpu, case, want, removed, off_in, off_out)


@gpu
def test_view_counts_and_sequence(pb3d_gpu, cases):
    case, want9, removed9 = cases["views9"]
    views, grid = case["views"], case["grid"]
    assert len(views) == 9
    assert len({np.asarray(m).dtype for m, _ in views}) >= 2 and any(np.asarray(m).ndim == 3 for m, _ in views)
    assert all(np.asarray(m).shape[1] % 32 for m, _ in views) and len({np.asarray(m).shape[:2] for m, _ in views}) == 9
    got = {}
    for K in (0, 1, 3, 9):
        g, rem = run(pb3d_gpu, case, views[:K])
        want, wrem = pr.carve(grid, views[:K])
        assert np.array_equal(g, want) and rem.shape == (K,) and rem.dtype == np.int64 and np.array_equal(rem, wrem), K
        assert np.array_equal(rem, removed9[:K]), K          # the counts of a prefix are a prefix of the counts
        got[K] = g
    assert np.array_equal(got[0], grid) and got[0] is not grid
    assert np.array_equal(got[9], want9)
    # [a, b] is a, then b on its result; the counts concatenate (also across the 8-view launch boundary)
    for cut in (1, 3, 8):
        first, r1 = run(pb3d_gpu, case, views[:cut])
        second, r2 = pb3d_gpu.perspective_carve(first, views[cut:], return_counts=True)
        assert np.array_equal(second, want9) and np.array_equal(np.concatenate([r1, r2]), removed9), cut
    # carving twice is carving once
    again, r = pb3d_gpu.perspective_carve(want9, views, return_counts=True)
    assert np.array_equal(again, want9) and not r.any()
    # the order of the views decides the counts, not the result
    back, rb = run(pb3d_gpu, case, views[::-1])
    assert np.array_equal(back, want9) and rb.sum() == removed9.sum() and not np.array_equal(rb[::-1], removed9)


@gpu
def test_device_grid_in_and_out(pb3d_gpu, cases):
    dev = pb3d_gpu.device
    for name in ("views9", "walk_lab_12x10x16"):
        case, want, removed = cases[name]
        dg = dev.DeviceGrid(dev.from_numpy(case["grid"]), case["grid"].shape)
        res, rem = pb3d_gpu.perspective_carve(dg, case["views"], return_counts=True)
        try:
            assert isinstance(res, dev.DeviceGrid) and res.shape == case["grid"].shape and res.buf.ptr != dg.buf.ptr
            assert np.array_equal(res.numpy(), want) and np.array_equal(rem, removed)
            assert np.array_equal(dg.numpy(), case["grid"])
        finally:
            res.free(); dg.free()
    # masks uploaded once (what the timing tool does) stand for the host ones
    case, want, removed = cases["views9"]
    masks = [pb3d_gpu.perspective._DeviceMaskBits(m) for m, _ in case["views"]]
    try:
        got, rem = pb3d_gpu.perspective_carve(case["grid"], [(mb, c) for mb, (_, c) in zip(masks, case["views"])], return_counts=True)
        assert np.array_equal(got, want) and np.array_equal(rem, removed)
    finally:
        for mb in masks:
            mb.free()
    empty, rem = pb3d_gpu.perspective_carve(np.zeros((0, 4, 5, 3), np.uint8), case["views"][:2], return_counts=True)
    assert empty.shape == (0, 4, 5, 3) and rem.tolist() == [0, 0]


@gpu
def test_arithmetic_paths(pb3d_gpu, cases):
    from pb3d.projection_utils import camera_args
    flags = {}
    for name in ("arith_f32", "arith_cx64", "arith_f64scale", "arith_f64cam", "arith_inside", "outside_carve", "outside_keep", "half_even"):
        case, want, removed = check(pb3d_gpu, cases, name)
        cam = case["views"][0][1]
        flags[name] = list(camera_args(np.zeros((1, 3), np.float32), cam["cam_pos"], cam["target"], cam["f"], cam["cx"], cam["cy"])[4])
    # the cases do take the promotion paths they are named for
    assert flags["arith_f32"] == [0, 0, 0, 0] and flags["arith_cx64"] == [0, 0, 1, 0]
    assert flags["arith_f64scale"] == [0, 1, 1, 1] and flags["arith_f64cam"] == [1, 1, 1, 1]
    # behind the camera: the clamp sends a voxel off the image unless it sits on the optical axis
    case, want, _ = cases["arith_inside"]
    from test_visibility_kernels import ref_frame
    pts, (a0, a1, a2) = pr.points_of(pr.subject(case["grid"]))
    X, Y, Z = ref_frame(pts, case["views"][0][1])
    behind, on_axis = Z < 1e-8, (X == 0) & (Y == 0)
    assert behind.sum() > 100 and (behind & on_axis).sum() == 1          # the voxel the camera sits in lands on (cx, cy), a set pixel
    assert np.array_equal(want[a0[behind], a1[behind], a2[behind]].any(axis=-1), on_axis[behind])
    # a mask smaller than the projection: what lands outside it goes, or stays
    keep, carve = cases["outside_keep"], cases["outside_carve"]
    assert np.array_equal(keep[0]["grid"], carve[0]["grid"]) and keep[2][0] < carve[2][0]
    gone_keep, gone_carve = ~pr.subject(keep[1]), ~pr.subject(carve[1])
    assert (gone_carve & ~gone_keep).sum() == carve[2][0] - keep[2][0] and not (gone_keep & ~gone_carve).any()


@gpu
def test_subject_colours(pb3d_gpu, cases):
    for name in ("colors_rgb_none", "colors_rgb_1", "colors_rgb_3", "colors_lab_none", "colors_lab_1", "colors_lab_3"):
        case, want, removed = cases[name]
        got, rem = run(pb3d_gpu, case)
        assert np.array_equal(got, want) and np.array_equal(rem, removed), name
        other = ~pr.subject(case["grid"], case["colors"])
        assert other.any() and np.array_equal(got[other], case["grid"][other]), name
        assert 0 < rem[0] < pr.subject(case["grid"], case["colors"]).sum(), name
        resident(pb3d_gpu, case, want, removed, 0, None)
        resident(pb3d_gpu, case, want, removed, 1, 3)


@gpu
def test_stored_monument(pb3d_gpu):
    from pb3d.config import PART_COLORS
    meta = json.load(open(os.path.join(pr.GOLDEN, "pcarve_charminar.json")))
    grid, views = pr.stored_case(meta["monument"])
    bg = np.array(PART_COLORS["background"], np.uint8)
    views = [(np.any(m != bg, axis=-1), c) for m, c in views]
    assert meta["runs"]["minarets"]["colors"] == [list(PART_COLORS["front_minarets"]), list(PART_COLORS["back_minarets"])]
    with np.load(os.path.join(pr.GOLDEN, "pcarve_charminar.npz")) as z:
        for run_name, rec in meta["runs"].items():
            got, rem = pb3d_gpu.perspective_carve(grid, views, colors=rec["colors"], outside=rec["outside"], return_counts=True)
            assert rem.tolist() == rec["removed"], run_name
            assert pr.sha(got) == rec["sha256"], run_name
            assert np.array_equal(pr.keep_bits(got), z[f"{run_name}/keep_bits"]), run_name
