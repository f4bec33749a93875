"""perspective_paint on the device (csrc/ppaint.hip) against the committed fixtures of tests/golden/ppaint_*: every comparison is exact
equality of grids, counts and digests.  The fixtures come from tests/paint_restate.py, which the generator ties to the reference's
compute_global_depth_buffer and project_part_visible and tests/test_perspective_paint_host.py re-runs on the CPU.

Shapes are the smallest that reach each path of the kernel: A0 = 70 crosses the 64-step chunk of the walk, A2 = 13 is ragged (byte
loads and stores), A2 = 16 on an aligned buffer moves whole dwords (C = 1: one, C = 3: three per lane), the same rows at an odd base
fall back to bytes; images are read by bytes at any base."""
import json
import os

import numpy as np
import pytest

import paint_restate as pt

gpu = pytest.mark.gpu
GUARD = 256


@pytest.fixture(scope="module")
def cases():
    return pt.load_synthetic()


def run(pb3d, case, grid=None, **kw):
    return pb3d.perspective_paint(case["grid"] if grid is None else grid, case["views"], colors=case["colors"], skip=case["skip"], eps=case["eps"],
                                  zbufs=case["zbufs"], **kw)


def resident(pb3d, case, want, decided, off_in, off_out, off_img=0):
    """the resident entry on windows into guarded arenas (tests/test_pointer_offsets.py): off_out None = in place; every image starts
    off_img bytes into its arena"""
    dev = pb3d.device
    grid = case["grid"]
    shape = grid.shape if grid.ndim == 4 else grid.shape + (1,)
    n, K = grid.nbytes, len(case["views"])

    def arena(off, fill, nbytes, payload=None):
        host = np.full(GUARD + off + nbytes + GUARD, fill, np.uint8)
        if payload is not None:
            host[GUARD + off:GUARD + off + nbytes] = payload.reshape(-1)
        return dev.from_numpy(host), host

    a_in, h_in = arena(off_in, 0xFF, n, grid)
    a_out, h_out = (a_in, h_in) if off_out is None else arena(off_out, 0xA5, n)
    off_o = off_in if off_out is None else off_out
    imgs = [arena(off_img, 0x5A, im.nbytes, im) for im, _ in case["views"]]
    d_cnt = dev.DeviceBuffer(8 * K + 16)
    d_z = []
    try:
        d_cnt.upload(np.full(K + 2, -7, np.int64))
        d_plain = dev.from_numpy(grid)                  # the z-buffers of the input grid, made on the device as perspective_paint makes them
        d_z.append(d_plain)
        for k, (im, cam) in enumerate(case["views"]):
            d_z.append(dev.from_numpy(case["zbufs"][k]) if case["zbufs"] is not None else
                       pb3d.eval_helpers_intra.depth_buffer_resident(d_plain, shape, cam, *im.shape[:2]))
        views = [(pb3d.perspective._DeviceImage(a.at(GUARD + off_img), *im.shape[:2]), cam) for (a, _), (im, cam) in zip(imgs, case["views"])]
        ret = pb3d.perspective_paint_resident(a_in.at(GUARD + off_in), shape, views, d_z[1:], colors=case["colors"], skip=case["skip"], eps=case["eps"],
                                              out=None if off_out is None else a_out.at(GUARD + off_out), d_painted=d_cnt.at(8))
        assert ret.value == a_out.ptr + GUARD + off_o
        got = a_out.download((h_out.size,))
        cnt = d_cnt.download((K + 2,), np.int64)
        what = (grid.shape, off_in, off_out, off_img)
        assert np.array_equal(got[:GUARD + off_o], h_out[:GUARD + off_o]) and np.array_equal(got[GUARD + off_o + n:], h_out[GUARD + off_o + n:]), (what, "guard")
        assert np.array_equal(got[GUARD + off_o:GUARD + off_o + n].reshape(want.shape), want), what
        assert cnt[0] == -7 and cnt[-1] == -7 and np.array_equal(cnt[1:-1], decided), (what, cnt)
        if off_out is not None:
            assert np.array_equal(a_in.download((h_in.size,)), h_in), (what, "the input changed")
        for a, h in imgs:
            assert np.array_equal(a.download((h.size,)), h), (what, "an image changed")
    finally:
        for b in list({id(a_in): a_in, id(a_out): a_out, id(d_cnt): d_cnt}.values()) + [a for a, _ in imgs] + d_z:
            b.free()


@gpu
def test_every_case_numpy_entry(pb3d_gpu, cases):
    for name, (case, want, decided) in cases.items():
        got, cnt = run(pb3d_gpu, case, return_counts=True)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), name
        assert cnt.dtype == np.int64 and cnt.shape == (len(case["views"]),) and np.array_equal(cnt, decided), (name, cnt, decided)
        assert np.array_equal(run(pb3d_gpu, case), want), name
    case, _, _ = cases["walk_rgb_5x7x16"]
    none, cnt = pb3d_gpu.perspective_paint(case["grid"], [], return_counts=True)
    assert np.array_equal(none, case["grid"]) and none is not case["grid"] and cnt.shape == (0,) and cnt.dtype == np.int64
    empty, cnt = pb3d_gpu.perspective_paint(np.zeros((0, 4, 5, 3), np.uint8), case["views"], return_counts=True)
    assert empty.shape == (0, 4, 5, 3) and cnt.tolist() == [0, 0]


@gpu
def test_every_case_device_grid(pb3d_gpu, cases):
    dev = pb3d_gpu.device
    for name, (case, want, decided) in cases.items():
        dg = dev.DeviceGrid(dev.from_numpy(case["grid"]), case["grid"].shape)
        res, cnt = run(pb3d_gpu, case, grid=dg, return_counts=True)
        try:
            assert isinstance(res, dev.DeviceGrid) and res.shape == case["grid"].shape and res.buf.ptr != dg.buf.ptr, name
            assert np.array_equal(res.numpy(), want) and np.array_equal(cnt, decided), name
            assert np.array_equal(dg.numpy(), case["grid"]), name
        finally:
            res.free(); dg.free()
    # z-buffers that are resident already stand for the host ones
    case, want, decided = cases["zbuf_other"]
    zb = [dev.from_numpy(z) for z in case["zbufs"]]
    try:
        got, cnt = pb3d_gpu.perspective_paint(case["grid"], case["views"], skip=case["skip"], zbufs=zb, return_counts=True)
        assert np.array_equal(got, want) and np.array_equal(cnt, decided)
    finally:
        for b in zb:
            b.free()


@gpu
def test_resident_in_place_and_out_of_place(pb3d_gpu, cases):
    for name, (case, want, decided) in cases.items():
        resident(pb3d_gpu, case, want, decided, 0, None)      # the same `want`: in place and out of place are equal
        resident(pb3d_gpu, case, want, decided, 0, 0)


@gpu
def test_odd_byte_offsets(pb3d_gpu, cases):
    """rows of whole dwords (A2 = 16) whose base is not 4-byte aligned, in either buffer or both, and images at any base"""
    for name in ("walk_rgb_5x7x16", "walk_lab_12x10x16"):
        case, want, decided = cases[name]
        for off_in, off_out, off_img in ((1, None, 0), (2, None, 3), (3, None, 1), (4, None, 2), (64, None, 4), (1, 0, 64), (0, 1, 1), (3, 2, 2),
                                         (2, 2, 3), (4, 64, 4), (64, 4, 64), (0, 3, 0)):
            resident(pb3d_gpu, case, want, decided, off_in, off_out, off_img)
    case, want, decided = cases["walk_rgb_70x9x13"]
    for off_in, off_out, off_img in ((1, None, 1), (2, 3, 2), (4, 64, 3)):
        resident(pb3d_gpu, case, want, decided, off_in, off_out, off_img)


@gpu
def test_run_to_run_and_repainting(pb3d_gpu, cases):
    case, want, decided = cases["views8"]
    assert len(case["views"]) == 8
    for _ in range(3):
        got, cnt = run(pb3d_gpu, case, return_counts=True)
        assert np.array_equal(got, want) and np.array_equal(cnt, decided)
    # Painting the result again with the same views and the same z-buffers changes nothing.  Occupancy is unchanged, so a view sees
    # and paints a voxel exactly as before: with colors=None the subject voxels are the same and so are the counts.  A colour subset
    # names the subject voxels by the colour they hold when the call starts; after the first call some of them hold an image colour
    # outside the subset and are copied, so there the counts are those of the restatement on the painted grid (never more than before).
    for name, (case, want, decided) in cases.items():
        zb = case["zbufs"] if case["zbufs"] is not None else pt.zbuffers(case["grid"], case["views"])
        again, cnt = pb3d_gpu.perspective_paint(want, case["views"], colors=case["colors"], skip=case["skip"], eps=case["eps"], zbufs=zb,
                                                return_counts=True)
        assert np.array_equal(again, want), name
        if case["colors"] is None:
            assert np.array_equal(cnt, decided), (name, cnt, decided)
        else:
            _, expect = pt.paint(want, case["views"], case["colors"], case["skip"], case["eps"], zb)
            assert np.array_equal(cnt, expect) and (cnt <= decided).all() and cnt.sum() > 0, (name, cnt, expect, decided)


@gpu
def test_stored_monument(pb3d_gpu):
    meta = json.load(open(os.path.join(pt.GOLDEN, "ppaint_charminar.json")))
    grid, views = pt.stored_case(meta["monument"])
    got, cnt = pb3d_gpu.perspective_paint(grid, views, skip=[tuple(c) for c in meta["skip"]], eps=pt.eps_from_record(meta["eps"]), return_counts=True)
    assert cnt.tolist() == meta["decided"]
    assert pt.sha(got) == meta["sha256"]
    at, vals = pt.changed_sample(grid, got)
    with np.load(os.path.join(pt.GOLDEN, "ppaint_charminar.npz")) as z:
        assert np.array_equal(at, z["sample/index"]) and np.array_equal(vals, z["sample/value"])
