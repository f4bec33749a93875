"""The fused component loop of left_right_guided_carve (csrc/guided.hip: k_crop_cells, k_crop_slice, k_crop_chain<NB>) on crops large
enough for every form of k_crop_chain, and the four pb3d_guided_carve*_dev entries called directly.

k_crop_chain<NB> is compiled in four forms, picked per batch of components from the largest crop's x-z cell count
(nbt = ceil(Wc * Dc / 4096): 1 -> <1>, 2 -> <2>, 3 -> <3>, 4 and 5 -> <5>).  The scenes of tests/guided_scenes.py reach all five
classes, crops deeper than a workgroup (Dc > 512), one voxel deep, wide or high, two and three plane groups, more components than a
batch holds, overlapping boxes (the copy-and-restore path) and the first square crop that does not fit the LDS.  Everything compared
here is an integer -- voxel bytes, counts, the printed log -- so every comparison is exact.

CPU tests: the oracle's left_right_guided_carve against the SciPy restatement on every scene (a pin of the oracle on shapes that are
no fixture), and the condition that lets the overlap scene fail at all.  GPU tests: the public functions against the oracle, then the
C entries through ctypes: whether the fused loop ran (`took`), the path without membership bits, the guard that refuses a label volume
whose bits are gone, the argument refusals, the queued entry with a colour index above 0."""
import contextlib
import ctypes as C
import io
import re

import numpy as np
import pytest

import guided_scenes as gs

gpu = pytest.mark.gpu

_want = {}


def captured(fn, *args, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = fn(*args, **kw)
    return res, buf.getvalue()


def log_counts(log):
    return np.array([int(v) for v in re.findall(r"carved voxels: (\d+)", log)], np.int64)


def want(oracle, name, angle):
    """(grid, printed log, carved-voxel counts) of the oracle on a scene, computed once per process"""
    key = (name, angle)
    if key not in _want:
        sc = gs.scene(name)
        g, log = captured(oracle.left_right_guided_carve, sc.grid, sc.sem, sc.color, angle=angle)
        g.setflags(write=False)
        _want[key] = (g, log, log_counts(log))
    return _want[key]


def differing(a, b):
    return int((a != b).reshape(a.shape[0], a.shape[1], a.shape[2], -1).any(-1).sum())


# =====================================================================================================================
# CPU: the scenes hold what they claim; oracle == restatement; the overlap scene can fail
# =====================================================================================================================

def test_scenes_hold_their_claims():
    """component counts, bounding boxes and nbt classes from scipy.ndimage.label of every scene (asserted inside gs.scene)"""
    for name in gs.NAMES + ("corner_small",):
        sc = gs.scene(name)
        assert sc.grid.dtype == np.uint8 and sc.sem.shape == (sc.shape[1], sc.shape[0], 3)
    assert {gs.nbt_of(b) for n in gs.FUSED for b in gs.scene(n).boxes} == {1, 2, 3, 4, 5}
    assert gs.nbt_classes() == {1, 2, 3, 4, 5}
    assert not any(gs.fits_lds(b) for b in gs.scene("over").boxes)
    assert gs.fits_lds((0, 0, 0, 137, 1, 137)) and not gs.fits_lds((0, 0, 0, 138, 1, 138))
    # Dc > 512: a workgroup's 512 threads never leave a row of cells; Dc == 1, Wc == 1, Hc == 1: each present
    crops = [tuple(int(b[3 + a] - b[a]) for a in range(3)) for n in gs.FUSED for b in gs.scene(n).boxes]
    assert any(c[2] > 512 for c in crops) and any(c[2] == 1 for c in crops) and any(c[0] == 1 for c in crops) and any(c[1] == 1 for c in crops)


def test_two_part_scene_is_what_part_carve_leaves(oracle):
    grid, sem, masked, boxes = gs.two_part()
    assert np.array_equal(oracle.part_carve(grid, sem, gs.TWO_PART_JOBS), masked)
    assert [gs.nbt_of(boxes[p][0]) for p in ("dome", "plinth", "main_door")] == [3, 2, 1]


@pytest.mark.parametrize("name", gs.NAMES)
def test_oracle_equals_restatement(oracle, name):
    sc = gs.scene(name)
    for angle in (5, 45):
        g, log, counts = want(oracle, name, angle)
        rg, comps = gs.restate(sc.grid, sc.sem, sc.color, angle)
        assert np.array_equal([c[0] for c in comps], sc.boxes), (name, angle)
        assert np.array_equal(g, rg), (name, angle, differing(g, rg))
        assert log == gs.log_text(sc.color, comps), (name, angle)
        assert counts.tolist() == [c[1] for c in comps], (name, angle)
        assert not np.array_equal(g, sc.grid), (name, angle, "nothing was carved")


def test_overlap_scene_discriminates(oracle):
    """a carve that cuts later crops from the grid as carved so far is wrong on `ell`, at every tested angle"""
    sc = gs.scene("ell")
    for angle in gs.ANGLES["ell"]:
        g, _, _ = want(oracle, "ell", angle)
        wg, _ = gs.restate(sc.grid, sc.sem, sc.color, angle, wrong=True)
        n = differing(g, wg)
        print("ell, angle", angle, ":", n, "voxels differ in the wrong variant")
        assert n >= 1, angle


# =====================================================================================================================
# GPU: the public functions
# =====================================================================================================================

@gpu
@pytest.mark.parametrize("name", gs.NAMES)
def test_public_api_matches_oracle(pb3d_gpu, oracle, name):
    sc = gs.scene(name)
    for angle in gs.ANGLES[name]:
        g, log, _ = want(oracle, name, angle)
        got, got_log = captured(pb3d_gpu.left_right_guided_carve, sc.grid, sc.sem, sc.color, angle=angle)
        assert np.array_equal(got, g), (name, angle, differing(got, g))
        assert got_log == log, (name, angle)


@gpu
@pytest.mark.parametrize("name", ["nb3_nb2", "nb5_corner", "ell", "over"])
def test_label_form_matches_oracle(pb3d_gpu, oracle, name):
    sc = gs.scene(name)
    pal = pb3d_gpu.Palette.from_part_colors(pb3d_gpu.PART_COLORS)
    lab, lab_sem = pb3d_gpu.rgb_to_label(sc.grid, pal), pal.mask_to_labels(sc.sem)
    assert np.array_equal(pb3d_gpu.label_to_rgb(lab, pal), sc.grid)
    for angle in gs.ANGLES[name]:
        g, log, _ = want(oracle, name, angle)
        gl, got_log = captured(pb3d_gpu.left_right_guided_carve_labels, lab, lab_sem, pal.label_of("dome"), angle=angle, log_color=sc.color)
        got = pb3d_gpu.label_to_rgb(gl, pal)
        assert np.array_equal(got, g), (name, angle, differing(got, g))
        assert got_log == log, (name, angle)


@gpu
def test_partwise_carve_two_parts(pb3d_gpu, oracle):
    """the queued entry behind ONE labelling of three colours: colour index 0 at <3>, 1 at <2>, 2 at <1>"""
    from pb3d import device as dev
    grid, sem, _, _ = gs.two_part()
    args = (sem, sem, gs.PCN, gs.TWO_PART_JOBS, gs.TWO_PART_SYMMETRY, {})
    g, log = captured(oracle.partwise_carve, grid, *args, recolor_back_minarets=False)
    assert log.count("3D components") == 3 and "bbox (1,1,4) → (93,34,95)" in log and "bbox (3,36,2) → (68,69,67)" in log
    got, got_log = captured(pb3d_gpu.partwise_carve, grid, *args, recolor_back_minarets=False)
    assert np.array_equal(got, g), differing(got, g)
    assert got_log == log
    d_in = dev.DeviceGrid(dev.from_numpy(grid), grid.shape)
    try:
        d_res, got_log = captured(pb3d_gpu.partwise_carve, d_in, *args, recolor_back_minarets=False)
        got = d_res.numpy()
        d_res.free()
    finally:
        d_in.free()
    assert np.array_equal(got, g), differing(got, g)
    assert got_log == log


# =====================================================================================================================
# GPU: the C entries
# =====================================================================================================================

CAP = 256


class Entries:
    """the label and carve entries of libpb3d.so on DeviceBuffers, as ctypes calls; every buffer made through buf() is freed by close()"""

    def __init__(self, pb3d):
        from pb3d import device as dev
        self.pb3d, self.dev, self.L = pb3d, dev, pb3d._lib
        self.lib, self.ctx = self.L.load(), self.L.ctx()
        self.live = []

    def buf(self, array=None, nbytes=None):
        b = self.dev.from_numpy(array) if array is not None else self.dev.DeviceBuffer(nbytes)
        self.live.append(b)
        return b

    def close(self):
        for b in self.live:
            b.free()
        self.live = []

    def error(self):
        return self.lib.pb3d_last_error().decode()

    def labels_buf(self, shape, fill=1):
        """a label volume that holds `fill` everywhere: a members-only labelling leaves that at every voxel that is no member, and 1 is
        the id of a component, so a kernel that read such a label would clear voxels that are not the component's"""
        return self.buf(np.full(int(np.prod(shape)), fill, np.int32))

    def label(self, d_grid, shape, colors, d_lab, members_only, channels=3):
        """one labelling of K colours (K x 3 bytes) or label values -> [boxes per colour]"""
        W, H, D = shape
        cols = np.ascontiguousarray(colors, np.uint8).reshape(-1, channels if channels == 3 else 1)
        K = len(cols)
        n = (C.c_int64 * K)(); ok = (C.c_int * K)()
        bbox = np.zeros((K, CAP, 6), np.int64); cnt = np.zeros((K, CAP), np.int64); sums = np.zeros((K, CAP, 3), np.int64)
        p = lambda a: a.ctypes.data_as(self.L.i64p)
        if K == 1 and channels == 3:
            rc = self.lib.pb3d_label_color_stats_dev(self.ctx, C.c_void_p(d_grid.ptr), W, H, D, self.L.p_u8(cols), C.c_void_p(d_lab.ptr), n, CAP, members_only,
                                                     p(bbox), p(cnt), p(sums), ok)
        else:
            fn = self.lib.pb3d_label_colors_stats_dev if channels == 3 else self.lib.pb3d_label_values_stats_dev
            rc = fn(self.ctx, C.c_void_p(d_grid.ptr), W, H, D, self.L.p_u8(cols), K, C.c_void_p(d_lab.ptr), n, CAP, members_only, p(bbox), p(cnt), p(sums), ok)
        self.L.check(rc)
        assert all(ok[k] == 1 for k in range(K))
        return [bbox[k, :n[k]].copy() for k in range(K)]

    def carve(self, entry, d_grid, d_lab, shape, boxes, masks, offs, angle, color_index=0, channels=3, d_counts=None, mask_bytes=None):
        """-> (return code, took, host counts); entry: 'rgb', 'label', 'color', 'queue'"""
        W, H, D = shape
        bb = np.ascontiguousarray(boxes, np.int64); mo = np.ascontiguousarray(offs, np.int64); mk = np.ascontiguousarray(masks, np.uint8)
        n = len(bb)
        cn = np.full(max(n, 1), -1, np.int64)
        took = C.c_int(-1)
        mbytes = mk.size if mask_bytes is None else mask_bytes
        tail = (n, bb.ctypes.data_as(self.L.i64p), self.L.p_u8(mk), mo.ctypes.data_as(self.L.i64p), mbytes, angle)
        g, l = C.c_void_p(d_grid.ptr), C.c_void_p(d_lab.ptr)
        if entry in ("rgb", "label"):
            fn = self.lib.pb3d_guided_carve_dev if entry == "rgb" else self.lib.pb3d_guided_carve_label_dev
            rc = fn(self.ctx, g, l, W, H, D, *tail, cn.ctypes.data_as(self.L.i64p), C.byref(took))
        elif entry == "color":
            rc = self.lib.pb3d_guided_carve_color_dev(self.ctx, g, l, color_index, channels, W, H, D, *tail, cn.ctypes.data_as(self.L.i64p), C.byref(took))
        else:
            rc = self.lib.pb3d_guided_carve_queue_dev(self.ctx, g, l, color_index, channels, W, H, D, *tail, C.c_void_p(d_counts.ptr), C.byref(took))
        return rc, took.value, cn[:n]

    def sync(self):
        self.L.check(self.lib.pb3d_sync(self.ctx))


@pytest.fixture
def entries(pb3d_gpu):
    e = Entries(pb3d_gpu)
    try:
        yield e
    finally:
        e.close()


def label_and_carve(e, sc, angle, d_grid, d_lab, masks, offs):
    """the package's pair of calls on a freshly uploaded scene: members-only labelling, then the fused loop -> (took, counts, grid)"""
    d_grid.upload(sc.grid)
    boxes, = e.label(d_grid, sc.shape, sc.color, d_lab, 1)
    assert np.array_equal(boxes, sc.boxes), sc.name
    rc, took, counts = e.carve("rgb", d_grid, d_lab, sc.shape, boxes, masks, offs, angle)
    e.L.check(rc)
    return took, counts, d_grid.download(sc.grid.shape)


@gpu
@pytest.mark.parametrize("name", gs.NAMES)
def test_entry_took(entries, oracle, name):
    """every scene whose crops fit the LDS is carved by the fused loop (took == 1: no silent fallback) with the oracle's grid and
    counts; the first square that does not fit comes back untouched with took == 0"""
    e, sc = entries, gs.scene(name)
    d_grid, d_lab = e.buf(nbytes=sc.grid.nbytes), e.labels_buf(sc.shape)
    masks, offs = gs.crop_masks(sc.sem, sc.color, sc.boxes)
    for angle in (5, 45):
        took, counts, got = label_and_carve(e, sc, angle, d_grid, d_lab, masks, offs)
        if name == "over":
            assert took == 0 and np.array_equal(got, sc.grid), (name, angle, took)
            continue
        g, _, wc = want(oracle, name, angle)
        assert took == 1, (name, angle)
        assert np.array_equal(got, g), (name, angle, differing(got, g))
        assert counts.tolist() == wc.tolist(), (name, angle)


@gpu
@pytest.mark.parametrize("name", ["nb2", "ell"])
def test_entry_without_membership_bits(entries, oracle, name):
    """a FULL label volume that is not the context's last labelling: the kernel reads labels[] at every candidate voxel (mbits64 == nullptr)"""
    e, sc, small = entries, gs.scene(name), gs.scene("plate_z")
    d_grid, d_l1 = e.buf(nbytes=sc.grid.nbytes), e.labels_buf(sc.shape, fill=-7)
    d_small, d_l2 = e.buf(small.grid), e.labels_buf(small.shape)
    masks, offs = gs.crop_masks(sc.sem, sc.color, sc.boxes)
    for angle in (5, 45):
        d_grid.upload(sc.grid)
        boxes, = e.label(d_grid, sc.shape, sc.color, d_l1, 0)
        assert np.array_equal(boxes, sc.boxes)
        e.label(d_small, small.shape, small.color, d_l2, 1)              # the context's membership bits now belong to L2
        rc, took, counts = e.carve("rgb", d_grid, d_l1, sc.shape, boxes, masks, offs, angle)
        e.L.check(rc)
        g, _, wc = want(oracle, name, angle)
        got = d_grid.download(sc.grid.shape)
        assert took == 1 and np.array_equal(got, g), (name, angle, took, differing(got, g))
        assert counts.tolist() == wc.tolist(), (name, angle)


@gpu
def test_entry_guard_bits_gone(entries, oracle):
    """a members-only (or multi-colour) label volume whose membership bits do not answer for this call is refused with the advice to
    label again, before anything is written; the context goes on working"""
    e, sc, angle = entries, gs.scene("nb2"), 45
    W, H, D = sc.shape
    d_grid, d_lab = e.buf(nbytes=sc.grid.nbytes), e.labels_buf(sc.shape)
    masks, offs = gs.crop_masks(sc.sem, sc.color, sc.boxes)
    g, _, wc = want(oracle, "nb2", angle)
    cases = [("colour index beyond a one-colour labelling", "color", (W, H, D), dict(color_index=1)),
             ("D does not match the labelling", "rgb", (W, H, D + 1), {}),
             ("W * H does not match the labelling", "rgb", (W + 1, H, D), {})]
    for what, entry, dims, kw in cases:
        d_grid.upload(sc.grid)
        boxes, = e.label(d_grid, sc.shape, sc.color, d_lab, 1)
        rc, took, _ = e.carve(entry, d_grid, d_lab, dims, boxes, masks, offs, angle, **kw)
        assert rc == -1 and took == 0 and "label again" in e.error(), (what, rc, took, e.error())
        assert np.array_equal(d_grid.download(sc.grid.shape), sc.grid), what
        took, counts, got = label_and_carve(e, sc, angle, d_grid, d_lab, masks, offs)
        assert took == 1 and np.array_equal(got, g) and counts.tolist() == wc.tolist(), what


@gpu
def test_entry_argument_refusals(entries, oracle):
    e, sc, angle = entries, gs.scene("nb2"), 45
    W, H, D = sc.shape
    d_grid, d_lab, d_cnt = e.buf(nbytes=sc.grid.nbytes), e.labels_buf(sc.shape), e.buf(nbytes=8 * len(sc.boxes))
    masks, offs = gs.crop_masks(sc.sem, sc.color, sc.boxes)
    g, _, wc = want(oracle, "nb2", angle)
    outside, empty = sc.boxes.copy(), sc.boxes.copy()
    outside[0, 3] = W + 1
    empty[0, 3] = empty[0, 0]
    cases = [("a box outside the grid", "rgb", dict(boxes=outside)), ("an empty box", "rgb", dict(boxes=empty)),
             ("a mask offset past mask_bytes", "rgb", dict(offs=np.array([masks.size], np.int64))),
             ("angle_interval 0", "rgb", dict(angle=0)), ("angle_interval -5", "rgb", dict(angle=-5)),
             ("channels 2, colour entry", "color", dict(channels=2)), ("channels 2, queue entry", "queue", dict(channels=2, d_counts=d_cnt))]
    for what, entry, kw in cases:
        d_grid.upload(sc.grid)
        boxes, = e.label(d_grid, sc.shape, sc.color, d_lab, 1)
        a = dict(boxes=boxes, masks=masks, offs=offs, angle=angle)
        a.update(kw)
        rc, took, _ = e.carve(entry, d_grid, d_lab, sc.shape, a.pop("boxes"), a.pop("masks"), a.pop("offs"), a.pop("angle"), **a)
        assert rc == -1 and took != 1 and e.error(), (what, rc, took)
        assert np.array_equal(d_grid.download(sc.grid.shape), sc.grid), what
        took, counts, got = label_and_carve(e, sc, angle, d_grid, d_lab, masks, offs)
        assert took == 1 and np.array_equal(got, g) and counts.tolist() == wc.tolist(), what


@gpu
@pytest.mark.parametrize("channels", [3, 1])
def test_entry_queue_second_colour(entries, oracle, channels):
    """pb3d_guided_carve_queue_dev for colour index 1 of a two-colour labelling, on the colour grid and on its 1-byte label volume:
    the counts stay on the device until pb3d_sync"""
    e, angle = entries, 45
    _, sem, masked, boxes = gs.two_part()
    shape = masked.shape[:3]
    color = gs.PCN["plinth"]
    g, log = captured(oracle.left_right_guided_carve, masked, sem, color, angle=angle)
    wc = log_counts(log)
    pal = np.array([gs.PCN[p] for p in ("dome", "plinth", "main_door", "windows")], np.uint8)

    def to_label(rgb):
        lab = np.zeros(rgb.shape[:3], np.uint8)
        for k, c in enumerate(pal, 1):
            lab[np.all(rgb == c, axis=-1)] = k
        assert np.array_equal(np.concatenate([np.zeros((1, 3), np.uint8), pal])[lab], rgb)
        return lab

    vol, wanted = (masked, g) if channels == 3 else (to_label(masked), to_label(g))
    colors = pal[:2] if channels == 3 else np.array([1, 2], np.uint8)
    d_grid, d_lab = e.buf(vol), e.labels_buf(shape)
    per_colour = e.label(d_grid, shape, colors, d_lab, 1, channels=channels)
    assert np.array_equal(per_colour[0], boxes["dome"]) and np.array_equal(per_colour[1], boxes["plinth"])
    bx = per_colour[1]
    assert len(bx) == len(wc)
    d_cnt = e.buf(np.full(len(bx), -3, np.int64))
    masks, offs = gs.crop_masks(sem, color, bx)
    rc, took, _ = e.carve("queue", d_grid, d_lab, shape, bx, masks, offs, angle, color_index=1, channels=channels, d_counts=d_cnt)
    e.L.check(rc)
    assert took == 1
    masks[:] = 0; offs[:] = -1                  # every host argument may be reused on return
    e.sync()
    assert d_cnt.download((len(bx),), np.int64).tolist() == wc.tolist()
    got = d_grid.download(vol.shape)
    assert np.array_equal(got, wanted), differing(got, wanted)
