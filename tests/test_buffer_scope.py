"""pb3d.device.Scope, the one owner of a wrapper's temporary device buffers: its contract on fake buffers, and every NumPy-form
wrapper that stages buffers driven against a stub library that counts live device blocks -- none may be left behind when the entry
fails or when any one of the wrapper's allocations fails.  No device is needed.

Wrappers the stub cannot drive past their first entry (at most three may stand here):
  * pb3d.device.meshify / meshify of a DeviceGrid: its four buffers are sized by the vertex and face counts the first entry writes
    through pointer arguments, and the stub's entries fail before writing anything.
  * evaluate_part_deform_batch: its points come from the host entry of get_voxel_points_by_parts before anything is uploaded
    (build_deformed_grid stands for pb3d/deformation_estimation.py)."""
import ctypes as C

import numpy as np
import pytest

import pb3d
from pb3d import _lib
from pb3d import device as dev

ENOMEM = -3     # PB3D_ENOMEM


# ---- 1. the scope's contract ---------------------------------------------------------------------------------------------------------
class Fake:
    def __init__(self, log, name, fail=False):
        self.log, self.name, self.fail = log, name, fail

    def free(self):
        self.log.append(self.name)
        if self.fail:
            raise RuntimeError(f"free of {self.name}")


@pytest.fixture
def fake_alloc(monkeypatch):
    """DeviceBuffer replaced by fakes named b0, b1, ... that record their free()"""
    log = []

    class FakeBuffer(Fake):
        def __init__(self, nbytes):
            super().__init__(log, f"b{sum(1 for _ in made)}")
            self.nbytes, self.uploaded = nbytes, None
            made.append(self)

        def upload(self, a):
            self.uploaded = ("sync", a.copy())
            return self

        def upload_async(self, a):
            self.uploaded = ("async", a.copy())
            return self

    made = []
    monkeypatch.setattr(dev, "DeviceBuffer", FakeBuffer)
    return log, made


def test_scope_releases_in_reverse_order_on_normal_exit(fake_alloc):
    log, _ = fake_alloc
    with dev.Scope() as sc:
        a = sc.alloc(8)
        b = sc.adopt(Fake(log, "adopted"))
        c = sc.upload(np.arange(3))
        assert (a.nbytes, c.nbytes) == (8, np.arange(3).nbytes) and b.name == "adopted"
        assert log == []
    assert log == ["b1", "adopted", "b0"]


def test_scope_releases_in_reverse_order_on_exception(fake_alloc):
    log, _ = fake_alloc
    with pytest.raises(KeyError):
        with dev.Scope() as sc:
            sc.alloc(8)
            sc.adopt((Fake(log, "t0"), None, Fake(log, "t1")))      # a tuple a resident form returned, with a None in it
            sc.alloc(8)
            raise KeyError("x")
    assert log == ["b1", "t1", "t0", "b0"]


def test_scope_uploads(fake_alloc):
    _, made = fake_alloc
    with dev.Scope() as sc:
        assert sc.upload(np.zeros((0, 3))) is None and sc.upload(np.zeros(0, np.uint8), wait=False) is None and made == []
        a = sc.upload(np.arange(6).reshape(2, 3).T)
        b = sc.upload(np.arange(4, dtype=np.uint8), wait=False)
    assert a.uploaded[0] == "sync" and a.uploaded[1].flags["C_CONTIGUOUS"] and np.array_equal(a.uploaded[1], np.arange(6).reshape(2, 3).T)
    assert b.uploaded[0] == "async" and b.nbytes == 4


def test_scope_result_is_kept_on_success_and_freed_on_exception_only_if_the_scope_made_it(fake_alloc):
    log, _ = fake_alloc
    with dev.Scope() as sc:
        r = sc.result(None, 16)
        t = sc.alloc(4)
    assert r.nbytes == 16 and log == [t.name]
    del log[:]
    with pytest.raises(ValueError):
        with dev.Scope() as sc:
            r = sc.result(None, 16)
            sc.alloc(4)
            raise ValueError("entry failed")
    assert log == ["b3", r.name]
    del log[:]
    mine = Fake(log, "callers_out")
    with dev.Scope() as sc:
        assert sc.result(mine, 16) is mine
    with pytest.raises(ValueError):
        with dev.Scope() as sc:
            assert sc.result(mine, 16) is mine
            raise ValueError("entry failed")
    assert log == []                                                # a caller's `out` is never freed


def test_scope_keep_and_early_free(fake_alloc):
    log, _ = fake_alloc
    with dev.Scope() as sc:
        a, b, c = sc.alloc(1), sc.alloc(2), sc.alloc(3)
        assert sc.keep(b) is b
        sc.free(a)
        assert log == ["b0"]
    assert log == ["b0", "b2"]                                      # a not twice, b not at all
    del log[:]
    with pytest.raises(KeyError):
        with dev.Scope() as sc:
            kept = sc.keep(sc.alloc(1))
            raise KeyError("x")
    assert log == [] and kept.nbytes == 1                           # kept buffers survive an exception too


def test_a_raising_free_neither_stops_the_others_nor_replaces_the_exception_in_flight():
    log = []
    with pytest.raises(KeyError, match="original"):
        with dev.Scope() as sc:
            sc.adopt(Fake(log, "first"))
            sc.adopt(Fake(log, "bad", fail=True))
            sc.adopt(Fake(log, "last"))
            raise KeyError("original")
    assert log == ["last", "bad", "first"]
    del log[:]
    with pytest.raises(RuntimeError, match="free of bad"):          # no exception in flight: the failed free is reported, after the rest
        with dev.Scope() as sc:
            sc.adopt(Fake(log, "first"))
            sc.adopt(Fake(log, "bad", fail=True))
            sc.adopt(Fake(log, "last"))
    assert log == ["last", "bad", "first"]


# ---- 2. no wrapper leaves a buffer behind -----------------------------------------------------------------------------------------------
class StubLib:
    """libpb3d with an allocator that works and entries that do not: pb3d_dev_alloc hands out fresh addresses and records them,
    pb3d_dev_free forgets them, uploads and memset succeed, every other entry returns PB3D_EINVAL.  fail_at = k makes the k-th
    allocation return PB3D_ENOMEM."""

    def __init__(self):
        self.live, self.allocs, self.fail_at, self._next = set(), 0, None, 0x10000

    def pb3d_dev_alloc(self, ctx, nbytes, ref):
        self.allocs += 1
        if self.allocs == self.fail_at:
            return ENOMEM
        self._next += 0x1000
        ref._obj.value = self._next
        self.live.add(self._next)
        return 0

    def pb3d_dev_free(self, ctx, ptr):
        self.live.remove(ptr.value)
        return 0

    def pb3d_h2d(self, *a):
        return 0

    pb3d_h2d_async = pb3d_dev_memset = pb3d_h2d

    def pb3d_last_error(self):
        return b"stub"

    def __getattr__(self, name):
        if not name.startswith("pb3d_"):
            raise AttributeError(name)
        return lambda *a: -1


@pytest.fixture
def stub(monkeypatch):
    lib = StubLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "ctx", lambda: C.c_void_p(1))
    return lib


RNG = np.random.default_rng(0)
PTS = RNG.random((10, 3))
PTS32 = PTS.astype(np.float32)
TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32) * 3 + 0.25
TET_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
PAL = pb3d.Palette.from_part_colors(pb3d.PART_COLORS)
DOME, PLINTH = (np.array(pb3d.PART_COLORS[k], np.uint8) for k in ("dome", "plinth"))
RGB = np.zeros((4, 4, 4, 3), np.uint8)
RGB[1:3, 1:3, 1:3] = DOME
LAB = np.zeros((4, 4, 4), np.uint8)
LAB[1:3, 1:3, 1:3] = PAL.label_of("dome")
OCC = (LAB != 0).astype(np.uint8)
IMG = np.zeros((8, 8, 3), np.uint8)
IMG[2:6, 2:6] = DOME
SEM4 = np.zeros((4, 4, 3), np.uint8)
SEM4[1:3, 1:3] = DOME
LAB4 = np.zeros((4, 4), np.uint8)
LAB4[1:3, 1:3] = PAL.label_of("dome")
CAM = {"cam_pos": np.array([2.0, 2.0, -20.0]), "target": np.array([2.0, 2.0, 2.0]), "f": 20.0, "cx": 4.0, "cy": 4.0}
ZBUF = np.full((8, 8), np.inf, np.float32)
JOBS = [(["dome"], 90)]
MINARETS = [pb3d.PART_COLORS["front_minarets"], pb3d.PART_COLORS["back_minarets"]]
ev, evi, ph, vcu, lb = pb3d.eval_helpers, pb3d.eval_helpers_intra, pb3d.preprocess_helpers, pb3d.voxel_carving_utils, pb3d.labels


class OnGrid:
    """a case whose grid is a DeviceGrid the caller owns: made before the wrapper runs, and the wrapper must leave its block alone"""

    def __init__(self, array, call):
        self.array, self.call, self.grid = array, call, None

    def __call__(self):
        if self.grid is None:
            self.grid = dev.DeviceGrid(dev.from_numpy(self.array), self.array.shape)
            return None
        return self.call(self.grid)


def camera_objective():
    """a long-lived owner: its four buffers are its own until close(); a failing allocation in its constructor leaves none"""
    obj = pb3d.CameraObjective(PTS32, np.tile(DOME, (10, 1)), IMG, {"dome": DOME})
    try:
        return obj(CAM)
    finally:
        obj.close()


WRAPPERS = {
    # pb3d/eval_helpers.py: every wrapper that stages buffers
    "nn_distances": lambda: ev.nn_distances(PTS, PTS32),
    "nn_distances_self": lambda: ev.nn_distances(PTS, PTS, k=2),
    "voxel_iou_counts": lambda: ev.voxel_iou_counts(PTS, PTS + 0.1),
    "pointcloud_to_voxel_grid": lambda: ev.pointcloud_to_voxel_grid(PTS, 4),
    "knn": lambda: ev.knn(PTS, PTS32, 3),
    "compute_triangle_normals": lambda: ev.compute_triangle_normals(TET_V, TET_F),
    "compute_vertex_normals": lambda: ev.compute_vertex_normals(TET_V, TET_F),
    "surface_metrics_per_vertex": lambda: ev.surface_metrics_per_vertex(TET_V, TET_F, 3),
    "point_to_mesh_distances": lambda: ev.point_to_mesh_distances(PTS, TET_V, TET_F, return_faces=True, return_closest=True),
    "sample_mesh_points": lambda: ev.sample_mesh_points(TET_V, TET_F, 5, return_faces=True),
    # pb3d/labels.py: every one
    "rgb_to_label": lambda: lb.rgb_to_label(RGB, PAL),
    "label_to_rgb": lambda: lb.label_to_rgb(LAB, PAL),
    "global_carve_labels": lambda: lb.global_carve_labels(LAB4 != 0, LAB4),
    "part_carve_labels": lambda: lb.part_carve_labels(LAB, LAB4, JOBS, PAL),
    "left_right_guided_carve_labels": lambda: lb.left_right_guided_carve_labels(LAB, LAB4, PAL.label_of("dome")),
    "extrude_from_surface_labels": lambda: lb.extrude_from_surface_labels(LAB, LAB4 != 0, 2),
    "recolor_backward_components_labels": lambda: lb.recolor_backward_components_labels(LAB, 1, 2),
    "extract_top_k_components_labels": lambda: lb.extract_top_k_components_labels(LAB, 1),
    "partwise_carve_labels": lambda: lb.partwise_carve_labels(LAB, LAB4, LAB4, PAL, JOBS, {"dome": 60}, {"dome": 1}),
    "get_voxel_points_by_parts_labels": lambda: lb.get_voxel_points_by_parts_labels(LAB, PAL, ["dome"]),
    "voxel_grid_to_points_labels": lambda: lb.voxel_grid_to_points_labels(LAB, PAL),
    # pb3d/preprocess_helpers.py: every one
    "transform_points": lambda: ph.transform_points(PTS, np.eye(4)),
    "estimate_normals": lambda: ph.estimate_normals(PTS, 3),
    "icp_align": lambda: ph.icp_align(PTS, PTS32),
    "icp_align_trimmed": lambda: ph.icp_align(PTS, PTS32, trim_fraction=0.5),
    "icp_align_plane": lambda: ph.icp_align(PTS, PTS32, method="point_to_plane", normals_k=3),
    "icp_align_plane_given_normals": lambda: ph.icp_align(PTS, PTS32, method="point_to_plane", target_normals=PTS),
    "crop_to_box": lambda: ph.crop_to_box(PTS, (0, 0, 0), (1, 1, 1), return_index=True),
    "fit_plane_ransac": lambda: ph.fit_plane_ransac(PTS, 0.1, 8),
    "symmetric_completion": lambda: ph.symmetric_completion(PTS),
    "symmetric_completion_centre": lambda: ph.symmetric_completion(PTS, (0.5, 0.5)),
    # pb3d/voxel_carving_utils.py: every one
    "process_voxel_grid_typed": lambda: vcu.process_voxel_grid(OCC.astype(np.float32), LAB4 != 0),
    "part_carve_resident": OnGrid(RGB, lambda g: vcu.part_carve(g, SEM4, JOBS)),
    "global_carve_on_device": lambda: vcu.global_carve(LAB4 != 0, SEM4, on_device=True),
    "left_right_guided_carve": lambda: vcu.left_right_guided_carve(RGB, SEM4, DOME),
    "extrude_from_surface": lambda: vcu.extrude_from_surface(RGB, LAB4 != 0, 2),
    "recolor_backward_components": lambda: vcu.recolor_backward_components(RGB, DOME, PLINTH),
    "partwise_carve": lambda: vcu.partwise_carve(RGB, SEM4, SEM4, pb3d.PART_COLORS_NP, JOBS, {"dome": 60}, {"dome": 1}),
    "partwise_carve_resident": OnGrid(RGB, lambda g: vcu.partwise_carve(g, SEM4, SEM4, pb3d.PART_COLORS_NP, JOBS, {"dome": 60}, {"dome": 1})),
    # the other modules
    "camera_objective": lambda: camera_objective(),
    "projection_iou_by_part": lambda: pb3d.camera_estimation.projection_iou_by_part(RGB, {"dome": DOME}, IMG, CAM),
    "grid_bounds": lambda: pb3d.camera_estimation.grid_bounds(RGB),
    "grid_hit_bits": lambda: pb3d.camera_estimation.grid_hit_bits(RGB, [DOME], CAM, 8, 8),
    "projection_overlays": lambda: pb3d.camera_estimation.projection_overlays(RGB, {"dome": DOME}, IMG, CAM, "part_on_whole"),
    "radius_neighbor_counts": lambda: pb3d.cluster.radius_neighbor_counts(PTS, 0.5),
    "cluster_points": lambda: pb3d.cluster.cluster_points(PTS, 0.5, 2),
    "select_points": lambda: pb3d.cluster.select_points(PTS, np.arange(10) % 2),
    "keep_largest_clusters": lambda: pb3d.cluster.keep_largest_clusters(PTS, 0.5, 2),
    "build_deformed_grid": lambda: pb3d.deformation_estimation.build_deformed_grid(RGB, {"dome": DOME}, {"dome": {"deform": (1, 1, 0, 0, 0)}}, (8, 8)),
    "project_sharded": lambda: pb3d.dist.project_colored_voxels_sharded(PTS32, np.tile(DOME, (10, 1)), 0, CAM["cam_pos"], CAM["target"], 20.0, 4.0,
                                                                        4.0, 8, 8, reduce=False),
    "distance_transform": lambda: pb3d.distance.distance_transform(OCC, return_indices=True),
    "distance_transform_resident_grid": OnGrid(OCC, lambda g: pb3d.distance.distance_transform(g)),
    "dilate_grid": lambda: pb3d.distance.dilate_grid(OCC, 1),
    "close_grid": lambda: pb3d.distance.close_grid(OCC, 1),
    "grid_surface_metrics": lambda: pb3d.distance.grid_surface_metrics(OCC, LAB),
    "voxel_downsample": lambda: pb3d.downsample.voxel_downsample(PTS, 0.25),
    "compute_global_depth_buffer": lambda: evi.compute_global_depth_buffer(RGB, CAM, 8, 8),
    "project_part_visible": lambda: evi.project_part_visible(PTS32, CAM, ZBUF, 8, 8),
    "grid_depth_buffer": lambda: evi.grid_depth_buffer(RGB, CAM, 8, 8),
    "grid_visible_bits": lambda: evi.grid_visible_bits(RGB, [DOME], CAM, ZBUF, 8, 8),
    "points_visible_bits": lambda: evi.points_visible_bits([PTS32, PTS32], CAM, ZBUF, 8, 8),
    "color_presence": lambda: evi.color_presence(LAB),
    "compute_binary_gt": lambda: evi.compute_binary_gt(IMG, RGB),
    "extract_minaret_voxels_by_label": lambda: pb3d.minarets.extract_minaret_voxels_by_label(RGB, MINARETS),
    "extract_minaret_masks_by_label": lambda: pb3d.minarets.extract_minaret_masks_by_label(IMG, MINARETS),
    "perspective_carve": lambda: pb3d.perspective.perspective_carve(RGB, [(IMG, CAM), (IMG[..., 0], CAM)], return_counts=True),
    "perspective_carve_resident_grid": OnGrid(LAB, lambda g: pb3d.perspective.perspective_carve(g, [(IMG, CAM)])),
    "perspective_paint": lambda: pb3d.perspective.perspective_paint(RGB, [(IMG, CAM), (IMG, CAM)], return_counts=True),
    "perspective_paint_host_zbuf": lambda: pb3d.perspective.perspective_paint(RGB, [(IMG, CAM)], zbufs=[ZBUF]),
    "render_mesh": lambda: pb3d.render.render_mesh(TET_V, TET_F, CAM["cam_pos"], CAM["target"], 20.0, 4.0, 4.0, 8, 8,
                                                   vertex_colors=np.arange(4, dtype=np.uint8), return_bary=True),
    "mesh_projection_iou": lambda: pb3d.render.mesh_projection_iou(TET_V, TET_F, np.tile(DOME, (4, 1)), IMG, {"dome": DOME}, CAM["cam_pos"],
                                                                   CAM["target"], 20.0, 4.0, 4.0),
    "kth_smallest": lambda: pb3d.selection.kth_smallest(PTS, 3),
    "mesh_vertex_adjacency": lambda: pb3d.smooth.mesh_vertex_adjacency(TET_F, 4, True, True),
    "smooth_mesh": lambda: pb3d.smooth.smooth_mesh(TET_V, TET_F, fixed=[1, 0, 0, 0]),
    "extract_top_k_components": lambda: pb3d.voxel_utils.extract_top_k_components(RGB, DOME, 1),
    "extract_top_k_components_resident": OnGrid(RGB, lambda g: pb3d.voxel_utils.extract_top_k_components(g, DOME, 1)),
    "voxelize_mesh": lambda: pb3d.voxelize.voxelize_mesh(TET_V, TET_F, (4, 4, 4), return_stats=True),
    "grid_overlap_counts": lambda: pb3d.voxelize.grid_overlap_counts(OCC, RGB),
    "mesh_grid_iou": lambda: pb3d.voxelize.mesh_grid_iou(TET_V, TET_F, OCC),
}


def leaked_while_failing(lib, call):
    """run a wrapper that must fail; (live blocks it made and left while its exception is still held, allocations it asked for)"""
    before, first = set(lib.live), lib.allocs
    try:
        call()
    except (ValueError, _lib.Pb3dError) as e:
        held = e                                                    # (with its traceback: nothing of the wrapper's frames is collected yet)
        left = set(lib.live) - before
        assert held is not None and before <= lib.live, "a buffer the wrapper was only handed is gone"
        return left, lib.allocs - first
    raise AssertionError("the wrapper succeeded against a library whose entries all fail")


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_wrapper_leaves_no_buffer_behind(stub, capsys, name):
    if isinstance(WRAPPERS[name], OnGrid):
        WRAPPERS[name].grid = None
        WRAPPERS[name]()                                            # the caller's grid goes up first
    left, n_allocs = leaked_while_failing(stub, WRAPPERS[name])
    assert n_allocs >= 1, "the wrapper allocated nothing: the stub does not drive it"
    assert not left, f"{name}: {len(left)} block(s) live after its entry failed"
    for k in range(1, n_allocs + 1):
        stub.fail_at = stub.allocs + k
        left, _ = leaked_while_failing(stub, WRAPPERS[name])
        assert not left, f"{name}: {len(left)} block(s) live after its allocation {k} of {n_allocs} failed"
    stub.fail_at = None


RESIDENT_WITH_OUT = {
    "nn_distances_resident": lambda d, out: ev.nn_distances_resident(d, 10, d, 10, out=out),
    "points_bounds_resident": lambda d, out: ev.points_bounds_resident(d, 10, out=out),
    "density_grid_resident": lambda d, out: ev.density_grid_resident(d, 10, 4, out=out),
    "vertex_normals_resident": lambda d, out: ev.vertex_normals_resident(d, 4, d, 4, out=out),
    "transform_points_resident": lambda d, out: ph.transform_points_resident(d, 10, np.eye(4), out=out),
    "icp_step_resident": lambda d, out: ph.icp_step_resident(d, 10, d, 10, np.eye(4), -1.0, (0, 0, 0), (0, 0, 0), out=out),
    "crop_to_box_resident": lambda d, out: ph.crop_to_box_resident(d, 10, (0, 0, 0), (1, 1, 1), out=out),
    "radius_neighbor_counts_resident": lambda d, out: pb3d.cluster.radius_neighbor_counts_resident(d, 10, 0.5, out=out),
    "select_points_resident": lambda d, out: pb3d.cluster.select_points_resident(d, 10, d, out=out, index=out),
    "smooth_mesh_resident": lambda d, out: pb3d.smooth.smooth_mesh_resident(d, 4, d, 4, out=out),
    "voxelize_mesh_resident": lambda d, out: pb3d.voxelize.voxelize_mesh_resident(d, 4, d, 4, (4, 4, 4), out=out),
    "depth_buffer_resident": lambda d, out: evi.depth_buffer_resident(d, (4, 4, 4, 3), CAM, 8, 8, out=out),
    "hit_bits_resident": lambda d, out: pb3d.camera_estimation.hit_bits_resident(d, (4, 4, 4, 3), [DOME], CAM, 8, 8, out=out),
    "render_shade_resident": lambda d, out: pb3d.render.render_shade_resident(d, d, 64, d, 4, 4, d, 3, out=out),
    "kth_smallest_resident": lambda d, out: pb3d.selection.kth_smallest_resident(d, 10, 3, out=out),
    "dilate_grid_resident": lambda d, out: pb3d.distance.dilate_grid_resident(dev.DeviceGrid(d, (4, 4, 4)), 1, out=None if out is None else dev.DeviceGrid(out, (4, 4, 4))),
}


@pytest.mark.parametrize("name", sorted(RESIDENT_WITH_OUT))
def test_a_callers_out_survives_a_failing_entry(stub, name):
    d_in, d_out = dev.DeviceBuffer(4096), dev.DeviceBuffer(4096)
    mine = {d_in.ptr, d_out.ptr}
    with pytest.raises((ValueError, _lib.Pb3dError)) as info:
        RESIDENT_WITH_OUT[name](d_in, d_out)
    assert info.value is not None and stub.live == mine            # `out` and the input are live, and nothing else is
    # and without `out` the result the form allocated itself is gone
    with pytest.raises((ValueError, _lib.Pb3dError)) as info:
        RESIDENT_WITH_OUT[name](d_in, None)
    assert info.value is not None and stub.live == mine
    d_in.free()
    d_out.free()
    assert not stub.live
