"""A triangle mesh as a comparison target on the device (csrc/meshdist.hip): point_to_mesh_distances, sample_mesh_points and
cloud_to_mesh_metrics.  There is no upstream text to be exact against, so the chain of evidence is the one of tests/test_icp.py:
include/pb3d.h states the arithmetic; tests/meshdist_restate.py and tests/meshsample_restate.py restate it in NumPy and
tests/test_meshdist_restate.py holds the restatements against geometry on the CPU; here the device must return the restatements'
bytes -- distances, face indices and closest points array_equal with a brute force over ALL faces, samples and their faces array_equal
with the restated sampler.  Every case has at most 8 000 faces and 3 000 queries."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mesh_cases as mc  # noqa: E402
import meshdist_restate as mr  # noqa: E402
import meshsample_restate as ms  # noqa: E402

import pb3d  # noqa: E402
from pb3d import device as dev  # noqa: E402
from pb3d import eval_helpers as eh  # noqa: E402

pytestmark = pytest.mark.gpu

ENTRY_CAP = 8       # include/pb3d.h: the index holds at most 8 (cell, face) entries per face unless it is down to one cell


def check(Q, v, f):
    """the three outputs against the brute force; returns them"""
    want = mr.brute_force(Q, v, f)
    got = pb3d.point_to_mesh_distances(Q, v, f, return_faces=True, return_closest=True)
    assert got[0].dtype == np.float64 and got[1].dtype == np.int32 and got[2].dtype == np.float64
    assert got[0].shape == (len(Q),) and got[1].shape == (len(Q),) and got[2].shape == (len(Q), 3)
    for name, g, w in zip(("distance", "face", "closest point"), got, want):
        bad = np.flatnonzero(~(g == w).reshape(len(Q), -1).all(1))
        assert np.array_equal(g, w), f"{name}: {len(bad)} of {len(Q)} queries differ, first {bad[:5]}: got {g[bad[:3]]}, want {w[bad[:3]]}"
    return got


def grid_respects_cap(nf):
    cells, entries, halvings = eh.mesh_grid_shape()
    assert entries <= ENTRY_CAP * nf or cells == (1, 1, 1), (cells, entries, nf)
    assert entries >= nf
    return cells, entries, halvings


@pytest.mark.parametrize("name", ["mc_f32", "sphere_f64", "flat_f64"])
def test_real_meshes(name):
    """the fixture meshes (float32 / int32 and float64; the flat one gives a one-cell axis): own vertices at distance 0 -- where the
    faces round a vertex tie and the lowest must win --, jittered vertices, a cloud in 1.5 x the box, 64 points at 100 x the box"""
    v, f = mc.fixture_mesh(name)
    own, rest = mc.real_mesh_queries(v, 3)
    d, face, cp = check(own, v, f)
    assert not d.any() and np.array_equal(cp, own)
    check(rest, v, f)
    cells, entries, halvings = grid_respects_cap(len(f))
    print(name, "cells", cells, "entries", entries, "per face", entries / len(f), "halvings", halvings)
    assert (cells, entries) == mc.index_entries(v, f, halvings)
    if name == "flat_f64":
        assert cells[2] == 1
    check(rest[::4].astype(np.float32), v, f.astype(np.int64))


def test_integer_lattice_ties_go_to_the_lowest_face():
    v, f, q = mc.lattice_mesh()
    assert len(f) == 2112 and len(q) == 2023
    d, face, cp = check(q, v, f)
    # the ties are real: for most queries a second face is exactly as near as the winner
    a, b, c = mr.corners(v, f)
    sub = slice(0, len(q), 7)
    d2 = mr.closest(tuple(q[sub, k][:, None] for k in range(3)), *(tuple(x[None, :] for x in t) for t in (a, b, c)))[0]
    tied = ((d2 == d2.min(1)[:, None]).sum(1) > 1).mean()
    print("share of queries with a tie for the nearest face:", tied)
    assert tied > 0.9
    perm = np.random.default_rng(0).permutation(len(f))     # another face order, another winner: still the lowest index
    check(q[::3], v, f[perm])


def test_giant_needles_and_degenerate_faces_coarsen_the_grid():
    v, f, q = mc.giant_and_needles()
    check(q, v, f)
    cells, entries, halvings = grid_respects_cap(len(f))
    print("cells", cells, "entries", entries, "faces", len(f), "halvings", halvings)
    assert halvings == 2 and (cells, entries) == mc.index_entries(v, f, 2)      # tests/test_meshdist_restate.py: 0 and 1 halvings overflow
    small = f[1:2001]                                       # without the giant and the needles nothing needs coarsening
    check(q[:300], v, small)
    assert grid_respects_cap(len(small))[2] == 0


def test_launch_seams_and_unaligned_queries():
    """a single face; nq = 1, 255, 256, 257; query lists that start 4 bytes (float32) or 8 bytes (float64) into an allocation"""
    rng = np.random.default_rng(6)
    v = np.array([[0.0, 0.0, 0.0], [2.0, 0.5, 0.0], [0.5, 3.0, 1.0]])
    one = np.array([[0, 1, 2]])
    vm, fm = mc.random_mesh(300, 1)
    for nq in (1, 255, 256, 257):
        q = rng.uniform(-2, 4, (nq, 3))
        check(q, v, one)
        assert eh.mesh_grid_shape()[:2] == ((1, 1, 1), 1)
        check(q, vm, fm)
    lib, L = pb3d._lib.load(), pb3d._lib
    d_v, d_f = dev.from_numpy(vm), dev.from_numpy(fm)
    bufs = [d_v, d_f]
    try:
        for dtype, off in ((np.float32, 4), (np.float64, 8)):
            q = rng.uniform(-4, 6, (257, 3)).astype(dtype)
            want = mr.brute_force(q, vm, fm)
            d_q = dev.DeviceBuffer(q.nbytes + 64)
            d_q.upload(q, byte_offset=off)
            outs = [dev.DeviceBuffer(257 * 8 + 64), dev.DeviceBuffer(257 * 4 + 64), dev.DeviceBuffer(257 * 24 + 64)]
            bufs += [d_q] + outs
            L.check(lib.pb3d_mesh_dist_resident(L.ctx(), d_q.at(off), int(dtype == np.float64), 257, C.c_void_p(d_v.ptr), 1, len(vm),
                                                C.c_void_p(d_f.ptr), 1, len(fm), outs[0].at(8), outs[1].at(4), outs[2].at(8)))
            assert np.array_equal(outs[0].download((257,), np.float64, byte_offset=8), want[0])
            assert np.array_equal(outs[1].download((257,), np.int32, byte_offset=4), want[1])
            assert np.array_equal(outs[2].download((257, 3), np.float64, byte_offset=8), want[2])
    finally:
        for b in bufs:
            b.free()


def test_face_and_vertex_forms():
    """the four (query, vertex) dtype pairs; int32 and int64 faces; negative indices; optional outputs; the resident form; an index of
    nv is an IndexError and the device stays usable"""
    rng = np.random.default_rng(8)
    v, f = mc.random_mesh(500, 2)
    q = rng.uniform(-4, 6, (700, 3))
    for qt in (np.float32, np.float64):
        for vt in (np.float32, np.float64):
            check(q.astype(qt), v.astype(vt), f)
    neg = f.copy()
    neg[::2] -= len(v)
    want = mr.brute_force(q, v, f)
    got = check(q, v, neg)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    check(q, v, f.astype(np.uint16))
    assert np.array_equal(pb3d.point_to_mesh_distances(q, v, f), want[0])                         # d_face and d_closest NULL
    d, cp = pb3d.point_to_mesh_distances(q, v, f, return_closest=True)
    assert np.array_equal(d, want[0]) and np.array_equal(cp, want[2])
    d, face = pb3d.point_to_mesh_distances(q, v, f, return_faces=True)
    assert np.array_equal(d, want[0]) and np.array_equal(face, want[1])
    # resident, float32 vertices and int32 faces as pb3d.device.meshify hands them out
    v32, f32, q32 = v.astype(np.float32), neg.astype(np.int32), q.astype(np.float32)
    want32 = mr.brute_force(q32, v32, f32)
    bufs = [dev.from_numpy(q32), dev.from_numpy(v32), dev.from_numpy(f32)]
    try:
        for _ in range(2):                                  # the second call finds every scratch slot large enough: no wait for a regrow
            before = dev.sync_count()
            outs = eh.point_to_mesh_distances_resident(bufs[0], len(q), bufs[1], len(v), bufs[2], len(f), False, False, False, True, True)
            waits = dev.sync_count() - before
            bufs += list(outs)
        assert np.array_equal(outs[0].download((len(q),), np.float64), want32[0])
        assert np.array_equal(outs[1].download((len(q),), np.int32), want32[1])
        assert np.array_equal(outs[2].download((len(q), 3), np.float64), want32[2])
        halvings = eh.mesh_grid_shape()[2]
        print("host waits of the resident call:", waits, "halvings", halvings)
        assert waits == 3 + halvings                        # the index check, the box, 1 + halvings entry counts (include/pb3d.h)
    finally:
        for b in bufs:
            b.free()
    for bad in (len(v), -len(v) - 1, 2 ** 40):
        g = f.copy()
        g[len(g) // 2, 1] = bad
        with pytest.raises(IndexError):
            pb3d.point_to_mesh_distances(q, v, g)
        with pytest.raises(IndexError):
            pb3d.sample_mesh_points(v, g, 10)
        assert np.array_equal(pb3d.point_to_mesh_distances(q[:50], v, f), want[0][:50])            # a following call succeeds


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------
def check_samples(v, f, n, seed):
    want_p, want_f, _ = ms.sample(v, f, n, seed)
    pts, face = pb3d.sample_mesh_points(v, f, n, seed=seed, return_faces=True)
    assert pts.dtype == np.float64 and face.dtype == np.int32 and pts.shape == (n, 3) and face.shape == (n,)
    assert np.array_equal(face, want_f), (n, seed, np.flatnonzero(face != want_f)[:5])
    assert np.array_equal(pts, want_p), (n, seed)
    assert np.array_equal(pb3d.sample_mesh_points(v, f, n, seed=seed), want_p)


@pytest.mark.parametrize("nf", [1, 1024, 1025, 2049])
def test_sampler_equals_restatement_across_prefix_blocks(nf):
    """nf at and across the 1024-face seams of the cumulative sum; zero-area faces at the start, the end and inside; n = 0, 1, 257,
    20 000; two seeds; float32 and float64 vertices"""
    zero = () if nf == 1 else (0, nf // 2, nf // 2 + 1, nf - 1)
    for dtype in (np.float32, np.float64):
        v, f = mc.random_mesh(nf, 20 + nf, dtype, zero)
        for n in (1, 257, 20000):
            for seed in (0, 0x9E3779B97F4A7C15):
                check_samples(v, f, n, seed)
        pts, face = pb3d.sample_mesh_points(v, f, 0, return_faces=True)
        assert pts.shape == (0, 3) and face.shape == (0,)
    if zero:
        A = ms.face_areas(v, f)
        assert not A[list(zero)].any()
        assert A[pb3d.sample_mesh_points(v, f, 20000, return_faces=True)[1]].all()


def test_sampler_on_the_marching_cubes_mesh_and_resident_form():
    v, f = mc.fixture_mesh("mc_f32")
    check_samples(v, f, 20000, 5)
    want_p, want_f, _ = ms.sample(v, f, 3001, 9)
    bufs = [dev.from_numpy(v), dev.from_numpy(f)]           # float32 vertices, int32 faces
    try:
        for _ in range(2):                                  # the second call finds every scratch slot large enough
            before = dev.sync_count()
            d_p, d_f = eh.sample_mesh_points_resident(bufs[0], len(v), bufs[1], len(f), 3001, 9, False, False)
            waits = dev.sync_count() - before
            bufs += [d_p, d_f]
        assert np.array_equal(d_p.download((3001, 3), np.float64), want_p) and np.array_equal(d_f.download((3001,), np.int32), want_f)
        assert waits == 2                                   # the index check and the total (include/pb3d.h)
        d_p2, none = eh.sample_mesh_points_resident(bufs[0], len(v), bufs[1], len(f), 3001, 9, False, False, return_faces=False)
        bufs.append(d_p2)
        assert none is None and np.array_equal(d_p2.download((3001, 3), np.float64), want_p)
    finally:
        for b in bufs:
            b.free()


def test_sampler_refuses_a_mesh_without_area():
    v, f = mc.random_mesh(40, 3)
    f[:, 2] = f[:, 1]
    with pytest.raises(ValueError, match="total area"):
        pb3d.sample_mesh_points(v, f, 100)
    v, f = mc.random_mesh(40, 3)
    assert pb3d.sample_mesh_points(v, f, 100).shape == (100, 3)         # the context is usable afterwards


# ---- the metric ------------------------------------------------------------------------------------------------------------------------
def test_cloud_to_mesh_metrics_is_the_composition_of_its_parts():
    v, f = mc.fixture_mesh("sphere_f64")
    rng = np.random.default_rng(12)
    P = v[rng.choice(len(v), 1500)] * rng.uniform(0.9, 1.1, (1500, 1))
    tau = 0.4
    for n_samples, seed in ((None, 0), (2000, 3)):
        got = pb3d.cloud_to_mesh_metrics(P, v, f, tau, n_samples=n_samples, seed=seed)
        d_P = mr.brute_force(P, v, f)[0]
        S = ms.sample(v, f, len(P) if n_samples is None else n_samples, seed)[0]
        d_S = pb3d.nn_distances(S, P)
        p, r = float(np.mean(d_P < tau)), float(np.mean(d_S < tau))
        want = {"accuracy": float(np.mean(d_P)), "completeness": float(np.mean(d_S)), "precision": p, "recall": r,
                "f1": 0.0 if p + r == 0 else 2 * p * r / (p + r)}
        print(got)
        assert got == want and tuple(got) == tuple(want)
        assert 0 < p < 1 and 0 < r < 1
    far = pb3d.cloud_to_mesh_metrics(P + 100.0, v, f, tau)
    assert far["precision"] == 0.0 and far["recall"] == 0.0 and far["f1"] == 0.0
