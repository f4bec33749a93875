"""pb3d_weld_vertices_resident and pb3d_mesh_orient_resident driven directly through ctypes on resident buffers whose base is an odd
number of elements past where pb3d_dev_alloc put it, in the arenas of tests/test_pointer_offsets.py: the payloads equal the
restatements byte for byte, the guard zones of every output still hold their fill, no input changed, and after a refused call (a bad
face index) nothing was written at all.

What the kernels need, per pointer argument, from reading them: csrc/weld.hip reads a float64 coordinate's two key words as one 64-bit
load (8-byte aligned, which an offset of whole elements keeps) and copies rows, indices and colour bytes element by element;
csrc/orient.hip and the front half of csrc/meshcomp.hip read and write face indices, flip bytes, patch numbers, counts and volumes by
element.  Neither has an address-keyed path."""
import ctypes as C

import numpy as np
import pytest

import meshcomp_restate as mc
import orient_restate as orr
import weld_restate as wr
from pb3d import orient_mesh, weld_vertices  # noqa: F401  (without the feature nothing in this file can run)
from test_pointer_offsets import OUT_FILL, Run, same

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("f64, i64", [(False, False), (True, True)])
def test_weld_at_odd_offsets(pb3d_gpu, f64, i64):
    V0, F0 = mc.fragments_mesh()
    V, F = wr.soup(V0.astype(np.float64) * np.pi if f64 else V0, F0)
    F = F.astype(np.int64 if i64 else np.int32)
    F[::7] -= len(V)                                                            # negative indices wrap
    cols = np.random.default_rng(3).integers(0, 256, (len(V), 3), dtype=np.uint8)
    ref = wr.restate(V, F, cols)
    nv, nf, m = len(V), len(F), len(ref["vertices"])
    ve, fe = V.dtype.itemsize, F.dtype.itemsize
    for k in (1, 3):
        r = Run(pb3d_gpu, ("weld", f64, i64, k))
        outs = [r.out(V.nbytes, k * ve), r.out(F.nbytes, k * fe), r.out(cols.nbytes, k), r.out(nv * 4, k * 4), r.out(nv * 4, k * 4), r.out(nv * 4, k * 4)]
        classes = C.c_int64(-1)
        r.ok(r.lib.pb3d_weld_vertices_resident(r.ctx, r.inp(V, k * ve), int(f64), nv, r.inp(F, k * fe), int(i64), nf, r.inp(cols, k), 3,
                                               *(o.ptr for o in outs), C.byref(classes)))
        assert classes.value == m
        rows = {0: [(0, m * 3 * ve)], 2: [(0, m * 3)], 3: [(0, m * 4)], 5: [(0, m * 4)]}      # the first m entries; inverse and faces whole
        got = r.finish(written=rows)
        same(got[0][:m * 3 * ve], ref["vertices"], "vertices")
        same(got[1], ref["faces"], "faces")
        same(got[2][:m * 3], ref["colors"], "colors")
        same(got[3][:m * 4], ref["index"], "index")
        same(got[4], ref["inverse"], "inverse")
        same(got[5][:m * 4], ref["counts"].astype(np.uint32), "counts")
    # a refused call writes nothing
    G = F.copy()
    G[nf // 2, 2] = nv
    r = Run(pb3d_gpu, "weld refusal")
    outs = [r.out(V.nbytes, ve), r.out(F.nbytes, fe), r.out(cols.nbytes, 1), r.out(nv * 4, 4), r.out(nv * 4, 4), r.out(nv * 4, 4)]
    classes = C.c_int64(-1)
    rc = r.lib.pb3d_weld_vertices_resident(r.ctx, r.inp(V, ve), int(f64), nv, r.inp(G, fe), int(i64), nf, r.inp(cols, 1), 3, *(o.ptr for o in outs),
                                           C.byref(classes))
    assert rc == -6 and classes.value == -1
    assert all((pay == OUT_FILL).all() for pay in r.finish())


@gpu
@pytest.mark.parametrize("f64, i64, sign", [(False, False, 0), (True, True, 1), (False, True, 2)])
def test_orient_at_odd_offsets(pb3d_gpu, f64, i64, sign):
    V, F0 = mc.fragments_mesh()
    V = V.astype(np.float64) * np.pi if f64 else V
    F = orr.preswapped(F0, 9)[0].astype(np.int64 if i64 else np.int32)
    F[::5] -= len(V)
    ref = orr.restate(F, len(V), V, (None, "positive", "negative")[sign])
    nv, nf, npatch = len(V), len(F), ref["totals"]["patches"]
    ve, fe = V.dtype.itemsize, F.dtype.itemsize
    names = orr.COUNTS + ("orientable", "inverted")
    counts = np.stack([ref["stats"][k].astype(np.int64) for k in names])
    for k in (1, 3):
        r = Run(pb3d_gpu, ("orient", f64, i64, sign, k))
        outs = [r.out(nf, k), r.out(nf * 4, k * 4), r.out(F.nbytes, k * fe), r.out(nf * 64, k * 8), r.out(nf * 8, k * 8)]
        totals = (C.c_int64 * 8)(*([-1] * 8))
        r.ok(r.lib.pb3d_mesh_orient_resident(r.ctx, r.inp(V, k * ve), int(f64), nv, r.inp(F, k * fe), int(i64), nf, sign, *(o.ptr for o in outs), totals))
        assert dict(zip(orr.TOTALS, totals)) == ref["totals"]
        got = r.finish(written={3: [(0, npatch * 64)], 4: [(0, npatch * 8)]})
        same(got[0], ref["flip"], "flip")
        same(got[1], ref["patch"], "patch")
        same(got[2], ref["faces"], "faces")
        same(got[3][:npatch * 64], counts, "counts")
        same(got[4][:npatch * 8], ref["stats"]["volume"], "volume")
    G = F.copy()
    G[nf // 2, 0] = -nv - 1
    r = Run(pb3d_gpu, "orient refusal")
    outs = [r.out(nf, 1), r.out(nf * 4, 4), r.out(F.nbytes, fe), r.out(nf * 64, 8), r.out(nf * 8, 8)]
    totals = (C.c_int64 * 8)(*([-1] * 8))
    rc = r.lib.pb3d_mesh_orient_resident(r.ctx, r.inp(V, ve), int(f64), nv, r.inp(G, fe), int(i64), nf, sign, *(o.ptr for o in outs), totals)
    assert rc == -6 and list(totals) == [-1] * 8
    assert all((pay == OUT_FILL).all() for pay in r.finish())
