"""mesh_vertex_adjacency and smooth_mesh (pb3d/smooth.py, csrc/smooth.hip) against the NumPy restatement of tests/smooth_restate.py, and
that restatement against a plain Python loop.  Every comparison of device output is np.array_equal, on bytes for float arrays:
include/pb3d.h states the result to the bit, so there is no tolerance anywhere."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import smooth_restate as sr

import pb3d
import pb3d.smooth  # noqa: F401  (without the feature every test of this file fails here)

gpu = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sr.constructed_cases()
FIXTURES = ("mc_f32", "sphere_f64", "height_f32", "height_f64", "flat_f64")
SMOOTHED = ("mc_f32", "sphere_f64", "height_f64")       # the three the two properties are measured on
DTYPES = (np.float64, np.float32)
WIDTHS = (np.int64, np.int32)
# what a smoothing is run with: Laplacian, Taubin, Taubin with the boundary fixed, Taubin with a random fixed mask
MODES = {"laplacian": dict(iterations=3, method="laplacian", lamb=0.6), "taubin": dict(iterations=2),
         "fix_boundary": dict(iterations=2, fix_boundary=True), "fixed": dict(iterations=2, lamb=0.4, mu=-0.45)}


@functools.lru_cache(maxsize=None)
def fixture(name):
    with np.load(os.path.join(GOLD, f"surface_{name}.npz")) as z:
        v, f = np.ascontiguousarray(z["vertices"]), np.ascontiguousarray(z["faces"])
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def mesh(name):
    return fixture(name[8:]) if name.startswith("fixture/") else CASES[name]


def fixed_mask(nv):
    return np.random.default_rng(nv).random(nv) < 0.3


def mode_args(mode, nv):
    kw = dict(MODES[mode])
    if mode == "fixed":
        kw["fixed"] = fixed_mask(nv)
    return kw


@functools.lru_cache(maxsize=None)
def want_adjacency(name):
    v, f = mesh(name)
    got = sr.adjacency(f, len(v))
    for a in got:
        a.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def want_smooth(name, f32, mode, iterations=None):
    """the restatement of one smoothing, computed once and shared"""
    v, f = mesh(name)
    kw = mode_args(mode, len(v))
    if iterations is not None:
        kw["iterations"] = iterations
    out = sr.restate(v.astype(np.float32 if f32 else np.float64), f, **kw)
    out.setflags(write=False)
    return out


def same_bytes(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    if not np.array_equal(got.view(np.uint8), ref.view(np.uint8)):
        bad = np.flatnonzero((got.view(np.uint8) != ref.view(np.uint8)).reshape(len(got), -1).any(axis=1))
        raise AssertionError((what, "first differing row", int(bad[0]), "rows differing", len(bad), "of", len(got)))


# =====================================================================================================================
# CPU: the restatement against the loop, its invariants, the pinned figures, the two properties; exports; validation
# =====================================================================================================================

@pytest.mark.parametrize("name", list(CASES))
def test_restatement_is_the_loop(name):
    v, f = CASES[name]
    nv = len(v)
    ref = sr.loop_adjacency(f, nv)
    for g, w in zip(want_adjacency(name), ref):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    big = nv > 5000
    for mode in MODES:
        if big and mode != "taubin":
            continue
        for dt in DTYPES:
            kw = mode_args(mode, nv)
            if big:
                kw["iterations"] = 1
            same_bytes(sr.restate(v.astype(dt), f, **kw), sr.loop(v.astype(dt), f, **kw), (name, mode, dt.__name__))


@pytest.mark.parametrize("name", list(CASES) + [f"fixture/{n}" for n in FIXTURES])
def test_adjacency_invariants(name):
    v, f = mesh(name)
    nv = len(v)
    starts, nbr, mult, boundary = want_adjacency(name)
    total = len(nbr)
    assert starts.shape == (nv + 1,) and starts[0] == 0 and starts[-1] == total and (np.diff(starts) >= 0).all()
    assert total % 2 == 0 and mult.shape == (total,) and boundary.shape == (nv,)
    src = sr.sources(starts)
    assert (src != nbr).all()
    key = src * max(nv, 1) + nbr
    assert (np.diff(key) > 0).all()                                     # every list strictly ascending, the lists in vertex order
    back = np.searchsorted(key, nbr.astype(np.int64) * max(nv, 1) + src)
    assert (back < total).all() and np.array_equal(key[back], nbr.astype(np.int64) * max(nv, 1) + src)      # j in N(i) <=> i in N(j)
    assert np.array_equal(mult[back], mult)                             # ... with the same multiplicity
    assert int(mult.sum()) == len(sr.pairs(f, nv)[0])


def test_pinned_figures_of_the_fixtures():
    for name, nb, deg in (("mc_f32", 0, 8), ("sphere_f64", 0, 6), ("height_f32", 220, 6), ("height_f64", 220, 6), ("flat_f64", 196, 6)):
        starts, nbr, mult, boundary = want_adjacency(f"fixture/{name}")
        assert int(boundary.sum()) == nb and int(np.diff(starts).max()) == deg, name
    assert int(np.diff(want_adjacency("fan/hub_first")[0]).max()) == 4097 and int(np.diff(want_adjacency("fan/hub_last")[0])[-1]) == 4097
    assert want_adjacency("awkward/duplicated")[2].tolist() == [2, 2, 2, 4, 2, 2, 4, 2, 2, 2] and not want_adjacency("awkward/duplicated")[3].any()
    assert want_adjacency("small/two_triangles")[2].tolist() == [1, 1, 1, 2, 1, 1, 2, 1, 1, 1] and want_adjacency("small/two_triangles")[3].all()
    assert len(want_adjacency("awkward/all_degenerate")[1]) == 0
    assert [6 * len(CASES[n][1]) for n in CASES if n.startswith("seam/")] == [2040, 2046, 2052, 2058, 4086, 4092, 4098, 4104]


@pytest.mark.parametrize("name", SMOOTHED)
def test_taubin_flattens_the_staircase_and_keeps_the_size(name):
    v, f = fixture(name)
    taubin = sr.restate(v, f, 10)
    laplacian = sr.restate(v, f, 20, method="laplacian", lamb=0.5)
    before, after = sr.mean_dihedral_deg(v, f), sr.mean_dihedral_deg(taubin, f)
    e0, et, el = sr.extent(v), sr.extent(taubin), sr.extent(laplacian)
    print(name, "mean dihedral", before, "->", after, "extent", e0, "taubin", et, "laplacian", el)
    assert after < before
    assert abs(et - e0) < abs(el - e0)


def test_exports():
    for n in ("mesh_vertex_adjacency", "mesh_vertex_adjacency_resident", "smooth_mesh", "smooth_mesh_resident"):
        assert callable(getattr(pb3d, n)) and n in pb3d.smooth.__all__
    for n in ("pb3d_mesh_adjacency_resident", "pb3d_mesh_smooth_resident"):
        assert n in pb3d._lib.EXPORTED_SYMBOLS


def test_validation_needs_no_device():
    v, f = CASES["small/tetrahedron"]
    for bad in ("cotangent", "", None, 0):
        with pytest.raises(ValueError, match="method must be 'taubin' or 'laplacian'"):
            pb3d.smooth_mesh(v, f, method=bad)
        with pytest.raises(ValueError, match="method must be 'taubin' or 'laplacian'"):
            pb3d.smooth_mesh_resident(None, 4, None, 4, method=bad)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="lamb must be finite"):
            pb3d.smooth_mesh(v, f, lamb=bad)
        with pytest.raises(ValueError, match="mu must be finite"):
            pb3d.smooth_mesh(v, f, mu=bad)
        with pytest.raises(ValueError, match="lamb must be finite"):
            pb3d.smooth_mesh_resident(None, 4, None, 4, lamb=bad)
    for bad in (-1, 1.5, True, None, "3"):
        with pytest.raises(ValueError, match="iterations must be an integer"):
            pb3d.smooth_mesh(v, f, iterations=bad)
        with pytest.raises(ValueError, match="iterations must be an integer"):
            pb3d.smooth_mesh_resident(None, 4, None, 4, iterations=bad)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        pb3d.smooth_mesh(np.zeros((4, 2)), f)
    with pytest.raises(ValueError, match=r"\(m, 3\)"):
        pb3d.smooth_mesh(v, np.zeros((4, 4), np.int64))
    with pytest.raises(ValueError, match=r"\(m, 3\)"):
        pb3d.mesh_vertex_adjacency(np.zeros(6, np.int64), 4)
    for fn in (lambda: pb3d.smooth_mesh(v, f.astype(np.float64)), lambda: pb3d.mesh_vertex_adjacency(f.astype(np.float32), 4)):
        with pytest.raises(IndexError, match="integer"):
            fn()
    for fn in (lambda: pb3d.smooth_mesh(v, np.array([[0, 1, 4]], np.uint32)), lambda: pb3d.mesh_vertex_adjacency(np.array([[0, 1, 4]], np.uint8), 4)):
        with pytest.raises(IndexError, match="out of bounds"):
            fn()
    for bad in (np.zeros(3, bool), np.zeros((4, 1), bool), np.zeros(4)):
        with pytest.raises(ValueError, match="fixed must be a mask of 4 entries"):
            pb3d.smooth_mesh(v, f, fixed=bad)
    for fn in (lambda: pb3d.mesh_vertex_adjacency(f, 2 ** 31), lambda: pb3d.mesh_vertex_adjacency(f, -1),
               lambda: pb3d.smooth_mesh_resident(None, 2 ** 31, None, 0), lambda: pb3d.mesh_vertex_adjacency_resident(None, 2 ** 31, 0)):
        with pytest.raises(ValueError, match="at most 2\\^31 - 1 vertices"):
            fn()
    huge = np.broadcast_to(np.zeros((1, 3), np.int32), ((2 ** 31 - 1) // 6 + 1, 3))        # a view: no memory behind it
    for fn in (lambda: pb3d.mesh_vertex_adjacency(huge, 4), lambda: pb3d.smooth_mesh_resident(None, 4, None, len(huge)),
               lambda: pb3d.mesh_vertex_adjacency_resident(None, 4, len(huge))):
        with pytest.raises(ValueError, match="at most \\(2\\^31 - 1\\) / 6 faces"):
            fn()
    for dt in DTYPES:                                                   # the empty mesh needs no device either
        out = pb3d.smooth_mesh(np.zeros((0, 3), dt), np.zeros((0, 3), np.int64))
        assert out.shape == (0, 3) and out.dtype == dt
    assert pb3d.smooth_mesh(np.zeros((0, 3), np.int16), np.zeros((0, 3), np.int32)).dtype == np.float64
    with pytest.raises(IndexError):
        pb3d.smooth_mesh(np.zeros((0, 3)), np.zeros((1, 3), np.int64))


def test_cabi_refusals_need_no_device():
    lib = pb3d._lib.load()
    one = C.c_void_p(256)
    total = C.c_int64(7)
    nan = float("nan")
    adj, smooth = lib.pb3d_mesh_adjacency_resident, lib.pb3d_mesh_smooth_resident

    def refused(rc, text):
        assert rc == -1 and text in lib.pb3d_last_error().decode(), (rc, lib.pb3d_last_error())

    refused(adj(None, one, 0, -1, 4, one, one, None, None, C.byref(total)), "negative count")
    refused(adj(None, one, 0, 4, -1, one, one, None, None, C.byref(total)), "negative count")
    refused(adj(None, one, 0, 2 ** 31, 4, one, one, None, None, C.byref(total)), "at most 2^31 - 1 vertices")
    refused(adj(None, one, 1, 4, (2 ** 31 - 1) // 6 + 1, one, one, None, None, C.byref(total)), "2^31 - 1 directed pairs")
    refused(adj(None, None, 0, 4, 4, one, one, None, None, C.byref(total)), "null buffer")
    refused(adj(None, one, 0, 4, 4, one, one, None, None, None), "null argument")
    refused(adj(None, one, 0, 4, 4, None, one, None, None, C.byref(total)), "null buffer")
    refused(adj(None, one, 0, 4, 4, one, None, None, None, C.byref(total)), "null buffer")
    refused(adj(None, one, 0, 4, 4, one, one, None, None, C.byref(total)), "null context")          # mult and boundary may be NULL
    refused(adj(None, None, 0, 4, 0, one, None, None, None, C.byref(total)), "null context")        # nf = 0 needs no faces
    assert total.value == 7                                             # a refusal writes nothing

    def sm(nv=4, nf=4, iterations=3, lam=0.5, mu=-0.53, verts=one, faces=one, out=C.c_void_p(512)):
        return smooth(None, verts, 1, nv, faces, 0, nf, iterations, lam, mu, None, 0, out)

    refused(sm(nv=-1), "negative count")
    refused(sm(nf=-1), "negative count")
    refused(sm(nv=2 ** 31), "at most 2^31 - 1 vertices")
    refused(sm(nf=(2 ** 31 - 1) // 6 + 1), "2^31 - 1 directed pairs")
    refused(sm(iterations=-1), "iterations must be >= 0")
    for bad in (nan, float("inf"), float("-inf")):
        refused(sm(lam=bad), "lambda must be finite")
    for bad in (float("inf"), float("-inf")):
        refused(sm(mu=bad), "mu must be finite, or NaN")
    refused(sm(faces=None), "null buffer")
    refused(sm(verts=None), "null buffer")
    refused(sm(out=None), "null buffer")
    refused(sm(out=one), "may not alias")
    refused(sm(mu=nan), "null context")                                 # NaN: Laplacian
    refused(sm(), "null context")
    refused(sm(nv=0, nf=0, verts=None, faces=None, out=None), "null context")


# =====================================================================================================================
# GPU: the device against the restatement
# =====================================================================================================================

def check_adjacency(pb3d, name, widths=WIDTHS):
    v, f = mesh(name)
    ref = want_adjacency(name)
    for w in widths:
        got = pb3d.mesh_vertex_adjacency(f.astype(w), len(v), return_multiplicity=True, return_boundary=True)
        for g, r, part in zip(got, ref, ("starts", "neighbours", "multiplicity", "boundary")):
            assert g.dtype == r.dtype and g.shape == r.shape and np.array_equal(g, r), (name, w.__name__, part)
        plain = pb3d.mesh_vertex_adjacency(f.astype(w), len(v))
        assert len(plain) == 2 and np.array_equal(plain[0], ref[0]) and np.array_equal(plain[1], ref[1]), (name, w.__name__)


def check_smooth(pb3d, name, combos=None, modes=tuple(MODES), iterations=None):
    v, f = mesh(name)
    for dt, w in combos or [(d, w) for d in DTYPES for w in WIDTHS]:
        for mode in modes:
            kw = mode_args(mode, len(v))
            if iterations is not None:
                kw["iterations"] = iterations
            got = pb3d.smooth_mesh(v.astype(dt), f.astype(w), **kw)
            same_bytes(got, want_smooth(name, dt == np.float32, mode, iterations), (name, dt.__name__, w.__name__, mode))


def check(pb3d, name, cheap=True):
    check_adjacency(pb3d, name, WIDTHS if cheap else (np.int32,))
    check_smooth(pb3d, name, None if cheap else [(np.float64, np.int64), (np.float32, np.int32)])


@gpu
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("small/")])
def test_smallest_meshes(pb3d_gpu, name):
    check(pb3d_gpu, name)


@gpu
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("fan/")])
def test_hub_fans(pb3d_gpu, name):
    """a vertex in every face: degree 4097 is past the lane cutoff and past one 64-gather, 24 576 pairs are 12 sort tiles; the small
    fans put the hub on either side of the cutoff (32) and of one and two gathers"""
    check(pb3d_gpu, name, cheap=not name.startswith("fan/hub"))


@gpu
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("seam/")])
def test_sort_seams(pb3d_gpu, name):
    check_adjacency(pb3d_gpu, name)
    check_smooth(pb3d_gpu, name, [(np.float64, np.int32), (np.float32, np.int64)], modes=("taubin", "fix_boundary"))


@gpu
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("radix/")])
def test_radix_passes(pb3d_gpu, name):
    check(pb3d_gpu, name, cheap=len(CASES[name][0]) < 5000)


@gpu
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("awkward/")])
def test_awkward_faces(pb3d_gpu, name):
    check(pb3d_gpu, name)


@gpu
def test_face_index_out_of_range_raises_and_device_stays_usable(pb3d_gpu):
    v, f = CASES["small/tetrahedron"]
    for bad in (4, -5):
        for w in WIDTHS:
            g = f.astype(w).copy()
            g[2, 1] = bad
            with pytest.raises(IndexError, match="out of bounds"):
                pb3d_gpu.mesh_vertex_adjacency(g, 4)
            for dt in DTYPES:
                with pytest.raises(IndexError, match="out of bounds"):
                    pb3d_gpu.smooth_mesh(v.astype(dt), g)
                with pytest.raises(IndexError, match="out of bounds"):
                    pb3d_gpu.smooth_mesh(v.astype(dt), g, iterations=0)
    check(pb3d_gpu, "small/tetrahedron")


@gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures(pb3d_gpu, name):
    key = f"fixture/{name}"
    v, f = mesh(key)
    check_adjacency(pb3d_gpu, key)
    for iterations in (1, 10):
        check_smooth(pb3d_gpu, key, [(v.dtype.type, np.int32), (v.dtype.type, np.int64)], iterations=iterations)


@gpu
@pytest.mark.parametrize("name", ("fixture/mc_f32", "fixture/height_f64"))
def test_identity_cases(pb3d_gpu, name):
    v, f = mesh(name)
    assert np.isfinite(v).all() and not (np.signbit(v) & (v == 0)).any()      # x + 0.0 * d is x for every such x and finite d
    for kw in (dict(iterations=0), dict(iterations=0, method="laplacian"), dict(method="laplacian", lamb=0.0),
               dict(lamb=0.0, mu=0.0), dict(fixed=np.ones(len(v), bool)), dict(fixed=np.ones(len(v), np.uint8), fix_boundary=True)):
        got = pb3d_gpu.smooth_mesh(v, f, **kw)
        assert got.dtype == v.dtype and got.tobytes() == v.tobytes(), (name, sorted(kw))
        same_bytes(got, sr.restate(v, f, **kw), (name, sorted(kw)))


@gpu
def test_non_finite_input_spreads_as_the_arithmetic_spreads_it(pb3d_gpu):
    v64, f = CASES["radix/200"]
    for dt in DTYPES:
        for bad in (np.nan, np.inf):
            v = v64.astype(dt)
            v[57, 1] = bad
            for mode in ("taubin", "laplacian"):
                kw = mode_args(mode, len(v))
                ref = sr.restate(v, f, **kw)
                assert np.isnan(ref).sum() > 3 and np.isfinite(ref).sum() > 3
                same_bytes(pb3d_gpu.smooth_mesh(v, f, **kw), ref, ("non-finite", dt.__name__, bad, mode))


@gpu
def test_determinism(pb3d_gpu):
    for name in ("fan/hub_first", "fixture/mc_f32"):
        v, f = mesh(name)
        once = pb3d_gpu.smooth_mesh(v, f, fix_boundary=True).tobytes()
        assert pb3d_gpu.smooth_mesh(v, f, fix_boundary=True).tobytes() == once
        adj = [a.tobytes() for a in pb3d_gpu.mesh_vertex_adjacency(f, len(v), True, True)]
        assert [a.tobytes() for a in pb3d_gpu.mesh_vertex_adjacency(f, len(v), True, True)] == adj


# ---- buffers that do not start where the allocator put them -----------------------------------------------------------------------------
GUARD = 256
IN_FILL, OUT_FILL = 0xFF, 0xA5


class Arena:
    """a payload at GUARD + off bytes inside a 256-byte aligned allocation, guard bytes on both sides"""

    def __init__(self, pb3d, nbytes, off, fill, payload=None):
        self.off, self.n, self.fill = int(off), int(nbytes), fill
        total = GUARD + self.off + self.n + GUARD
        total += -total % 256
        self.buf = pb3d.device.DeviceBuffer(total)
        assert self.buf.ptr % 256 == 0
        self.host = np.full(total, fill, np.uint8)
        if payload is not None:
            self.host[GUARD + self.off:GUARD + self.off + self.n] = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        self.buf.upload(self.host)
        self.ptr = self.buf.at(GUARD + self.off)

    def payload(self, dtype=np.uint8):
        """the payload, after checking that both guards still hold the fill"""
        got = self.buf.download((self.buf.nbytes,))
        lo, hi = GUARD + self.off, GUARD + self.off + self.n
        assert (got[:lo] == self.fill).all() and (got[hi:] == self.fill).all(), "a guard zone was written"
        return got[lo:hi].copy().view(dtype)


@gpu
def test_pointer_offsets(pb3d_gpu):
    """faces and float32 vertices one and three elements (4 and 12 bytes) into their buffers, float64 vertices and int64 faces 8 and 24
    bytes, every output likewise (the boundary and fixed bytes at 1 and 3); entries past `total` stay untouched and no input changes"""
    L = pb3d_gpu._lib
    lib, ctx = L.load(), L.ctx()
    name = "seam/2052"
    v64, f64 = CASES[name]
    nv, nf = len(v64), len(f64)
    starts, nbr, mult, boundary = want_adjacency(name)
    total = len(nbr)
    fixed = fixed_mask(nv).view(np.uint8)
    for elems in (1, 3, 0):
        for w in WIDTHS:
            arenas = []

            def arena(nbytes, off, fill, payload=None):
                arenas.append(Arena(pb3d_gpu, nbytes, off, fill, payload))
                return arenas[-1]

            try:
                faces = np.ascontiguousarray(f64.astype(w))
                fs = faces.dtype.itemsize
                a_f = arena(faces.nbytes, elems * fs, IN_FILL, faces)
                a_st, a_nb = arena((nv + 1) * 8, elems * 8, OUT_FILL), arena(6 * nf * 4, elems * 4, OUT_FILL)
                a_mu, a_bd = arena(6 * nf * 4, elems * 4, OUT_FILL), arena(nv, elems, OUT_FILL)
                got_total = C.c_int64(-1)
                L.check(lib.pb3d_mesh_adjacency_resident(ctx, a_f.ptr, int(fs == 8), nv, nf, a_st.ptr, a_nb.ptr, a_mu.ptr, a_bd.ptr, C.byref(got_total)))
                what = (name, "adjacency", elems, w.__name__)
                assert got_total.value == total, what
                assert np.array_equal(a_st.payload(np.int64), starts), what
                assert np.array_equal(a_nb.payload(np.int32)[:total], nbr) and (a_nb.payload()[4 * total:] == OUT_FILL).all(), what
                assert np.array_equal(a_mu.payload(np.uint32)[:total], mult) and (a_mu.payload()[4 * total:] == OUT_FILL).all(), what
                assert np.array_equal(a_bd.payload().astype(bool), boundary), what
                a_fx = arena(nv, elems, IN_FILL, fixed)
                for dt in DTYPES:
                    verts = np.ascontiguousarray(v64.astype(dt))
                    vs = verts.dtype.itemsize
                    a_v, a_out = arena(verts.nbytes, elems * vs, IN_FILL, verts), arena(verts.nbytes, elems * vs, OUT_FILL)
                    kw = mode_args("fixed", nv)
                    L.check(lib.pb3d_mesh_smooth_resident(ctx, a_v.ptr, int(vs == 8), nv, a_f.ptr, int(fs == 8), nf, kw["iterations"], kw["lamb"],
                                                          kw["mu"], a_fx.ptr, 1, a_out.ptr))
                    ref = sr.restate(verts, faces, fix_boundary=True, **kw)
                    same_bytes(a_out.payload(dt).reshape(nv, 3), ref, (name, "smooth", elems, w.__name__, dt.__name__))
                    assert a_v.payload(dt).tobytes() == verts.tobytes()
                assert a_f.payload(w).tobytes() == faces.tobytes() and a_fx.payload().tobytes() == fixed.tobytes()
            finally:
                for a in arenas:
                    a.buf.free()


@gpu
def test_host_waits(pb3d_gpu):
    """once the scratch is warm the adjacency entry waits twice (the index check and total), a smoothing once (the index check)"""
    L = pb3d_gpu._lib
    lib, ctx = L.load(), L.ctx()
    dev = pb3d_gpu.device
    v, f = CASES["radix/70000"]
    nv, nf = len(v), len(f)
    bufs = [dev.from_numpy(v), dev.from_numpy(f), dev.DeviceBuffer((nv + 1) * 8), dev.DeviceBuffer(6 * nf * 4), dev.DeviceBuffer(nv * 24)]
    d_v, d_f, d_st, d_nb, d_out = (C.c_void_p(b.ptr) for b in bufs)
    try:
        for rep in range(2):
            before, total = dev.sync_count(), C.c_int64(0)
            L.check(lib.pb3d_mesh_adjacency_resident(ctx, d_f, 1, nv, nf, d_st, d_nb, None, None, C.byref(total)))
            adj_waits = dev.sync_count() - before
            before = dev.sync_count()
            L.check(lib.pb3d_mesh_smooth_resident(ctx, d_v, 1, nv, d_f, 1, nf, 10, 0.5, -0.53, None, 1, d_out))
            smooth_waits = dev.sync_count() - before
        print("host waits: adjacency", adj_waits, "smooth", smooth_waits)
        assert total.value == len(want_adjacency("radix/70000")[1])
        assert adj_waits == 2 and smooth_waits == 1
        before = dev.sync_count()                                       # nf = 0: nothing to check, nothing to wait for
        L.check(lib.pb3d_mesh_adjacency_resident(ctx, None, 1, nv, 0, d_st, None, None, None, C.byref(total)))
        L.check(lib.pb3d_mesh_smooth_resident(ctx, d_v, 1, nv, None, 1, 0, 10, 0.5, -0.53, None, 1, d_out))
        assert total.value == 0 and dev.sync_count() == before
        assert not bufs[2].download((nv + 1,), np.int64).any() and bufs[4].download((nv, 3), np.float64).tobytes() == v.tobytes()
    finally:
        for b in bufs:
            b.free()


# the host waits of the warm resident chain: the mesh counts, the index check of the smoothing, the index check of the normals
CHAIN_WAITS = 3


@gpu
def test_resident_chain(pb3d_gpu):
    """meshify -> smooth_mesh_resident -> vertex_normals_resident with everything resident equals the chain through the NumPy forms, and
    waits for the host CHAIN_WAITS times"""
    import synth_host
    from pb3d import eval_helpers as eh
    dev = pb3d_gpu.device
    S = 48
    x, y, z = np.mgrid[0:S, 0:S, 0:S]
    ball = (x - 23.5) ** 2 + (y - 23.5) ** 2 * 1.7 + (z - 23.5) ** 2 < 20.0 ** 2
    grid = np.ascontiguousarray(synth_host.sem_slab(0, S, S, S, 48) * ball[..., None].astype(np.uint8))
    v, f = pb3d_gpu.meshify_colored_voxel_grid(grid)[:2]
    smoothed = pb3d_gpu.smooth_mesh(v, f)
    normals = pb3d_gpu.compute_vertex_normals(smoothed, f)
    assert v.dtype == np.float32 and len(v) > 5000
    same_bytes(smoothed, sr.restate(v, f), "chain/numpy")
    assert sr.mean_dihedral_deg(smoothed, f) < sr.mean_dihedral_deg(v, f)

    d_grid = dev.DeviceGrid(dev.from_numpy(grid), grid.shape)
    for rep in range(2):
        held = []
        try:
            before = dev.sync_count()
            (dv, df, dn, dc), (nv, nf) = dev.meshify(d_grid, grid.shape, download=False)
            held += [dv, df, dn, dc]
            d_s = pb3d_gpu.smooth_mesh_resident(dv, nv, df, nf)
            held.append(d_s)
            d_n = eh.vertex_normals_resident(d_s, nv, df, nf)
            held.append(d_n)
            waits = dev.sync_count() - before
            assert (nv, nf) == (len(v), len(f))
            same_bytes(d_s.download((nv, 3), np.float32), smoothed, "chain/resident")
            same_bytes(d_n.download((nv, 3), np.float32), np.ascontiguousarray(normals), "chain/normals")
        finally:
            for b in held:
                b.free()
    d_grid.free()
    print("host waits of the warm chain:", waits)
    assert waits <= CHAIN_WAITS
