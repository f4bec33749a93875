"""The notebook-4 visibility kernels (csrc/visibility.hip) against a vectorised NumPy restatement, compared exactly: float32 bit
patterns, uint32 bit images and int64 counts.

The restatement is the reference's arithmetic (utils/eval_helpers_intra.py:134-190) with NumPy's own promotion rules: the camera's
width, weak Python f / cx / cy / eps against NumPy scalars.  Its one deviation from the reference's text is the matmul: each
component of (p - cam) @ R.T is written out as the chain fma(d2, r2, fma(d1, r1, d0 * r0)) that NumPy's gemm evaluates
(csrc/project.hip), with correctly rounded FMAs emulated in float64 (float32) and by Boldo and Melquiond's rounding-to-odd
construction (float64).  So the restatement is exact for any camera, not only for the signed-permutation views the scalar
references of test_projection_edges are limited to; on those views the CPU tests below pin it to them.

The GPU tests reach the kernels' shape-dependent paths on purpose:
  * grid walk: A0 in {1, 63, 64, 65, 129} (the 64-step kChunk seam along a0), A2 mod 4 in {0, 1, 2, 3} (dword loads when
    A2 % 4 == 0 on an aligned grid, byte loads otherwise), grids at byte offsets 1..3 with A2 % 4 == 0 (byte loads on an
    unaligned pointer), C = 1 labels and C = 3 RGB, cameras along a0 (long runs per pixel), along a2 (the pixel changes every
    voxel), oblique, straight down and inside the grid (voxels behind the camera are dropped mid-run);
  * |Z - zbuf| exactly eps, one ulp under and one over, for the grid walk and the point-list kernel;
  * k_iou_rows: 1, 7 and 32 rows (lane r keeps row r), npix tails that are not multiples of 64, null pred / gt and gated rows;
  * presence: nvox mod 4 in {0..3}, unaligned grids, every non-black colour once, a wave of distinct keys (the leader loop).
"""
from fractions import Fraction

import numpy as np
import pytest

from test_projection_edges import (VIS_EPS, assert_signed_permutation, axis_views, ref_depth, ref_look_at,
                                   ref_visible, tie_cases, visibility_cases)

gpu = pytest.mark.gpu
ANY = 1 << 31
MONUMENTS = ["Taj", "Bibi", "Itimad", "Akbar", "Charminar"]
PARTS = ["dome", "chhatris", "main_door", "windows", "plinth"]
MINARETS = ["LM1", "RM1", "LM2", "RM2"]

# =====================================================================================================================
# Correctly rounded FMAs on float64 arrays
# =====================================================================================================================


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(x):
    t = 134217729.0 * x                     # 2^27 + 1: Veltkamp's split into two 26-bit halves
    hi = t - (t - x)
    return hi, x - hi


def fma32(a, b, c):
    """float32 fma(a, b, c), correctly rounded: a * b is exact in float64 and a * b + c is exact as a float64 pair (s, e); s
    rounds to float32 like s + e unless s is a float32 midpoint that e moves off"""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    s, e = _two_sum(a * b, c)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    n = np.nextafter(r, np.where(s > r64, np.float32(np.inf), np.float32(-np.inf)))
    n64 = n.astype(np.float64)
    tie = (e != 0) & (s != r64) & (2 * s == r64 + n64)
    return np.where(tie & ((e > 0) == (n64 > r64)), n, r)


def fma64(a, b, c):
    """float64 fma(a, b, c), correctly rounded: exact product (Dekker), exact sum with c, the tail rounded to odd, one final
    round to nearest (Boldo and Melquiond, 'Emulation of FMA and correctly rounded sums', 2008)"""
    a, b, c = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (a, b, c)))
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    pe = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s, t = _two_sum(c, p)
    u, v = _two_sum(t, pe)
    even = (u.view(np.int64) & 1) == 0
    u = np.where((v != 0) & even, np.nextafter(u, np.where(v > 0, np.inf, -np.inf)), u)
    return s + u


# =====================================================================================================================
# The restatement
# =====================================================================================================================

def ref_frame(pts, cam):
    """X, Y, Z of (pts - cam_pos) @ R.T in the width NumPy gives (pts, cam_pos, R); R is the host's look_at_rotation"""
    from pb3d.camera_geometry import look_at_rotation
    pts = np.asarray(pts).reshape(-1, 3)
    eye, tgt = np.asarray(cam["cam_pos"]), np.asarray(cam["target"])
    R = look_at_rotation(eye, tgt)
    wt = np.result_type(pts, eye, R)
    d = pts.astype(wt) - eye.astype(wt)
    Rw = R.astype(wt)
    fma = fma64 if wt == np.float64 else fma32
    return [fma(d[:, 2], Rw[r, 2], fma(d[:, 1], Rw[r, 1], d[:, 0] * Rw[r, 0])).astype(wt) for r in range(3)]


def ref_pixels(pts, cam, H, W, chunk=1 << 20):
    """(ui, vi, Z, index) of the points the z-buffer functions keep: Z > 1e-6, rounded pixel inside the image.  Long lists go in
    chunks over a few threads (NumPy releases the GIL); every point is independent, so the result does not depend on it."""
    pts = np.asarray(pts).reshape(-1, 3)
    if len(pts) > chunk:
        import os
        from concurrent.futures import ThreadPoolExecutor
        starts = range(0, len(pts), chunk)
        with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
            parts = list(pool.map(lambda s: ref_pixels(pts[s:s + chunk], cam, H, W, chunk), starts))
        return tuple(np.concatenate([p[k] + (s if k == 3 else 0) for s, p in zip(starts, parts)]) for k in range(4))
    X, Y, Z = ref_frame(pts, cam)
    keep = np.flatnonzero(Z > 1e-6)
    X, Y, Z = X[keep], Y[keep], Z[keep]
    u = np.round((X / Z) * cam["f"] + cam["cx"])
    v = np.round(-(Y / Z) * cam["f"] + cam["cy"])
    inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    return u[inside].astype(np.int64), v[inside].astype(np.int64), Z[inside], keep[inside]


def ref_points_zbuf(pts, cam, H, W):
    return zbuf_of(ref_pixels(pts, cam, H, W), H, W)


def _keys(grid, C):
    g = np.asarray(grid)
    if C == 1:
        return g.astype(np.uint32)
    return g[..., 0].astype(np.uint32) | (g[..., 1].astype(np.uint32) << 8) | (g[..., 2].astype(np.uint32) << 16)


def _colour_keys(colours, C):
    t = np.asarray(colours, np.int64).reshape(-1, C) if len(colours) else np.zeros((0, C), np.int64)
    return _keys(t.astype(np.uint8), C).reshape(-1)


def _grid_points(keys):
    """voxel (a0, a1, a2) is the float32 point (a2, a1, a0)"""
    a0, a1, a2 = np.nonzero(keys)
    return np.stack([a2, a1, a0], 1).astype(np.float32), keys[a0, a1, a2]


def _channels(grid):
    return 3 if np.asarray(grid).ndim == 4 else 1


def ref_grid_zbuf(grid, cam, H, W):
    """compute_global_depth_buffer of a (A0, A1, A2, 3) RGB or (A0, A1, A2) label grid"""
    return zbuf_of(ref_grid_project(grid, cam, H, W), H, W)


def _visible(Z, zbuf, vi, ui, eps):
    return np.abs(Z - np.asarray(zbuf, np.float32)[vi, ui]) < eps


def ref_grid_project(grid, cam, H, W, points=None):
    """(ui, vi, Z, key) of the grid's occupied voxels that land in the image; points: the grid's _grid_points, if known"""
    pts, keys = points if points is not None else _grid_points(_keys(grid, _channels(grid)))
    ui, vi, Z, idx = ref_pixels(pts, cam, H, W)
    return ui, vi, Z, keys[idx]


def zbuf_of(proj, H, W):
    ui, vi, Z, _ = proj
    zb = np.full((H, W), np.inf, np.float32)
    np.minimum.at(zb, (vi, ui), Z.astype(np.float32))
    return zb


def bits_of(proj, colours, C, zbuf, H, W, eps=1e-3):
    ui, vi, Z, keys = proj
    vis = _visible(Z, zbuf, vi, ui, eps)
    k = keys[vis]
    b = np.full(len(k), ANY, np.uint32)
    for j, c in enumerate(_colour_keys(colours, C)):
        b |= (k == c).astype(np.uint32) << np.uint32(j)
    bits = np.zeros((H, W), np.uint32)
    np.bitwise_or.at(bits, (vi[vis], ui[vis]), b)
    return bits


def ref_grid_bits(grid, colours, cam, zbuf, H, W, eps=1e-3):
    """bit k: a visible voxel of colour (or label) k; bit 31: any visible occupied voxel"""
    return bits_of(ref_grid_project(grid, cam, H, W), colours, _channels(grid), zbuf, H, W, eps)


def ref_points_bits(lists, cam, zbuf, H, W, eps=1e-3):
    """bit k: some point of lists[k] is visible"""
    bits = np.zeros((H, W), np.uint32)
    for j, pts in enumerate(lists):
        ui, vi, Z, _ = ref_pixels(pts, cam, H, W)
        vis = _visible(Z, zbuf, vi, ui, eps)
        bits[vi[vis], ui[vis]] |= np.uint32(1 << j)
    return bits


def ref_presence(grid_keys, colour_keys=()):
    """(bitmap, present) of a colour set: bit `key` of the 2^24-bit map for every non-zero key; bit k of present for the colour
    keys that occur"""
    on = np.zeros(1 << 24, bool)
    on[np.asarray(grid_keys, np.int64).ravel()] = True
    on[0] = False
    present = sum(1 << k for k, c in enumerate(colour_keys) if on[int(c)])
    return np.packbits(on, bitorder="little").view("<u4"), present


def ref_mask_bits(mask, colours, grid_keys=None):
    """bit k: the mask pixel has colour k; bit 31 (when a grid's keys are given): the pixel is not black and its colour is in the grid"""
    key = _keys(np.asarray(mask).reshape(-1, 3), 3)
    bits = np.zeros(len(key), np.uint32)
    for j, c in enumerate(_colour_keys(colours, 3)):
        bits |= (key == c).astype(np.uint32) << np.uint32(j)
    if grid_keys is not None:
        bits |= np.where((key != 0) & np.isin(key, np.asarray(grid_keys, np.uint32)), np.uint32(ANY), np.uint32(0))
    return bits


def ref_iou_rows(rows, npix):
    """rows of (pred image or None, pred bits, gt image or None, gt bits, gate image or None, gate bits): pred = pred & pred_bits,
    gt = gt & gt_bits [& gate & gate_bits]; (|pred & gt|, |pred | gt|) per row, int64"""
    def hit(img, m):
        return np.zeros(npix, bool) if img is None else (np.asarray(img, np.uint32).ravel()[:npix] & np.uint32(m & 0xffffffff)) != 0
    out = np.zeros((len(rows), 2), np.int64)
    for r, (pi, pm, gi, gm, ki, km) in enumerate(rows):
        pr, gt = hit(pi, pm), hit(gi, gm)
        if ki is not None:
            gt &= hit(ki, km)
        out[r] = np.count_nonzero(pr & gt), np.count_nonzero(pr | gt)
    return out


# =====================================================================================================================
# Cases
# =====================================================================================================================

TIE_EPS = dict(VIS_EPS, **{"py1e-4": 1e-4, "np32_1e-4": np.float32(1e-4), "np64_1e-4": np.float64(1e-4)})
TIE_A1, TIE_A2 = 3, 8


def eps_tie_cases():
    """A (2, 3, 8) grid under a camera at z = -d looking along +z (R = I, f = d, cx = 0, cy = 2): the voxels of plane a0 = 0 have
    Z = d exactly and land on distinct pixels (a2, 2 - a1); plane a0 = 1 lands on pixel (0, 2).  zbuf per pixel: 0 and 2d
    (|Z - zbuf| = d, that is Z -+ d), d, +inf, NaN, 7.  d is eps in the width of the compare, one ulp under and one ulp over.
    Checked here: wherever the camera's width holds that eps, all three distances really occur."""
    assert float(np.float32(1e-4)) < 1e-4            # its float32 rounding is below it: weak and float64 eps must differ
    out = []
    rng = np.random.default_rng(31)
    for ename, eps in TIE_EPS.items():
        for cdt in (np.float32, np.float64):
            E = np.result_type(cdt, eps).type(eps)   # eps in the width of the compare (float32 grid points, cdt camera)
            Ed = cdt(E)
            found = set()
            for d in (Ed, np.nextafter(Ed, cdt(0)), np.nextafter(Ed, cdt(1))):
                cam = {"cam_pos": np.array([0, 0, -d], cdt), "target": np.array([0, 0, 1], cdt), "f": float(d), "cx": 0.0, "cy": 2.0}
                assert_signed_permutation(ref_look_at(cam["cam_pos"], cam["target"]))
                grid = np.zeros((2, TIE_A1, TIE_A2, 3), np.uint8)
                grid[0] = rng.integers(1, 4, (TIE_A1, TIE_A2, 1)) * np.array([60, 1, 7], np.uint8)
                grid[1, rng.random((TIE_A1, TIE_A2)) < 0.5] = (200, 9, 9)
                zb = np.array([0.0, 2 * d, d, np.inf, np.nan, 7.0], np.float64)
                zbuf = zb[np.arange(TIE_A1 * TIE_A2) % len(zb)].reshape(TIE_A1, TIE_A2)[::-1].astype(np.float32)
                case = {"name": f"{ename}-{cdt.__name__}cam-d{d!r}", "grid": grid, "cam": cam, "zbuf": zbuf, "eps": eps, "H": TIE_A1,
                        "W": TIE_A2, "colours": np.array([[60, 1, 7], [120, 2, 14], [200, 9, 9]], np.uint8)}
                pts, _ = _grid_points(_keys(grid, 3))
                ui, vi, Z, _ = ref_pixels(pts, cam, TIE_A1, TIE_A2)
                front = Z == d
                assert np.count_nonzero(front) == TIE_A1 * TIE_A2 and len(set(zip(ui[front], vi[front]))) == TIE_A1 * TIE_A2
                dz = np.abs(Z - zbuf[vi, ui])
                found |= {x for x in (E, np.nextafter(E, E.dtype.type(0)), np.nextafter(E, E.dtype.type(1))) if np.any(dz == x)}
                out.append(case)
            if E.dtype == cdt:                   # the compare is in the camera's width (not a float32 camera against float64 eps)
                assert len(found) == 3, (ename, cdt, found)
    return out


def small_random_grids():
    rng = np.random.default_rng(8)
    out = []
    for shape in ((6, 5, 7), (9, 4, 8), (3, 6, 5)):
        pal = rng.integers(1, 256, (4, 3)).astype(np.uint8)
        g = pal[rng.integers(0, 4, shape)]
        g[rng.random(shape) < 0.4] = 0
        out.append((g, pal[:3]))
    return out


# =====================================================================================================================
# CPU: the FMAs, and the restatement against the scalar references of test_projection_edges
# =====================================================================================================================

def _round_exact(x, dt):
    """Fraction x rounded to nearest-even in dt"""
    y = dt(float(x))
    cands = [np.nextafter(y, dt(-np.inf)), y, np.nextafter(y, dt(np.inf))]
    ity = np.int32 if dt == np.float32 else np.int64
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - x), int(np.array(c, dt).view(ity)) & 1))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_fma_emulation_is_correctly_rounded(dt):
    rng = np.random.default_rng(17)
    n = 3000
    a = (rng.normal(size=n) * 2.0 ** rng.integers(-8, 9, n)).astype(dt)
    b = rng.normal(size=n).astype(dt)
    c = (rng.normal(size=n) * 2.0 ** rng.integers(-20, 9, n)).astype(dt)
    c[::3] = -(a[::3].astype(np.float64) * b[::3]).astype(dt)                # cancellation: the result is the product's tail
    if dt == np.float32:        # (2^12 + 1)^2 is a float32 midpoint; a tiny c decides the rounding, which float64 alone would lose
        a[:2] = b[:2] = 4097.0
        c[:2] = (2.0 ** -30, -2.0 ** -30)
        fma = fma32
    else:                       # (2^26 + 1)(2^27 + 1) is a float64 midpoint
        a[:2], b[:2] = 2.0 ** 26 + 1, 2.0 ** 27 + 1
        c[:2] = (2.0 ** -20, -2.0 ** -20)
        fma = fma64
    got = fma(a, b, c)
    want = [_round_exact(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)), dt) for x, y, z in zip(a, b, c)]
    assert np.array_equal(got, np.array(want, dt))
    mid = int(a[0]) * int(b[0])
    assert int(got[0]) == mid + 1 and int(got[1]) == mid - 1          # the tiny c broke the tie both ways


def test_restatement_equals_scalar_references():
    """the vectorised z-buffer and visibility equal ref_depth / ref_visible (test_projection_edges, pinned to the oracle) on the tie
    cases, the visibility cases and small random grids under the six axis views"""
    for case in tie_cases():
        pts, cam, H, W = case["pts"], case["cam"], case["H"], case["W"]
        zb = ref_points_zbuf(pts, cam, H, W)
        assert np.array_equal(zb.view(np.uint32), ref_depth(pts, cam, H, W).view(np.uint32)), case["name"]
        assert np.array_equal(ref_points_bits([pts[::3]], cam, zb, H, W) != 0, ref_visible(pts[::3], cam, zb, H, W, 1e-3)), case["name"]
    for case in visibility_cases():
        pts, cam, H, W = case["pts"], case["cam"], case["H"], case["W"]
        want = ref_visible(pts, cam, case["zbuf"], H, W, case["eps"])
        assert np.array_equal(ref_points_bits([pts], cam, case["zbuf"], H, W, case["eps"]) != 0, want), case["name"]
    for g, pal in small_random_grids():
        A0, A1, A2 = g.shape[:3]
        pts, _ = _grid_points(_keys(g, 3))
        for dtype in (np.float32, np.float64):
            for view in axis_views((A2 / 2, A1 / 2, A0 / 2), 12, dtype):
                for f, cx, cy in ((6.0, 5.5, 4.0), (np.float64(6.0), 5.0, np.float32(4.5))):
                    cam = dict(view, f=f, cx=cx, cy=cy)
                    zb = ref_grid_zbuf(g, cam, 9, 11)
                    assert np.array_equal(zb.view(np.uint32), ref_depth(pts, cam, 9, 11).view(np.uint32))
                    bits = ref_grid_bits(g, pal, cam, zb, 9, 11)
                    assert np.array_equal((bits >> 31) != 0, ref_visible(pts, cam, zb, 9, 11, 1e-3))
                    for k, c in enumerate(pal):
                        a0, a1, a2 = np.nonzero(np.all(g == c, axis=-1))
                        sel = np.stack([a2, a1, a0], 1).astype(np.float32)
                        assert np.array_equal((bits >> k) & 1 != 0, ref_visible(sel, cam, zb, 9, 11, 1e-3))
                    assert bits.any()


def test_eps_tie_restatement_equals_scalar_reference():
    cases = eps_tie_cases()
    assert len(cases) == 3 * 2 * len(TIE_EPS)
    for case in cases:
        pts, _ = _grid_points(_keys(case["grid"], 3))
        want = ref_visible(pts, case["cam"], case["zbuf"], case["H"], case["W"], case["eps"])
        bits = ref_grid_bits(case["grid"], case["colours"], case["cam"], case["zbuf"], case["H"], case["W"], case["eps"])
        assert np.array_equal((bits >> 31) != 0, want) and want.any() and not want.all(), case["name"]


def test_restatement_general_camera_is_the_fma_chain():
    """an oblique camera: each component is the FMA chain rounded once per FMA (checked against exact fractions)"""
    from pb3d.camera_geometry import look_at_rotation
    rng = np.random.default_rng(4)
    pts = rng.integers(0, 60, (200, 3)).astype(np.float32)
    for cdt in (np.float32, np.float64):
        cam = {"cam_pos": np.array([-40.5, 70.25, -55], cdt), "target": np.array([30, 20.5, 31], cdt)}
        R = look_at_rotation(cam["cam_pos"], cam["target"])
        assert not np.all((R == 0) | (np.abs(R) == 1))
        wt = np.result_type(pts, cam["cam_pos"], R)
        got = ref_frame(pts, cam)
        d = pts.astype(wt) - cam["cam_pos"].astype(wt)
        for r in range(3):
            for i in range(0, 200, 7):
                acc = wt.type(d[i, 0] * wt.type(R[r, 0]))
                for k in (1, 2):
                    acc = _round_exact(Fraction(float(d[i, k])) * Fraction(float(wt.type(R[r, k]))) + Fraction(float(acc)), wt.type)
                assert got[r][i] == acc


@pytest.mark.parametrize("dt", [np.int64, np.int32, np.uint32, np.uint64])
def test_camera_args_keeps_integer_points_exact(dt):
    """integer points that NumPy promotes with the camera to float64 go to the kernels as float64: 2^24 + 1 stays 2^24 + 1"""
    from pb3d.projection_utils import camera_args, points_f64
    pts = np.array([[2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 1], [3, 5, 7]], dt)
    for cdt in (np.float32, np.float64):
        p, pf64, R, cp, prec = camera_args(pts, np.array([0, 0, -5], cdt), np.array([0, 0, 1], cdt), 4.0, 1.0, 1.0)
        assert pf64 == 1 and p.dtype == np.float64 and np.array_equal(p, pts.astype(np.float64)) and p[0, 0] == 16777217.0
        assert prec[0] == 1 and np.result_type(pts, cdt) == np.float64
    assert points_f64(dt)
    for dt in (np.int16, np.uint8, np.float32, np.bool_):          # exact in float32: stay float32, the camera decides prec
        p, pf64, _, _, prec = camera_args(np.ones((2, 3), dt), np.zeros(3, np.float32), np.ones(3, np.float32), 4.0, 1.0, 1.0)
        assert pf64 == 0 and p.dtype == np.float32 and not points_f64(dt)
    p, pf64, _, _, _ = camera_args(np.ones((2, 3), np.float64), np.zeros(3, np.float32), np.ones(3, np.float32), 4.0, 1.0, 1.0)
    assert pf64 == 1 and p.dtype == np.float64


# =====================================================================================================================
# GPU helpers
# =====================================================================================================================

class _At:
    """a device pointer at a byte offset inside a buffer, for the *_resident entries (which read .ptr)"""

    def __init__(self, buf, off):
        self.ptr = buf.ptr + int(off)


class Bufs:
    """device buffers of one call; all freed on exit"""

    def __init__(self, pb3d):
        self.dev = pb3d.device
        self.held = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.held:
            b.free()

    def keep(self, b):
        self.held.append(b)
        return b

    def put(self, a, off=0):
        a = np.ascontiguousarray(a)
        b = self.keep(self.dev.DeviceBuffer(off + max(a.nbytes, 4)))
        if a.nbytes:
            b.upload(a, off)
        return _At(b, off)

    def empty(self, nbytes):
        return self.keep(self.dev.DeviceBuffer(max(int(nbytes), 4)))


def dev_grid_walk(pb3d, grid, colours, cam, zbuf, H, W, eps=1e-3, off=0):
    """(z-buffer, visible bits) of the grid-walk kernels, the grid at byte `off` of its buffer, the bits against `zbuf`"""
    ev = pb3d.eval_helpers_intra
    g = np.ascontiguousarray(grid)
    shape = g.shape[:3] + (_channels(g),)
    with Bufs(pb3d) as b:
        d_g = b.put(g, off)
        d_z = b.keep(ev.depth_buffer_resident(d_g, shape, cam, H, W))
        d_b = b.keep(ev.visible_bits_resident(d_g, shape, colours, cam, b.put(np.asarray(zbuf, np.float32)), (H, W), H, W, eps))
        return d_z.download((H, W), np.float32), d_b.download((H, W), np.uint32)


def check_walk(pb3d, grid, colours, cam, H, W, what, off=0, eps=1e-3):
    zb = ref_grid_zbuf(grid, cam, H, W)
    want = ref_grid_bits(grid, colours, cam, zb, H, W, eps)
    got_z, got_b = dev_grid_walk(pb3d, grid, colours, cam, zb, H, W, eps, off)
    assert np.array_equal(got_z.view(np.uint32), zb.view(np.uint32)), what
    assert np.array_equal(got_b, want), what
    return zb, want


def walk_cams(shape, H, W, cdt):
    """along a0, along a2, oblique, straight down, inside the grid (points are (a2, a1, a0))"""
    A0, A1, A2 = shape
    c = np.array([A2 / 2, A1 / 2, A0 / 2])
    ext = float(max(shape))
    D = 2 * ext + 6

    def cam(eye, tgt, f):
        return {"cam_pos": np.asarray(eye, cdt), "target": np.asarray(tgt, cdt), "f": f, "cx": W / 2 - 0.5, "cy": H / 2 + 0.25}
    return {
        "a0": cam([c[0] + 0.25, c[1] - 0.5, -D], [c[0] + 0.25, c[1] - 0.5, c[2]], 0.6 * min(H, W) * D / ext),
        "a2": cam([-D, c[1], c[2] + 0.5], [c[0], c[1], c[2] + 0.5], 1.2 * (D + ext)),
        "oblique": cam(c + [-0.55 * D, 0.35 * D, -0.75 * D], c + [0.3, -0.2, 0.1], 0.5 * min(H, W) * D / ext),
        "down": cam([c[0] + 0.5, A1 + D, c[2] - 0.25], [c[0] + 0.5, c[1], c[2] - 0.25], 0.6 * min(H, W) * D / ext),
        "inside": cam(c + [0.3, 0.1, -0.2], c + [0.7, 0.4, 40], 0.5 * W),
    }


def _walk_grid(shape, C, seed):
    rng = np.random.default_rng(seed)
    pal = np.array([[60, 1, 7], [120, 2, 14], [200, 9, 9], [3, 250, 40], [9, 9, 9], [255, 255, 255]], np.uint8)
    idx = rng.integers(0, len(pal), shape)
    occ = rng.random(shape) < 0.3
    if C == 3:
        g = np.where(occ[..., None], pal[idx], 0).astype(np.uint8)
        return g, pal[:5]
    g = np.where(occ, idx * 40 + 1, 0).astype(np.uint8)
    return g, (np.arange(5) * 40 + 1).astype(np.uint8).reshape(-1, 1)


# =====================================================================================================================
# GPU 1: the grid walk
# =====================================================================================================================

@gpu
@pytest.mark.parametrize("A0", [1, 63, 64, 65, 129])
def test_grid_walk_shapes_cameras_widths(pb3d_gpu, A0):
    """z-buffer and visible bits of every A2 mod 4, C = 1 and 3, five cameras, float32 / float64 cameras and Python /
    float64 f equal the restatement bit for bit"""
    H, W = 40, 48
    seen = set()
    for A2 in (16, 17, 18, 19):
        for C in (1, 3):
            g, cols = _walk_grid((A0, 5, A2), C, A0 * 100 + A2 * 3 + C)
            for cdt, fkind in ((np.float32, float), (np.float64, float), (np.float32, np.float64)):
                for name, cam in walk_cams(g.shape[:3], H, W, cdt).items():
                    cam = dict(cam, f=fkind(cam["f"]))
                    zb, bits = check_walk(pb3d_gpu, g, cols, cam, H, W, (A0, A2, C, cdt.__name__, fkind.__name__, name))
                    if np.isfinite(zb).any() and (bits & 1).any():
                        seen.add(name)
    assert seen >= {"a0", "a2", "oblique", "down"} | ({"inside"} if A0 > 1 else set()), seen


@gpu
def test_grid_walk_unaligned_and_medium(pb3d_gpu):
    """A2 % 4 == 0 grids at byte offsets 0 and 4 (dword loads) and 1..3 (byte loads on an unaligned pointer), C = 1 and 3; and a
    sparse 400 x 256 x 400 grid whose columns flush many runs onto the same pixels"""
    H, W = 36, 44
    for C in (1, 3):
        g, cols = _walk_grid((70, 6, 20), C, 5 + C)
        for cdt in (np.float32, np.float64):
            for name, cam in walk_cams(g.shape[:3], H, W, cdt).items():
                for off in (0, 1, 2, 3, 4):
                    check_walk(pb3d_gpu, g, cols, cam, H, W, (C, cdt.__name__, name, off), off=off)
    rng = np.random.default_rng(400)
    pal = np.array([[60, 1, 7], [120, 2, 14], [200, 9, 9], [3, 250, 40]], np.uint8)
    shape = (400, 256, 400)
    occ = rng.integers(0, 100, shape, dtype=np.uint8) == 0
    g = np.zeros(shape + (3,), np.uint8)
    g[occ] = pal[rng.integers(0, len(pal), int(occ.sum()))]
    for name in ("a0", "oblique"):
        cam = walk_cams(shape, 240, 320, np.float32)[name]
        zb, bits = check_walk(pb3d_gpu, g, pal[:3], cam, 240, 320, ("medium", name))
        assert np.isfinite(zb).sum() > 5000 and (bits & 7).any()


# =====================================================================================================================
# GPU 2: the eps tie on both kernels
# =====================================================================================================================

@gpu
def test_eps_tie_grid_and_points(pb3d_gpu):
    """|Z - zbuf| == eps, one ulp under and over, with eps weak, float32 and float64 (1e-3, 2^-10, 1e-4), float32 and float64
    cameras, and zbuf +inf, NaN, 0: the grid walk and the point-list kernel (float32, float64 and int64 lists)"""
    for case in eps_tie_cases():
        g, cam, zbuf, eps, H, W = case["grid"], case["cam"], case["zbuf"], case["eps"], case["H"], case["W"]
        want = ref_grid_bits(g, case["colours"], cam, zbuf, H, W, eps)
        _, got = dev_grid_walk(pb3d_gpu, g, case["colours"], cam, zbuf, H, W, eps)
        assert np.array_equal(got, want), case["name"]
        pts, keys = _grid_points(_keys(g, 3))
        lists = [pts[keys == c] for c in _colour_keys(case["colours"], 3)] + [pts]
        for dt in (np.float32, np.float64, np.int64):
            ls = [p.astype(dt) for p in lists]
            want = ref_points_bits(ls, cam, zbuf, H, W, eps)
            assert want.any() and np.array_equal(pb3d_gpu.points_visible_bits(ls, cam, zbuf, H, W, eps), want), (case["name"], dt)


# =====================================================================================================================
# GPU 3: point lists
# =====================================================================================================================

def _lists(rng, dt, lengths):
    out = []
    for n in lengths:
        p = rng.uniform(0, 40, (n, 3))
        out.append(np.round(p).astype(dt) if dt == np.int64 else p.astype(dt))
    return out


@gpu
def test_points_visible_bits_lists(pb3d_gpu):
    """1, 2 and 31 lists of float32, float64 and int64 points with lengths 0, 1, 255, 256, 257 and 1 000 003 in one call (the
    grid stride runs over the longest list); 32 lists, mixed dtypes and a zbuf of the wrong shape are refused"""
    H, W = 48, 64
    rng = np.random.default_rng(31)
    cams = {cdt: {"cam_pos": np.array([-30.5, 55.25, -42], cdt), "target": np.array([20, 18.5, 21], cdt), "f": 70.0, "cx": 31.5,
                  "cy": 23.0} for cdt in (np.float32, np.float64)}
    for dt in (np.float32, np.float64, np.int64):
        for lengths in ([257], [1000003, 0], [0, 1, 255, 256, 257] * 6 + [1000003]):
            ls = _lists(rng, dt, lengths)
            for cdt, cam in cams.items():
                if cdt == np.float64 and len(lengths) != 2:
                    continue
                zb = ref_points_zbuf(np.concatenate(ls), cam, H, W)
                want = ref_points_bits(ls, cam, zb, H, W)
                assert np.array_equal(pb3d_gpu.points_visible_bits(ls, cam, zb, H, W), want), (dt, lengths[:3], cdt)
                assert want.any() and not any(((want >> k) & 1).any() for k, n in enumerate(lengths) if n == 0)
    zb = np.zeros((H, W), np.float32)
    with pytest.raises(ValueError, match="at most 31"):
        pb3d_gpu.points_visible_bits(_lists(rng, np.float32, [3] * 32), cams[np.float32], zb, H, W)
    with pytest.raises(TypeError):
        pb3d_gpu.points_visible_bits(_lists(rng, np.float32, [3]) + _lists(rng, np.float64, [3]), cams[np.float32], zb, H, W)
    with pytest.raises(ValueError, match="zbuf is"):
        pb3d_gpu.points_visible_bits(_lists(rng, np.float32, [3]), cams[np.float32], np.zeros((H, W + 1), np.float32), H, W)


@gpu
def test_int64_points_beyond_2_24(pb3d_gpu):
    """int64 coordinates at and past 2^24 (odd ones are not float32 values) under a float32 camera next to them: the point-list
    kernel and project_part_visible both equal the restatement, which subtracts in float64 as NumPy does"""
    H, W = 8, 8
    base = 1 << 24
    j, r = np.meshgrid(np.arange(-2, 6), np.arange(8), indexing="ij")
    pts = np.stack([base + j.ravel(), r.ravel(), np.zeros(j.size, np.int64)], 1).astype(np.int64)
    for x0 in (base, 2 * base):
        # pixel (j + 2, 7 - r) for the point (x0 + j, r, 0): every pixel once, no negative coordinate (the unsigned types)
        sel = pts + np.array([x0 - base, 0, 0])
        assert np.count_nonzero(sel[:, 0].astype(np.float32).astype(np.int64) != sel[:, 0]) >= 8
        cam = {"cam_pos": np.array([x0, 0, -8], np.float32), "target": np.array([x0, 0, 100], np.float32), "f": 8.0, "cx": 2.0, "cy": 7.0}
        zb = ref_points_zbuf(sel, cam, H, W)
        want = ref_points_bits([sel], cam, zb, H, W)
        assert np.count_nonzero(want) == H * W
        assert np.array_equal(pb3d_gpu.points_visible_bits([sel], cam, zb, H, W), want), x0
        for dt in (np.int64, np.int32, np.uint32, np.uint64):
            assert np.array_equal(pb3d_gpu.project_part_visible(sel.astype(dt), cam, zb, H, W), want != 0), (x0, dt)
        from pb3d import dist
        img, _ = dist.project_colored_voxels_sharded(sel, np.full((len(sel), 3), 9, np.uint8), 0, cam["cam_pos"], cam["target"],
                                                     cam["f"], cam["cx"], cam["cy"], H, W, reduce=False)
        assert (img == 9).all() and (pb3d_gpu.project_colored_voxels(sel, np.full((len(sel), 3), 9, np.uint8), cam["cam_pos"],
                                                                     cam["target"], cam["f"], cam["cx"], cam["cy"], H, W) == 9).all(), x0


# =====================================================================================================================
# GPU 4: colour presence and mask bits
# =====================================================================================================================

def dev_presence(pb3d, flat, C, colours=(), off=0):
    """(bitmap words, present) of presence_resident on a flat (nvox,) label or (nvox, 3) RGB array at byte `off`"""
    ev = pb3d.eval_helpers_intra
    with Bufs(pb3d) as b:
        d_g = b.put(flat, off)
        d_p = b.empty(8)
        d_bm = b.keep(ev.presence_resident(d_g, (len(flat), 1, 1, C), colours, d_p if len(colours) else None))
        present = int(d_p.download((1,), np.int64)[0]) if len(colours) else 0
        return d_bm.download((pb3d._lib.PRESENCE_BYTES // 4,), np.uint32), present


@gpu
def test_color_presence_tails_offsets_and_waves(pb3d_gpu):
    """nvox mod 4 in {0..3} at byte offsets 0..3 (dword and byte loads), C = 1 and 3, with the present bits of a colour table;
    a wave whose 64 lanes hold 256 distinct keys, repeated (shifted) by the later waves"""
    rng = np.random.default_rng(24)
    for C in (1, 3):
        pal = rng.integers(0, 256, (300, C)).astype(np.uint8)
        table = np.concatenate([pal[1:20], rng.integers(1, 256, (5, C)).astype(np.uint8)])
        table = table[_colour_keys(table, C) != 0][:31]
        for nvox in (4096, 4097, 4098, 4099, 1, 2, 3):
            flat = pal[rng.integers(0, len(pal), nvox)].reshape((nvox,) if C == 1 else (nvox, 3))
            keys = _keys(flat, C)
            want_bm, want_p = ref_presence(keys, _colour_keys(table, C))
            for off in (0, 1, 2, 3):
                bm, p = dev_presence(pb3d_gpu, flat, C, table, off)
                assert np.array_equal(bm, want_bm) and p == want_p, (C, nvox, off)
    nvox = 4 * 64 * 48
    g = np.arange(nvox) // 4
    lane, wave = g % 64, g // 64
    keys = (1 + lane * 4 + np.arange(nvox) % 4 + 256 * (wave % 3)).astype(np.uint32)
    rgb = np.stack([keys & 255, (keys >> 8) & 255, keys >> 16], 1).astype(np.uint8)
    want_bm, _ = ref_presence(keys)
    assert np.count_nonzero(np.unpackbits(want_bm.view(np.uint8))) == 768
    for off in (0, 1):
        assert np.array_equal(dev_presence(pb3d_gpu, rgb, 3, off=off)[0], want_bm), off
    lab = (1 + (lane * 4 + np.arange(nvox) % 4) % 255).astype(np.uint8)
    assert np.array_equal(dev_presence(pb3d_gpu, lab, 1)[0], ref_presence(lab.astype(np.uint32))[0])


@gpu
def test_color_presence_every_colour(pb3d_gpu):
    """each of the 2^24 - 1 non-black colours once, shuffled: every bit but bit 0; with one black voxel added (nvox = 2^24, dword
    loads) and without (nvox = 2^24 - 1, byte loads)"""
    rng = np.random.default_rng(1 << 24)
    keys = rng.permutation(np.arange(1, 1 << 24, dtype=np.uint32))
    want = np.full((1 << 19,), 0xFFFFFFFF, np.uint32)
    want[0] = 0xFFFFFFFE
    for with_black in (True, False):
        k = np.insert(keys, 12345, 0) if with_black else keys
        rgb = np.stack([k & 255, (k >> 8) & 255, k >> 16], 1).astype(np.uint8)
        assert np.array_equal(dev_presence(pb3d_gpu, rgb, 3)[0], want), with_black


@gpu
def test_mask_bits(pb3d_gpu):
    """0 to 31 colours, with and without a grid's bitmap, npix tails; black pixels never get bit 31; a black colour is refused"""
    ev = pb3d_gpu.eval_helpers_intra
    rng = np.random.default_rng(9)
    pal = rng.integers(1, 256, (40, 3)).astype(np.uint8)
    pal[0] = 0
    grid = pal[rng.integers(0, 25, 5000)]               # colours 25.. never occur in the grid
    gkeys = _keys(grid, 3)
    for ncol in (0, 1, 7, 31):
        cols = pal[1:1 + ncol] if ncol < 31 else pal[5:36]
        for npix in (1, 63, 64, 65, 257, 4099):
            mask = pal[rng.integers(0, len(pal), npix)]
            mask[::5] = 0
            for with_bm in (False, True):
                with Bufs(pb3d_gpu) as b:
                    d_m = b.put(mask)
                    d_bm = b.keep(ev.presence_resident(b.put(grid), (len(grid), 1, 1, 3), [])) if with_bm else None
                    got = b.keep(ev.mask_bits_resident(d_m, npix, cols, d_bm)).download((npix,), np.uint32)
                want = ref_mask_bits(mask, cols, gkeys if with_bm else None)
                assert np.array_equal(got, want), (ncol, npix, with_bm)
                assert not (got[::5] >> 31).any() and (with_bm or not (got >> 31).any())
    with Bufs(pb3d_gpu) as b:
        with pytest.raises(ValueError, match="black"):
            ev.mask_bits_resident(b.put(pal), 40, np.array([[1, 2, 3], [0, 0, 0]], np.uint8))


# =====================================================================================================================
# GPU 5: IoU rows
# =====================================================================================================================

def _row_images(rng, npix):
    imgs = [rng.integers(0, 1 << 32, npix, dtype=np.uint64).astype(np.uint32) for _ in range(3)]
    imgs[0][rng.random(npix) < 0.5] = 0                 # sparse images: unions smaller than npix
    imgs[2] &= np.uint32(0x8000000F)
    return imgs


def _rows(n, rng):
    """n rows over images 0, 1, 2 (None: a null buffer) mixing single and multi-bit masks, null pred, null gt, gates, and a row whose
    union is empty (row 5: bits 20 and 21 of image 2 are never set)"""
    kinds = [(0, 1, 1, 1, None, 0), (0, 0xF0, 1, 0x3, 2, 0x1), (None, 0, 1, 1 << 7, None, 0), (0, 1 << 31, None, 0, None, 0),
             (0, 0x5, 1, 0xA, 2, 0x80000000), (2, 1 << 20, 2, 1 << 21, None, 0), (1, 0xFFFFFFFF, 0, 0xFFFFFFFF, 1, 0x100)]
    rows = []
    for r in range(n):
        pi, pm, gi, gm, ki, km = kinds[r % len(kinds)]
        if r >= len(kinds):
            pm, gm = pm and int(rng.integers(1, 1 << 32)), gm and int(rng.integers(1, 1 << 32))
        rows.append((pi, pm, gi, gm, ki, km))
    return rows


def _images_of(row, imgs):
    pi, pm, gi, gm, ki, km = row
    return (None if pi is None else imgs[pi], pm, None if gi is None else imgs[gi], gm, None if ki is None else imgs[ki], km)


@gpu
def test_iou_rows(pb3d_gpu):
    """1, 7 and 32 rows over npix in {0, 1, 63, 64, 65, 257, 2048 * 2049}: counts land at byte 16 of a buffer whose sentinels
    before and after stay; 33 rows are refused"""
    ev = pb3d_gpu.eval_helpers_intra
    rng = np.random.default_rng(32)
    sentinel = np.int64(-0x5A5A5A5A5A5A5A5B)
    for npix in (0, 1, 63, 64, 65, 257, 2048 * 2049):
        imgs = _row_images(rng, max(npix, 1))
        for n in (1, 7, 32):
            rows = _rows(n, rng)
            want = ref_iou_rows([_images_of(r, imgs) for r in rows], npix)
            if n >= 7:
                assert want[5, 1] == 0                  # the empty union
            if npix >= 257 and n >= 7:
                assert (want[:, 0] > 0).sum() >= 3 and (want[:, 1] > want[:, 0]).sum() >= 3
            with Bufs(pb3d_gpu) as b:
                d_imgs = [b.put(x) for x in imgs]
                dev_rows = [_images_of(r, d_imgs) for r in rows]
                d_c = b.empty((2 * n + 4) * 8)
                d_c.upload(np.full(2 * n + 4, sentinel, np.int64))
                ev.iou_rows_resident(dev_rows, npix, d_c, byte_offset=16)
                got = d_c.download((2 * n + 4,), np.int64)
            assert (got[:2] == sentinel).all() and (got[-2:] == sentinel).all(), (npix, n)
            assert np.array_equal(got[2:-2].reshape(n, 2), want), (npix, n)
    with Bufs(pb3d_gpu) as b:
        d = b.put(np.zeros(64, np.uint32))
        with pytest.raises(ValueError, match="at most 32 rows"):
            ev.iou_rows_resident([(d, 1, d, 1, None, 0)] * 33, 64, b.empty(33 * 16))


# =====================================================================================================================
# GPU 6: notebook 4 in exact counts
# =====================================================================================================================

def ref_part_rows(gi, gd, mask, cam, colours, points):
    """the rows of part_minaret_binary_cells (reference :605-738) as integer counts, and the init grid's part-presence bits; points:
    the _grid_points of gi and gd"""
    H, W = mask.shape[:2]
    pi, pd = (ref_grid_project(g, cam, H, W, p) for g, p in zip((gi, gd), points))
    zi, zd = zbuf_of(pi, H, W), zbuf_of(pd, H, W)
    v_ii = bits_of(pi, colours, 3, zi, H, W)
    v_dd = bits_of(pd, colours, 3, zd, H, W)
    v_id = bits_of(pi, colours[len(PARTS):], 3, zd, H, W)
    gkeys = np.unique(points[0][1])
    _, present = ref_presence(gkeys, _colour_keys(colours, 3))
    gt = ref_mask_bits(mask, colours, gkeys)
    rows = []
    for k in range(len(PARTS)):
        rows += [(v_ii, 1 << k, gt, 1 << k, None, 0), (v_dd, 1 << k, gt, 1 << k, None, 0), (None, 0, gt, 1 << k, None, 0)]
    rows += [(v_ii, 3 << 5, gt, 3 << 5, None, 0), (v_id, 3, gt, 3 << 5, None, 0)]
    rows += [(v_ii, ANY, gt, ANY, None, 0), (v_dd, ANY, gt, ANY, None, 0)]
    return ref_iou_rows(rows, H * W), present


def ref_minaret_rows(g, mask, vox, msk, cams, points):
    """the twelve rows of minaret_iou_cells (reference :471-532): per camera, minaret j's visible voxels against its mask pixels,
    gated by the visible pixels of all four"""
    H, W = mask.shape[:2]
    gt = np.zeros((H, W), np.uint32)
    for j, m in enumerate(MINARETS):
        gt |= msk[m].astype(bool).astype(np.uint32) << np.uint32(j)
    rows = []
    for cam in cams:
        vb = ref_points_bits([vox[m] for m in MINARETS], cam, zbuf_of(ref_grid_project(g, cam, H, W, points), H, W), H, W)
        rows += [(vb, 1 << j, gt, 1 << j, vb, 0xF) for j in range(len(MINARETS))]
    return ref_iou_rows(rows, H * W)


def dev_part_rows(pb3d, gi, gd, mask, cam):
    ev, dev = pb3d.eval_helpers_intra, pb3d.device
    bufs = []
    g_i, g_d = dev.DeviceGrid(dev.from_numpy(gi), gi.shape), dev.DeviceGrid(dev.from_numpy(gd), gd.shape)
    try:
        counts, present, _ = ev._part_rows(g_i, g_d, mask, cam, pb3d.PART_COLORS, bufs)
    finally:
        for b in bufs:
            b.free()
        g_i.free()
        g_d.free()
    return counts, present


def dev_minaret_rows(pb3d, g, mask, cams):
    """minaret_iou_cells' device half rebuilt from the resident entries: z-buffer, visible bits of the four int64 minaret sets, one
    row pass"""
    from pb3d.minarets import extract_minaret_masks_by_label, extract_minaret_voxels_by_label
    ev, dev = pb3d.eval_helpers_intra, pb3d.device
    PC = pb3d.PART_COLORS
    colours = [PC["front_minarets"], PC["back_minarets"]]
    H, W = mask.shape[:2]
    grid = dev.DeviceGrid(dev.from_numpy(g), g.shape)
    with Bufs(pb3d) as b:
        try:
            vox = extract_minaret_voxels_by_label(grid, colours)
            msk = extract_minaret_masks_by_label(mask, colours)
            gt = np.zeros((H, W), np.uint32)
            for j, m in enumerate(MINARETS):
                gt |= msk[m].astype(bool).astype(np.uint32) << np.uint32(j)
            d_gt = b.put(gt)
            rows = []
            for cam in cams:
                d_z = b.keep(ev.depth_buffer_resident(grid.buf, g.shape, cam, H, W))
                d_v = b.keep(ev.points_visible_bits_resident([vox[m] for m in MINARETS], cam, d_z, (H, W), H, W))
                rows += [(d_v, 1 << j, d_gt, 1 << j, d_v, 0xF) for j in range(len(MINARETS))]
            d_c = b.empty(len(rows) * 16)
            ev.iou_rows_resident(rows, H * W, d_c)
            return d_c.download((len(rows), 2), np.int64)
        finally:
            grid.free()


@gpu
@pytest.mark.parametrize("mon", MONUMENTS)
def test_notebook4_rows_exact_counts(pb3d_gpu, mon):
    """the counts the notebook-4 table cells are computed from: _part_rows' (inter, union) rows and present bits under the final
    camera, front and drone views, and the twelve gated rows of minaret_iou_cells (init, kp and final cameras) equal the
    restatement's integer counts"""
    from test_intra_eval import _cam, _grid, _resized_mask, ref_minaret_parts
    PC = pb3d_gpu.PART_COLORS
    colours = [PC[p] for p in PARTS] + [PC["front_minarets"], PC["back_minarets"]]
    gi, gd = _grid(mon), _grid(mon, True)
    points = (_grid_points(_keys(gi, 3)), _grid_points(_keys(gd, 3)))
    for view in ("front", "drone"):
        mask = _resized_mask(mon, gi.shape, view)
        cam = _cam(mon, "final", view)
        want, want_present = ref_part_rows(gi, gd, mask, cam, colours, points)
        counts, present = dev_part_rows(pb3d_gpu, gi, gd, mask, cam)
        assert present == want_present and np.array_equal(counts, want), (mon, view)
        assert (want[:, 1] > 0).sum() >= 4
    g, mask, vox, msk = ref_minaret_parts(mon, PC)
    cams = [_cam(mon, t) for t in ("init", "kp", "final")]
    want = ref_minaret_rows(g, mask, vox, msk, cams, points[0])
    assert np.array_equal(dev_minaret_rows(pb3d_gpu, g, mask, cams), want), mon
    assert (want[:, 0] > 0).sum() >= 8
