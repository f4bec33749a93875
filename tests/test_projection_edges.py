"""Edge cases of the projection family (csrc/project.hip, csrc/project_point.h) and of deform_coords (csrc/deform.hip).

The exact reference.  For a camera whose look-at rotation is a signed permutation matrix (views along +-x, +-z and straight
down / up +-y) every product and every sum in (p - cam) @ R.T is exact, so the reference's NumPy code
(utils/projection_utils.py:5-23, utils/eval_helpers_intra.py:134-190) can simply be run as written, with NumPy's own promotion
rules and without the claim the oracle and the kernels share about how the host's BLAS orders or fuses the matmul.  The
helpers below assert that R really is a signed permutation, so they are never used where they would not be exact; general
cameras are compared with the oracle.

The inputs are built so that the decisions random data almost never reaches do happen, and the tests count them before
trusting a comparison: u and v exactly on k + 0.5 (half-to-even rint; -0.5 -> -0 -> pixel 0), depths at the drop and clamp
thresholds, equal and adjacent-ulp depths on one pixel, |z - zbuf| exactly at eps, point lists at 4-byte (not 16-byte)
offsets and of every length mod 4, camera batches over several passes, key images at index bases near 2^32 and 2^39, and
deformations whose float64 values sit exactly on .5.
"""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu

# =====================================================================================================================
# The exact restatement (fresh NumPy, reference semantics)
# =====================================================================================================================


def assert_signed_permutation(R):
    R = np.asarray(R)
    assert R.shape == (3, 3)
    assert np.all((R == 0) | (R == 1) | (R == -1)), R
    assert np.array_equal(np.abs(R).sum(axis=0), [1, 1, 1]) and np.array_equal(np.abs(R).sum(axis=1), [1, 1, 1]), R


def ref_look_at(eye, target):
    """utils/camera_geometry.py:3-14 (same operations and dtypes)"""
    z = target - eye
    z = z / np.linalg.norm(z)
    up = np.array([0, 1, 0], dtype=np.float32)
    if np.allclose(np.abs(np.dot(z, up)), 1.0):
        up = np.array([0, 0, 1], dtype=np.float32)
    x = np.cross(up, z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=0)
    assert_signed_permutation(R)          # the restatement is exact only for these views
    return R


def ref_frame(pts, cam):
    eye, target = np.asarray(cam["cam_pos"]), np.asarray(cam["target"])
    return ((np.asarray(pts) - eye) @ ref_look_at(eye, target).T).T


def ref_uv(pts, cam, drop):
    """u, v (before rounding) and Z of the points the reference keeps.  drop=False: project_colored_voxels (Z clamped at
    1e-8); drop=True: the z-buffer functions (Z <= 1e-6 dropped)."""
    X, Y, Z = ref_frame(pts, cam)
    if drop:
        valid = Z > 1e-6
        X, Y, Z = X[valid], Y[valid], Z[valid]
    else:
        Z = np.where(Z < 1e-8, 1e-8, Z)
    u = (X / Z) * cam["f"] + cam["cx"]
    v = -(Y / Z) * cam["f"] + cam["cy"]
    return u, v, Z


def ref_pixels(u, v, H, W):
    ui = np.round(u).astype(int)
    vi = np.round(v).astype(int)
    return ui, vi, (ui >= 0) & (ui < W) & (vi >= 0) & (vi < H)


def ref_project(pts, cols, cam, H, W):
    u, v, _ = ref_uv(pts, cam, drop=False)
    ui, vi, valid = ref_pixels(u, v, H, W)
    img = np.zeros((H, W, 3), dtype=np.uint8)
    img[vi[valid], ui[valid]] = np.asarray(cols)[valid]          # fancy assignment: the last writer wins
    return img


def ref_depth(pts, cam, H, W):
    u, v, Z = ref_uv(pts, cam, drop=True)
    ui, vi, inside = ref_pixels(u, v, H, W)
    zbuf = np.full((H, W), np.inf, dtype=np.float32)
    for x, y, z in zip(ui[inside], vi[inside], Z[inside]):
        if z < zbuf[y, x]:
            zbuf[y, x] = z
    return zbuf


def ref_visible(pts, cam, zbuf, H, W, eps):
    u, v, Z = ref_uv(pts, cam, drop=True)
    ui, vi, inside = ref_pixels(u, v, H, W)
    mask = np.zeros((H, W), dtype=bool)
    for x, y, z in zip(ui[inside], vi[inside], Z[inside]):
        if abs(z - zbuf[y, x]) < eps:
            mask[y, x] = True
    return mask


def ref_iou_counts(img, seg, colors):
    inter, uni = [], []
    for c in np.asarray(colors):
        a = np.all(img == c, axis=-1)
        b = np.all(seg == c, axis=-1)
        inter.append(np.count_nonzero(a & b))
        uni.append(np.count_nonzero(a | b))
    return np.array(inter, np.int64), np.array(uni, np.int64)


def to_world(pc, cam, dtype=np.float32):
    """world points whose camera-frame coordinates are exactly `pc` (checked)"""
    eye = np.asarray(cam["cam_pos"])
    R = ref_look_at(eye, np.asarray(cam["target"])).astype(np.float64)
    p = np.asarray(pc, np.float64) @ R + eye.astype(np.float64)
    out = p.astype(dtype)
    assert np.array_equal(out.astype(np.float64), p)
    assert np.array_equal(((out - eye.astype(np.float64)) @ R.T), np.asarray(pc, np.float64))
    return out


def index_colours(n):
    """colour of point i encodes i + 1 (r low byte): an image says which point won each pixel"""
    k = np.arange(1, n + 1, dtype=np.int64)
    return np.stack([k & 255, (k >> 8) & 255, (k >> 16) & 255], 1).astype(np.uint8)


def winner_index(img):
    return img[..., 0].astype(np.int64) | (img[..., 1].astype(np.int64) << 8) | (img[..., 2].astype(np.int64) << 16)


def half_count(a):
    a = np.asarray(a, np.float64)
    return int(np.count_nonzero(a - np.floor(a) == 0.5))


# =====================================================================================================================
# Cases (shared by the CPU checks of the restatement and the GPU tests)
# =====================================================================================================================

def axis_views(center, dist, dtype):
    """the six axis-aligned views of `center`: +z, -z, +x, -x, straight down (-y) and straight up (+y)"""
    c = np.asarray(center, dtype)
    out = []
    for axis, sign in ((2, 1), (2, -1), (0, 1), (0, -1), (1, -1), (1, 1)):
        eye = c.copy()
        eye[axis] -= sign * dist
        out.append({"cam_pos": eye, "target": c.copy()})
    return out


SCALARS = {          # f, cx, cy: Python floats are weak scalars; NumPy scalars carry their width into the later stages
    "py": (4.0, 3.0, 2.5),
    "np32": (np.float32(4.0), np.float32(3.0), np.float32(2.5)),
    "np64_f": (np.float64(4.0), 3.0, 2.5),
    "np64_cx": (4.0, np.float64(3.0), 2.5),
}
SHAPES = [(5, 7), (6, 8)]                   # odd and even W: half-even decides whether u = W - 0.5 lands in the last column


def tie_cases():
    """points whose u, v are EXACTLY every multiple of 0.5 in [-2.5, W + 1.5] x [-2.5, H + 1.5], at depths 1, 2, 4, 8
    (f, cx, cy dyadic, depths powers of two: every stage is exact), for three exact views x float32 / float64 cameras x
    the scalar kinds x both widths"""
    out = []
    for dtype in (np.float32, np.float64):
        for view in [axis_views((8, 6, 10), 16, dtype)[k] for k in (0, 3, 4)]:
            for sk, (f, cx, cy) in SCALARS.items():
                for H, W in SHAPES:
                    cam = dict(view, f=f, cx=cx, cy=cy)
                    t = np.arange(-5, 2 * W + 4) / 2.0
                    s = np.arange(-5, 2 * H + 4) / 2.0
                    T, S, Z = (a.ravel() for a in np.meshgrid(t, s, [1.0, 2.0, 4.0, 8.0], indexing="ij"))
                    pc = np.stack([(T - float(cx)) * Z / float(f), -(S - float(cy)) * Z / float(f), Z], 1)
                    pts = to_world(pc, cam)
                    perm = np.random.default_rng(len(out)).permutation(len(pts))
                    out.append({"name": f"{dtype.__name__}-{sk}-{H}x{W}-{len(out)}", "pts": pts[perm], "cam": cam, "H": H, "W": W})
    return out


def origin_cam(dtype, z0=0.0, f=1.0, cx=0.0, cy=0.0):
    """camera at (0, 0, z0) looking along +z: R = I, Z = p_z - z0"""
    return {"cam_pos": np.array([0, 0, z0], dtype), "target": np.array([0, 0, 1], dtype), "f": f, "cx": cx, "cy": cy}


def on_pixels(Z, dtype, W):
    """points with depths Z on distinct pixels (k % W, k // W) of an origin camera with f = 1, cx = cy = 0"""
    Z = np.asarray(Z, dtype)
    k = np.arange(len(Z))
    return np.stack([(k % W).astype(dtype) * Z, -(k // W).astype(dtype) * Z, Z], 1).astype(dtype)


def threshold_cases():
    """depths at the z-buffer drop threshold (Z <= 1e-6, in the camera's width) and at the projection's clamp (Z < 1e-8)"""
    f32, f64 = np.float32, np.float64
    t32 = f32(1e-6)
    z32 = [t32, np.nextafter(t32, f32(1)), np.nextafter(t32, f32(0)), f32(2e-6), f32(1.0)]
    z64 = [1e-6, np.nextafter(1e-6, 1.0), np.nextafter(1e-6, 0.0), float(t32), float(np.nextafter(t32, f32(1))), 1.0]
    c32 = f32(1e-8)
    clamp32 = [c32, np.nextafter(c32, f32(0)), c32 / f32(2), f32(0), f32(-1), np.nextafter(c32, f32(1)), f32(2e-8)]
    clamp64 = [1e-8, np.nextafter(1e-8, 0.0), 0.5e-8, 0.0, -1.0, np.nextafter(1e-8, 1.0), 2e-8]
    W, H = 8, 4
    out = []
    # "edges": depths that must occur, with their count (the threshold itself and its successor in the camera's width)
    e32 = [(t32, 1), (np.nextafter(t32, f32(1)), 1)]
    for name, pts, cam, edges in (
            ("f32cam", on_pixels(z32, f32, W), origin_cam(f32), e32),
            ("f32cam-np64f", on_pixels(z32, f32, W), origin_cam(f32, f=np.float64(1.0)), e32),     # float32 camera, generic kernel
            ("f64cam-f64pts", on_pixels(z64, f64, W), origin_cam(f64), [(1e-6, 1), (np.nextafter(1e-6, 1.0), 1)]),
            ("f64cam-f32pts", on_pixels(z32, f32, W), origin_cam(f64), [(float(t32), 1), (float(np.nextafter(t32, f32(1))), 1)])):
        out.append({"name": name, "pts": pts, "cam": cam, "H": H, "W": W, "kind": "drop", "edges": edges})
    # a float64 camera just in front of z = 0: float32 points at z = 0 have Z == 1e-6 exactly, or its successor
    for z0 in (1e-6, np.nextafter(1e-6, 1.0)):
        pts = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1]], np.float32)
        out.append({"name": f"f64cam-z0=-{z0!r}", "pts": pts, "cam": origin_cam(f64, z0=-z0, f=1e-6), "H": H, "W": W, "kind": "drop",
                    "edges": [(z0, 2)]})
    # clamp: x = col * 1e-8, so a clamped point lands on col and an unclamped Z = 0.5e-8 would land on 2 col
    for name, zs, dt in (("clamp-f32", clamp32, f32), ("clamp-f64", clamp64, f64)):
        zs = np.asarray(zs, dt)
        k = np.arange(len(zs))
        cols = 1 + k % 3
        pts = np.stack([cols.astype(dt) * dt(1e-8), np.zeros(len(zs), dt), zs], 1).astype(dt)
        out.append({"name": name, "pts": pts, "cam": origin_cam(dt), "H": 1, "W": 8, "kind": "clamp"})
        out.append({"name": name + "-f32pts", "pts": pts.astype(f32), "cam": origin_cam(f64), "H": 1, "W": 8, "kind": "clamp"})
    return out


def depth_stack_cases():
    """several points on each pixel: equal depths, adjacent float32 ulps, ascending / descending / shuffled order; for float64
    points also depths closer than a float32 ulp and on float32 rounding ties (the stored value is float32(z))"""
    out = []
    W, H = 6, 3
    two = np.float32(2.0)
    up, dn = np.nextafter(two, np.float32(3)), np.nextafter(two, np.float32(1))
    stacks32 = [[2, 2, 2], [two, up, dn], [dn, two, up], [up, two, dn], [up, up, dn, dn], [8, 4, 2, 1], [1, 2, 4, 8],
                [4, 4, np.nextafter(np.float32(4), np.float32(5)), np.nextafter(np.float32(4), np.float32(3))]]
    e = 2.0 ** -24
    stacks64 = [[2 + e, 2.0, 2 + 3 * e], [2 + 3 * e, 2 + 4 * e, 2 + 2 * e], [2 + e / 64, 2 + e, 2 - e / 2, 2.0],
                [2 + 5 * e, 2 + 3 * e, 2 + 4 * e], [2 - e / 4, 2 - e / 2, 2 - e / 4], [1 + e, 1 + e / 2, 1 + 3 * e / 2]]
    for dt, stacks in ((np.float32, stacks32), (np.float64, stacks64)):
        rows = []
        for k, st in enumerate(stacks):
            col, row = k % W, k // W
            for z in st:
                rows.append([col * z, -row * z, z])
        pts = np.asarray(rows, dt)
        for cdt in ((np.float32, np.float64) if dt is np.float32 else (np.float64,)):
            out.append({"name": f"{dt.__name__}pts-{cdt.__name__}cam", "pts": pts, "cam": origin_cam(cdt), "H": H, "W": W})
    return out


VIS_EPS = {"py1e-3": 1e-3, "np64_1e-3": np.float64(1e-3), "np32_1e-3": np.float32(1e-3), "py2^-10": 2.0 ** -10,
           "np64_2^-10": np.float64(2.0 ** -10)}


def visibility_cases():
    """|z - zbuf| exactly eps (in the width the reference compares in), one ulp under, one ulp over; and a user zbuf with
    +inf, NaN, zeros and values below and above the points"""
    out = []
    W, H = 8, 4
    for ename, eps in VIS_EPS.items():
        for cdt, pdt in ((np.float32, np.float32), (np.float64, np.float64), (np.float64, np.float32)):
            E = pdt(eps)                                          # eps in the points' width
            zs, zb = [], []
            for d in (E, np.nextafter(E, pdt(0)), np.nextafter(E, pdt(1))):
                zs += [d, 2 * d, d, pdt(1)]                       # z = d over 0; z = 2d over d; z = d under 2d; z = 1 over 1 - d
                zb += [0.0, d, 2 * d, pdt(1) - d]
            zs += [pdt(1), pdt(1), pdt(0.5), pdt(0.25), pdt(1)]
            zb += [np.inf, np.nan, 0.25, 0.5, 1.0]
            pts = on_pixels(zs, pdt, W)
            zbuf = np.full((H, W), 7.0, np.float32)
            zbuf.ravel()[:len(zb)] = np.asarray(zb, np.float64).astype(np.float32)
            out.append({"name": f"{ename}-{cdt.__name__}cam-{pdt.__name__}pts", "pts": pts, "cam": origin_cam(cdt), "H": H, "W": W,
                        "zbuf": zbuf, "eps": eps})
    return out


def vis_dz(case):
    """|z - zbuf| of every point that reaches the compare, and eps in the width the reference compares in"""
    u, v, Z = ref_uv(case["pts"], case["cam"], drop=True)
    ui, vi, inside = ref_pixels(u, v, case["H"], case["W"])
    dz = np.array([abs(z - case["zbuf"][y, x]) for x, y, z in zip(ui[inside], vi[inside], Z[inside])])
    return dz, np.result_type(dz.dtype, case["eps"]).type(case["eps"])


# =====================================================================================================================
# Oracle helpers (general cameras)
# =====================================================================================================================

def orc_depth(oracle, pts, cam, H, W):
    p, pf64, R, cp, prec, _ = oracle._pin_args(pts, cam)
    zbuf = np.empty((H, W), np.float32)
    oracle.lib().orc_depth_buffer(p.ctypes.data_as(C.c_void_p), pf64, C.c_int64(len(p)), oracle._dp(R), oracle._dp(cp),
                                  C.c_double(float(cam["f"])), C.c_double(float(cam["cx"])), C.c_double(float(cam["cy"])), prec, int(H),
                                  int(W), zbuf.ctypes.data_as(C.POINTER(C.c_float)))
    return zbuf


def orc_args(cam):
    return cam["cam_pos"], cam["target"], cam["f"], cam["cx"], cam["cy"]


# =====================================================================================================================
# CPU: the restatement against the oracle, and the edges really are in the inputs
# =====================================================================================================================

def test_restatement_ties_equal_oracle(oracle):
    cases = tie_cases()
    assert len(cases) == 48
    for case in cases:
        pts, cam, H, W = case["pts"], case["cam"], case["H"], case["W"]
        cols = index_colours(len(pts))
        u, v, _ = ref_uv(pts, cam, drop=False)
        # every u, v is exactly on the grid of halves, and the three named edges are present
        assert np.array_equal(2 * u, np.round(2 * u)) and np.array_equal(2 * v, np.round(2 * v)), case["name"]
        assert half_count(u) > len(u) // 3 and half_count(v) > len(v) // 3, case["name"]
        for edge in (-0.5, -1.5, W - 0.5):
            assert np.count_nonzero(u == edge) > 0, (case["name"], edge)
        ui, vi, valid = ref_pixels(u, v, H, W)
        at0 = (u == -0.5) & (v == 0.5)
        assert np.all(ui[u == -0.5] == 0) and at0.any() and np.all(valid[at0])                 # -0.5 -> -0 -> column 0
        assert not np.any(valid[u == -1.5])
        assert np.any(valid[u == W - 0.5]) == (W % 2 == 1)                                  # half-even: the last column only for odd W
        want = ref_project(pts, cols, cam, H, W)
        assert np.array_equal(want, oracle.project_colored_voxels(pts, cols, *orc_args(cam), H, W)), case["name"]
        assert np.array_equal(ref_depth(pts, cam, H, W), orc_depth(oracle, pts, cam, H, W)), case["name"]


def test_restatement_thresholds_and_depth_stacks_equal_oracle(oracle):
    for case in threshold_cases() + depth_stack_cases():
        pts, cam, H, W = case["pts"], case["cam"], case["H"], case["W"]
        X, Y, Z = ref_frame(pts, cam)
        for z, count in case.get("edges", []):
            assert np.count_nonzero(Z == z) == count, (case["name"], z)
        if case.get("kind") == "clamp":
            zmin = Z.dtype.type(1e-8)
            assert np.count_nonzero(Z < zmin) >= 3, case["name"]
            u, v, _ = ref_uv(pts, cam, drop=False)
            assert np.all(u[Z < zmin] == X[Z < zmin] / zmin)                   # the clamp is what puts them in the image
            assert np.all(ref_pixels(u, v, H, W)[2][Z < zmin]), case["name"]
        cols = index_colours(len(pts))
        assert np.array_equal(ref_project(pts, cols, cam, H, W), oracle.project_colored_voxels(pts, cols, *orc_args(cam), H, W)), case["name"]
        want = ref_depth(pts, cam, H, W)
        assert np.array_equal(want, orc_depth(oracle, pts, cam, H, W)), case["name"]
        assert np.isfinite(want).any() == (case.get("kind") != "clamp"), case["name"]
    # the float64 stacks really exercise float32 rounding of the stored depth
    st = [c for c in depth_stack_cases() if c["pts"].dtype == np.float64][0]
    Z = ref_frame(st["pts"], st["cam"])[2]
    assert np.count_nonzero(Z.astype(np.float32).astype(np.float64) != Z) >= 8


def test_restatement_visibility_equal_oracle(oracle):
    hits = {}
    for case in visibility_cases():
        pts, cam, H, W = case["pts"], case["cam"], case["H"], case["W"]
        want = ref_visible(pts, cam, case["zbuf"], H, W, case["eps"])
        assert np.array_equal(want, oracle.project_part_visible(pts, cam, case["zbuf"], H, W, case["eps"])), case["name"]
        assert want.any() and not want.all()
        dz, e = vis_dz(case)
        hits[case["name"]] = np.count_nonzero(dz == e)
    # |z - zbuf| == eps exactly, in the width of the compare, wherever the points' width can hold that eps: 2^-10 always, float32(1e-3)
    # when the compare is in float32 or eps is a float32 scalar, 1e-3 itself for float64 points
    for name, n in hits.items():
        if "2^-10" in name or "np32" in name or "float64cam-float64pts" in name or name.startswith("py1e-3-float32cam"):
            assert n >= 1, (name, n)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_general_scalars_equal_oracle(oracle, dtype):
    """Python-float and NumPy-scalar f / cx / cy / eps on the exact views, float32 and float64 cameras"""
    rng = np.random.default_rng(5)
    pts = rng.integers(0, 16, (3000, 3)).astype(np.float32)
    cols = index_colours(len(pts))
    for view in axis_views((8, 8, 8), 24, dtype):
        for f, cx, cy in ((30.0, 12.5, 9.5), (np.float32(30.25), np.float32(12.5), 9.0), (np.float64(29.5), 12.0, np.float64(9.5))):
            cam = dict(view, f=f, cx=cx, cy=cy)
            assert np.array_equal(ref_project(pts, cols, cam, 20, 26), oracle.project_colored_voxels(pts, cols, *orc_args(cam), 20, 26))
            zb = ref_depth(pts, cam, 20, 26)
            assert np.array_equal(zb, orc_depth(oracle, pts, cam, 20, 26))
            for eps in (1e-3, np.float64(1e-3), 0.5, np.float32(0.5)):
                assert np.array_equal(ref_visible(pts[::7], cam, zb, 20, 26, eps), oracle.project_part_visible(pts[::7], cam, zb, 20, 26, eps))


# =====================================================================================================================
# Device wrappers: the C-ABI entries, points at a byte offset inside their allocation
# =====================================================================================================================

class Dev:
    """buffers of one call; every buffer is freed on exit"""

    def __init__(self, pb3d):
        self.pb3d, self.lib, self.ctx = pb3d, pb3d._lib.load(), pb3d._lib.ctx()
        self.bufs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()

    def put(self, a, off=0):
        """a copy of `a` at byte `off` of a buffer that ends right after it (at least 4 bytes past off)"""
        a = np.ascontiguousarray(a)
        b = self.pb3d.device.DeviceBuffer(off + max(a.nbytes, 4))
        self.bufs.append(b)
        if a.nbytes:
            b.upload(a, off)
        return b.at(off)

    def empty(self, nbytes):
        b = self.pb3d.device.DeviceBuffer(nbytes)
        self.bufs.append(b)
        return b

    def check(self, rc):
        self.pb3d._lib.check(rc)


def cam_args(pts, cam):
    from pb3d.projection_utils import camera_args
    p, pf64, R, cp, prec = camera_args(pts, cam["cam_pos"], cam["target"], cam["f"], cam["cx"], cam["cy"])
    return p, pf64, R, cp, prec, (float(cam["f"]), float(cam["cx"]), float(cam["cy"]))


def dev_project(pb3d, pts, cols, cam, H, W, off=0):
    p, pf64, R, cp, prec, fcc = cam_args(pts, cam)
    assert off % 16 == 0 or not pf64
    with Dev(pb3d) as d:
        img = d.empty(H * W * 3)
        d.check(d.lib.pb3d_project_dev(d.ctx, d.put(p, off), pf64, d.put(np.asarray(cols, np.uint8)), len(p), pb3d._lib.p_dbl(R),
                                       pb3d._lib.p_dbl(cp), *fcc, prec, H, W, img.at(0)))
        return img.download((H, W, 3))


def dev_keys(pb3d, pts, cols, base, cam, H, W, off=0):
    p, pf64, R, cp, prec, fcc = cam_args(pts, cam)
    with Dev(pb3d) as d:
        keys = d.empty(H * W * 8)
        d.check(d.lib.pb3d_project_keys_dev(d.ctx, d.put(p, off), pf64, d.put(np.asarray(cols, np.uint8)), len(p), int(base),
                                            pb3d._lib.p_dbl(R), pb3d._lib.p_dbl(cp), *fcc, prec, H, W, keys.at(0)))
        return keys.download((H, W), np.uint64)


def dev_depth(pb3d, pts, cam, H, W, off=0):
    p, pf64, R, cp, prec, fcc = cam_args(pts, cam)
    with Dev(pb3d) as d:
        z = d.empty(H * W * 4)
        d.check(d.lib.pb3d_depth_buffer_dev(d.ctx, d.put(p, off), pf64, len(p), pb3d._lib.p_dbl(R), pb3d._lib.p_dbl(cp), *fcc, prec, H, W,
                                            z.at(0)))
        return z.download((H, W), np.float32)


def dev_visible(pb3d, pts, cam, zbuf, H, W, eps, off=0):
    from pb3d.projection_utils import _promotes_to_f64
    p, pf64, R, cp, prec, fcc = cam_args(pts, cam)
    eps_f32 = int((not prec[0]) and not _promotes_to_f64(eps))
    with Dev(pb3d) as d:
        m = d.empty(H * W)
        d.check(d.lib.pb3d_visible_mask_dev(d.ctx, d.put(p, off), pf64, len(p), pb3d._lib.p_dbl(R), pb3d._lib.p_dbl(cp), *fcc, prec,
                                            d.put(np.ascontiguousarray(zbuf, np.float32)), H, W, float(eps), eps_f32, m.at(0)))
        return m.download((H, W)).astype(bool)


def cam_records(pb3d, pts_dtype, cams):
    rec = np.zeros(len(cams), pb3d.CameraObjective._CAM)
    for k, cam in enumerate(cams):
        _, _, R, cp, prec, (f, cx, cy) = cam_args(np.zeros((1, 3), pts_dtype), cam)
        rec["R"][k] = R.reshape(9); rec["cam"][k] = cp
        rec["f"][k] = f; rec["cx"][k] = cx; rec["cy"][k] = cy; rec["prec"][k] = list(prec)
    return rec


def dev_batch(pb3d, pts, cols, cams, seg, colors, off=0):
    """pb3d_project_iou_batch_dev: (K, P) inter and union counts"""
    pts = np.ascontiguousarray(pts)
    H, W = seg.shape[:2]
    colors = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
    rec = cam_records(pb3d, pts.dtype, cams)
    inter = np.full((len(cams), len(colors)), -1, np.int64); uni = inter.copy()
    with Dev(pb3d) as d:
        d.check(d.lib.pb3d_project_iou_batch_dev(d.ctx, d.put(pts, off), int(pts.dtype == np.float64), d.put(np.asarray(cols, np.uint8)),
                                                 len(pts), rec.ctypes.data_as(C.c_void_p), len(cams), H, W, d.put(seg), pb3d._lib.p_u8(colors),
                                                 len(colors), inter.ctypes.data_as(pb3d._lib.i64p), uni.ctypes.data_as(pb3d._lib.i64p)))
    return inter, uni


def dev_single_counts(pb3d, pts, cols, cam, seg, colors):
    """the one-camera route: pb3d_project_dev into a device image, then pb3d_partwise_iou_dev against the part image"""
    p, pf64, R, cp, prec, fcc = cam_args(pts, cam)
    H, W = seg.shape[:2]
    colors = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
    inter = np.full(len(colors), -1, np.int64); uni = inter.copy()
    with Dev(pb3d) as d:
        img = d.empty(H * W * 3)
        d.check(d.lib.pb3d_project_dev(d.ctx, d.put(p), pf64, d.put(np.asarray(cols, np.uint8)), len(p), pb3d._lib.p_dbl(R),
                                       pb3d._lib.p_dbl(cp), *fcc, prec, H, W, img.at(0)))
        d.check(d.lib.pb3d_partwise_iou_dev(d.ctx, img.at(0), d.put(seg), H * W, pb3d._lib.p_u8(colors), len(colors),
                                            inter.ctypes.data_as(pb3d._lib.i64p), uni.ctypes.data_as(pb3d._lib.i64p)))
    return inter, uni


# =====================================================================================================================
# GPU: ties and thresholds, both kernel forms
# =====================================================================================================================

@gpu
def test_ties_project_keys_depth(pb3d_gpu):
    """u, v exactly on k + 0.5 through the float32 kernels (float32 camera, weak or float32 scalars) and the generic kernel
    (float64 camera, or a float64 NumPy scalar): image, key image, depth buffer and visibility all equal the restatement"""
    from pb3d import dist
    kinds = set()
    for case in tie_cases():
        pts, cam, H, W = case["pts"], case["cam"], case["H"], case["W"]
        cols = index_colours(len(pts))
        want = ref_project(pts, cols, cam, H, W)
        assert np.array_equal(pb3d_gpu.project_colored_voxels(pts, cols, *orc_args(cam), H, W), want), case["name"]
        assert np.array_equal(dev_project(pb3d_gpu, pts, cols, cam, H, W), want), case["name"]
        img, keys = dist.project_colored_voxels_sharded(pts, cols, 7, *orc_args(cam), H, W, reduce=False)
        w = winner_index(want).astype(np.uint64)
        assert np.array_equal(img, want) and np.array_equal(keys, np.where(w > 0, ((w + np.uint64(7)) << np.uint64(24)) | w, 0)), case["name"]
        zb = ref_depth(pts, cam, H, W)
        assert np.array_equal(dev_depth(pb3d_gpu, pts, cam, H, W), zb), case["name"]
        vis = ref_visible(pts[::3], cam, zb, H, W, 1e-3)
        assert vis.any() and np.array_equal(pb3d_gpu.project_part_visible(pts[::3], cam, zb, H, W), vis), case["name"]
        _, _, _, _, prec, _ = cam_args(pts, cam)
        kinds.add(tuple(prec))
    assert (0, 0, 0, 0) in kinds and (1, 1, 1, 1) in kinds and (0, 1, 1, 1) in kinds and (0, 0, 1, 0) in kinds


@gpu
def test_thresholds_and_depth_stacks(pb3d_gpu):
    """Z at float32(1e-6) / 1e-6 and their neighbours (dropped / kept), Z around the 1e-8 clamp, and stacks of equal,
    adjacent-ulp and sub-float32 depths on one pixel in every order: the sequential `if z < zbuf` loop of the reference"""
    for case in threshold_cases() + depth_stack_cases():
        pts, cam, H, W = case["pts"], case["cam"], case["H"], case["W"]
        cols = index_colours(len(pts))
        want = ref_project(pts, cols, cam, H, W)
        assert np.array_equal(dev_project(pb3d_gpu, pts, cols, cam, H, W), want), case["name"]
        zb = ref_depth(pts, cam, H, W)
        assert np.array_equal(dev_depth(pb3d_gpu, pts, cam, H, W), zb), case["name"]
        assert np.array_equal(pb3d_gpu.project_part_visible(pts, cam, zb, H, W), ref_visible(pts, cam, zb, H, W, 1e-3)), case["name"]


@gpu
def test_visibility_at_eps(pb3d_gpu):
    """|z - zbuf| == eps, one ulp under and one over, with weak (Python) and NumPy eps of both widths; zbuf with +inf, NaN,
    zeros and values on both sides of the points"""
    for case in visibility_cases():
        pts, cam, H, W = case["pts"], case["cam"], case["H"], case["W"]
        want = ref_visible(pts, cam, case["zbuf"], H, W, case["eps"])
        assert np.array_equal(pb3d_gpu.project_part_visible(pts, cam, case["zbuf"], H, W, case["eps"]), want), case["name"]
        assert np.array_equal(dev_visible(pb3d_gpu, pts, cam, case["zbuf"], H, W, case["eps"]), want), case["name"]


# =====================================================================================================================
# GPU: unaligned and ragged point lists through the C-ABI
# =====================================================================================================================

NS = list(range(10)) + [10001, 10002, 10003]
OFFSETS = (0, 4, 8, 12, 16)          # 4, 8, 12: the float32 kernels' scalar-load branch (vec = 0)


def offset_inputs():
    rng = np.random.default_rng(12)
    n = max(NS)
    # exact view + points on pixel centres (all land); general camera + a box of points in front of it
    ex = dict(axis_views((8, 6, 10), 16, np.float32)[0], f=4.0, cx=20.0, cy=15.0)
    T, S = rng.integers(0, 40, n), rng.integers(0, 30, n)
    Z = 2.0 ** rng.integers(0, 4, n)
    ex_pts = to_world(np.stack([(T - 20.0) * Z / 4, -(S - 15.0) * Z / 4, Z], 1), ex)
    gen = {"cam_pos": np.array([1.5, -2.25, -30], np.float32), "target": np.array([0.5, 0.25, 4], np.float32), "f": 61.7, "cx": 20.25,
           "cy": 14.5}
    gen_pts = rng.uniform(-6, 6, (n, 3)).astype(np.float32)
    return [("exact", ex, ex_pts), ("general", gen, gen_pts)]


@gpu
def test_unaligned_ragged_point_lists(pb3d_gpu, oracle):
    """the five float32-point entries with the point list at byte offsets 0..16 of its allocation and n = 0..9 and 10001..10003:
    every result equals the offset-0 result and the oracle (or the restatement for the exact view), in both kernel forms"""
    H, W = 30, 40
    rng = np.random.default_rng(3)
    palette = np.array(list(pb3d_gpu.PART_COLORS.values())[:5], np.uint8)
    seg = palette[rng.integers(0, 5, (H, W))]
    for label, cam32, pts_all in offset_inputs():
        for cdt in (np.float32, np.float64):
            cam = dict(cam32, cam_pos=cam32["cam_pos"].astype(cdt), target=cam32["target"].astype(cdt))
            for n in NS:
                pts = np.ascontiguousarray(pts_all[:n])
                cols = index_colours(n)
                pal_cols = palette[np.arange(n) % 5]
                img = oracle.project_colored_voxels(pts, cols, *orc_args(cam), H, W)
                zb = orc_depth(oracle, pts, cam, H, W)
                vis = oracle.project_part_visible(pts, cam, zb, H, W)
                if label == "exact":
                    assert np.array_equal(img, ref_project(pts, cols, cam, H, W)) and np.array_equal(zb, ref_depth(pts, cam, H, W))
                    assert np.array_equal(vis, ref_visible(pts, cam, zb, H, W, 1e-3))
                if label == "exact":
                    assert ref_pixels(*ref_uv(pts, cam, drop=True)[:2], H, W)[2].all()     # every point lands (the ragged tail's too)
                w = winner_index(img).astype(np.uint64)
                base = 2 ** 33 + 5
                keys = np.where(w > 0, ((w + np.uint64(base)) << np.uint64(24)) | w, 0)
                cams = [cam, dict(cam, f=cam["f"] * 1.25, cx=cam["cx"] - 3)]
                counts = [oracle.partwise_iou_counts(oracle.project_colored_voxels(pts, pal_cols, *orc_args(c), H, W), seg, palette) for c in cams]
                for off in OFFSETS:
                    what = (label, cdt.__name__, n, off)
                    assert np.array_equal(dev_project(pb3d_gpu, pts, cols, cam, H, W, off), img), what
                    assert np.array_equal(dev_keys(pb3d_gpu, pts, cols, base, cam, H, W, off), keys), what
                    assert np.array_equal(dev_depth(pb3d_gpu, pts, cam, H, W, off), zb), what
                    assert np.array_equal(dev_visible(pb3d_gpu, pts, cam, zb, H, W, 1e-3, off), vis), what
                    inter, uni = dev_batch(pb3d_gpu, pts, pal_cols, cams, seg, palette, off)
                    assert np.array_equal(inter, np.stack([c[0] for c in counts])) and np.array_equal(uni, np.stack([c[1] for c in counts])), what


# =====================================================================================================================
# GPU: camera batches over several passes
# =====================================================================================================================

@gpu
def test_camera_batch_three_passes(pb3d_gpu, oracle):
    """70 cameras on a 2048 x 2048 part image: passes of 32 (float32 kernel), 32 (float64 cameras -> generic kernel) and 6
    (float32 kernel).  Every camera's counts equal the one-camera route; the exact views equal the restatement."""
    H = W = 2048
    assert (512 << 20) // (H * W * 4) == 32                     # cameras per pass of pb3d_project_iou_batch_dev
    rng = np.random.default_rng(2048)
    N = 200003
    pts = rng.integers(0, 64, (N, 3)).astype(np.float32)
    palette = np.array(list(pb3d_gpu.PART_COLORS.values())[:6], np.uint8)
    cols = palette[rng.integers(0, 6, N)]
    center = np.array([32, 32, 32], np.float32)
    views = axis_views(center, 96, np.float32)
    seg = ref_project(pts, cols, dict(views[0], f=1500.0, cx=1024.0, cy=1024.0), H, W)
    cams, exact = [], {5: 0, 37: 2, 45: 4, 66: 5}
    for k in range(70):
        if k in exact:
            cam = dict(views[exact[k]], f=1500.0 + k, cx=1024.0, cy=1020.5)
        else:
            d = rng.normal(size=3)
            d = d / np.linalg.norm(d)
            cam = {"cam_pos": (center + 90 * d).astype(np.float32), "target": (center + rng.normal(size=3)).astype(np.float32),
                   "f": float(1400 + 200 * rng.random()), "cx": float(1024 + rng.normal()), "cy": float(1024 + rng.normal())}
        cams.append(cam)
    cams[45] = dict(cams[45], cam_pos=cams[45]["cam_pos"].astype(np.float64), target=cams[45]["target"].astype(np.float64))
    cams[40] = dict(cams[40], cam_pos=cams[40]["cam_pos"].astype(np.float64), target=cams[40]["target"].astype(np.float64))
    cams[50] = dict(cams[50], f=np.float64(cams[50]["f"]))
    generic = [k for k, c in enumerate(cams) if any(cam_args(pts[:1], c)[4])]
    assert generic == [40, 45, 50]                                # the float64 cameras are all in the middle pass
    inter, uni = dev_batch(pb3d_gpu, pts, cols, cams, seg, palette)
    assert (uni > 0).any(axis=1).all() and (inter > 0).sum() > 20
    for k, cam in enumerate(cams):
        si, su = dev_single_counts(pb3d_gpu, pts, cols, cam, seg, palette)
        assert np.array_equal(inter[k], si) and np.array_equal(uni[k], su), k
    for k in exact:
        ri, ru = ref_iou_counts(ref_project(pts, cols, cams[k], H, W), seg, palette)
        assert np.array_equal(inter[k], ri) and np.array_equal(uni[k], ru), k
    for k in (12, 40, 50):
        oi, ou = oracle.partwise_iou_counts(oracle.project_colored_voxels(pts, cols, *orc_args(cams[k]), H, W), seg, palette)
        assert np.array_equal(inter[k], oi) and np.array_equal(uni[k], ou), k


@gpu
@pytest.mark.parametrize("W", [(1 << 24) - 1, 1 << 24])
def test_fast_path_image_width_limit(pb3d_gpu, oracle, W):
    """W = 2^24 - 1 is the widest image of the float32 kernels, W = 2^24 goes to the generic kernel; points land in and
    just past the last columns"""
    cam = dict(origin_cam(np.float32), cx=float(W - 3))
    X = np.arange(-3, 6, dtype=np.float32)
    pts = np.stack([X, np.zeros_like(X), np.ones_like(X)], 1)
    cols = index_colours(len(pts))
    want = ref_project(pts, cols, cam, 1, W)
    assert want[0, W - 1].any() and np.count_nonzero(winner_index(want)) == 6
    assert np.array_equal(oracle.project_colored_voxels(pts, cols, *orc_args(cam), 1, W), want)
    assert np.array_equal(dev_project(pb3d_gpu, pts, cols, cam, 1, W), want)
    inter, uni = dev_batch(pb3d_gpu, pts, cols, [cam, dict(cam, cx=float(W - 5))], want, cols)
    ri, ru = ref_iou_counts(ref_project(pts, cols, dict(cam, cx=float(W - 5)), 1, W), want, cols)
    assert np.array_equal(inter[0], [np.count_nonzero(winner_index(want) == i + 1) for i in range(len(pts))])
    assert np.array_equal(uni[0], inter[0]) and np.array_equal(inter[1], ri) and np.array_equal(uni[1], ru)


# =====================================================================================================================
# GPU: key images at large index bases
# =====================================================================================================================

@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_keys_large_index_bases(pb3d_gpu, oracle, dtype):
    """sharded key images with index_base near 2^32 (the indices cross it) and up to 2^39 - 1: merged by max and resolved,
    they equal the unsharded image, and every key holds (index + 1, colour) of the pixel's winner; index_base + n >= 2^39 is
    refused before anything is written"""
    from pb3d import dist
    from pb3d.projection_utils import camera_args
    rng = np.random.default_rng(39)
    n, H, W = 3001, 40, 56
    pts = rng.integers(-8, 9, (n, 3)).astype(np.float32)          # many points per pixel
    cols = index_colours(n)
    cam = {"cam_pos": np.array([1.5, -2.25, -30], dtype), "target": np.array([0.5, 0.25, 4], dtype), "f": 70.3, "cx": 28.25, "cy": 19.5}
    want = oracle.project_colored_voxels(pts, cols, *orc_args(cam), H, W)
    w = winner_index(want).astype(np.uint64)
    assert np.count_nonzero(w) > 300
    for base in (2 ** 32 - 1500, 2 ** 32, 2 ** 39 - n - 1):
        keys = np.where(w > 0, ((w + np.uint64(base)) << np.uint64(24)) | w, 0)
        merged = np.zeros((H, W), np.uint64)
        for r in range(3):
            i0, i1 = dist.point_shard_bounds(n, r, 3)
            _, k_r = dist.project_colored_voxels_sharded(pts[i0:i1], cols[i0:i1], base + i0, *orc_args(cam), H, W, reduce=False)
            merged = np.maximum(merged, k_r)
        assert np.array_equal(dist.resolve_keys(merged), want) and np.array_equal(merged, keys), base
        img, k_all = dist.project_colored_voxels_sharded(pts, cols, base, *orc_args(cam), H, W, reduce=False)
        assert np.array_equal(img, want) and np.array_equal(k_all, keys), base
    with pytest.raises(ValueError):
        dist.project_colored_voxels_sharded(pts, cols, 2 ** 39 - n, *orc_args(cam), H, W, reduce=False)
    p, pf64, R, cp, prec = camera_args(pts, cam["cam_pos"], cam["target"], cam["f"], cam["cx"], cam["cy"])
    sentinel = np.full((H, W), 0xA5A5A5A5A5A5A5A5, np.uint64)
    with Dev(pb3d_gpu) as d:
        kb = d.empty(H * W * 8)
        kb.upload(sentinel)
        for base in (2 ** 39 - n, 2 ** 39):
            rc = d.lib.pb3d_project_keys_dev(d.ctx, d.put(p), pf64, d.put(cols), n, base, pb3d_gpu._lib.p_dbl(R), pb3d_gpu._lib.p_dbl(cp),
                                             float(cam["f"]), float(cam["cx"]), float(cam["cy"]), prec, H, W, kb.at(0))
            assert rc == -1
        pb3d_gpu.device.sync()
        assert np.array_equal(kb.download((H, W), np.uint64), sentinel)


# =====================================================================================================================
# Deformation ties (csrc/deform.hip)
# =====================================================================================================================

JITTER = np.array([[0, 0, 0], [0.25, 0, 0], [-0.25, 0, 0], [0, 0.25, 0], [0, -0.25, 0], [0, 0, 0.25], [0, 0, -0.25]])


def ref_deform_passes(coords, image_shape, voxel_shape, deform):
    """one_pass() of utils/deformation_estimation.py:70-98 for the seven jitters: (value before rounding, centred value)"""
    out = []
    for offset in JITTER:
        c = coords + offset
        center = c.mean(axis=0, keepdims=True)
        c = c - center
        centred = c.copy()
        H_img, W_img = image_shape
        D, H, W = voxel_shape
        pix2vox_x = W / float(W_img)
        pix2vox_y = H / float(H_img)
        pix2vox_z = D / float(W_img)
        c[:, 0] = c[:, 0] * deform["scale_xz"] + deform["shift_xz"] * pix2vox_x * np.sign(c[:, 0])
        c[:, 1] = c[:, 1] * deform["scale_y"] - deform["shift_y"] * pix2vox_y
        c[:, 2] = c[:, 2] * deform["scale_xz"] + deform["shift_xz"] * pix2vox_z * np.sign(c[:, 2])
        out.append((c + center, centred))
    return out


def ref_deform(coords, image_shape, voxel_shape, deform):
    passes = ref_deform_passes(coords, image_shape, voxel_shape, deform)
    return np.unique(np.vstack([np.round(v).astype(int) for v, _ in passes]), axis=0)


def deform_point_sets():
    """power-of-two sizes: every mean is dyadic, so the float64 pipeline is exact and .5 ties survive to the rounding"""
    rng = np.random.default_rng(64)
    v = [0, 2, 2, 4]
    cube = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)             # mean (2, 2, 2)
    half = rng.integers(0, 9, (512, 3))
    half[:8] = 4
    big = np.concatenate([half, 8 - half])[rng.permutation(1024)]          # mean exactly (4, 4, 4), sixteen points on it
    sets = {1: [[0, 0, 1]], 2: [[1, 0, 2], [1, 3, 4]], 4: [[2, 2, 2], [2, 2, 2], [1, 3, 0], [3, 1, 4]], 64: cube, 1024: big}
    return {k: np.asarray(v, np.float32) for k, v in sets.items()}


DEFORM_SHAPES = [((32, 32), (32, 32, 32)), ((64, 64), (32, 32, 32))]       # pix2vox 1 and 0.5


def deform_tuples():
    out = []
    for sxz in (0.5, 1, 1.5, 2.5):
        for sy in (0.5, 1, 1.5, 2.5):
            for shift_xz, shift_y in ((0.0, 0.0), (0.5, -1.5), (-2.5, 1.0)):
                out.append({"scale_xz": sxz, "scale_y": sy, "shift_xz": shift_xz, "shift_y": shift_y})
    return out


def test_restatement_deform_ties_equal_oracle(oracle):
    for n, pts in deform_point_sets().items():
        ties = zero_sign = negative = 0
        for image_shape, voxel_shape in DEFORM_SHAPES:
            for d in deform_tuples():
                passes = ref_deform_passes(pts, image_shape, voxel_shape, d)
                ties += sum(half_count(v) for v, _ in passes)
                zero_sign += sum(int(np.count_nonzero(c[:, [0, 2]] == 0)) for _, c in passes)
                want = ref_deform(pts, image_shape, voxel_shape, d)
                negative += int((want < 0).any())
                assert np.array_equal(want, oracle.deform_coords(pts, image_shape, voxel_shape, d)), (n, image_shape, d)
        assert ties > 0 and zero_sign > 0 and negative > 0, (n, ties, zero_sign, negative)


@gpu
def test_deform_ties(pb3d_gpu):
    for n, pts in deform_point_sets().items():
        for image_shape, voxel_shape in DEFORM_SHAPES:
            for d in deform_tuples():
                want = ref_deform(pts, image_shape, voxel_shape, d)
                assert np.array_equal(pb3d_gpu.deform_coords(pts, image_shape, voxel_shape, d), want), (n, image_shape, d)


@gpu
def test_deform_ties_batched_equals_one_at_a_time(pb3d_gpu, oracle):
    """the tie-heavy tuples through evaluate_part_deform_batch == evaluate_part_deform per tuple (and the oracle on a few)"""
    PC = pb3d_gpu.PART_COLORS
    grid = np.zeros((32, 32, 32, 3), np.uint8)
    grid[10:14, 12:16, 8:12] = PC["dome"]               # 64 voxels
    grid[4:12, 16:24, 16:32] = PC["plinth"]             # 1024 voxels
    labels = {"dome": PC["dome"], "plinth": PC["plinth"]}
    for (Hi, Wi), _ in DEFORM_SHAPES:
        cam = {"cam_pos": np.array([16, 16, -40], np.float32), "target": np.array([16, 16, 16], np.float32), "f": 1.25 * Wi, "cx": Wi / 2,
               "cy": Hi / 2}
        pts, cols = pb3d_gpu.get_voxel_points_by_parts(grid, labels, list(labels))
        image = pb3d_gpu.project_colored_voxels(pts, cols, *orc_args(cam), Hi, Wi)
        for part in labels:
            deforms = deform_tuples()
            ious, nvalid = pb3d_gpu.evaluate_part_deform_batch(grid, labels, part, deforms, image, cam)
            assert (nvalid > 0).all() and len(set(ious)) > 3
            for k, d in enumerate(deforms):
                assert ious[k] == pb3d_gpu.evaluate_part_deform(grid, labels, part, d, image, cam)[1], (part, d)
            for d in deforms[::11]:
                assert ious[deforms.index(d)] == oracle.evaluate_part_deform(grid, labels, part, d, image, cam)[1], (part, d)
