"""Constructed inputs for the connected-component labelling (csrc/ccl.hip): plain NumPy, no GPU.

Every builder returns a list of cases (name, grid, colours, channels): grid is RGB (A0, A1, A2, 3) uint8 with `colours` a list of
uint8[3] for channels = 3, or a 1-byte label volume (A0, A1, A2) with `colours` a list of ints for channels = 1.  A few voxels of
colours that are not asked for are sprinkled over the background of every case.  CLAIMS[name] says, from the construction alone, what
the case is meant to hold (component counts, a run over a chunk edge, windows with 8 and 9 segments, ...): the CPU tests of
tests/test_ccl_topologies.py check every claim against scipy.ndimage.label and the window arithmetic below, so a builder that
degenerates fails there, before any kernel runs.

Vocabulary of the kernels (labelling): a row is cut into 64-voxel WINDOWS, a window's maximal runs are its SEGMENTS (the
union-find nodes), k_ccl_init takes a row in CHUNKS of 1024 voxels (16 windows) and carries the open run across, a window is
PASS-THROUGH when its only segment continues the run of the window before."""
import numpy as np

# colour 0 = background, 1..8 = the colours a case may ask for, 9 and 10 = sprinkled colours nobody asks for
PALETTE = np.array([[0, 0, 0], [253, 248, 96], [0, 0, 255], [255, 120, 230], [1, 220, 5], [63, 138, 173], [190, 0, 255], [180, 140, 255],
                    [9, 9, 9], [5, 223, 223], [200, 10, 30]], np.uint8)
VALUES = np.array([0, 1, 2, 3, 4, 5, 6, 7, 200, 9, 255], np.uint8)
MAX_VOXELS = 300000
CLAIMS = {}


def _emit(name, lab, K=1, claims=None, channels=(3,)):
    """cases of a volume of colour indices (0 = background, 1..K = members): sprinkles, then one case per channel count"""
    lab = np.ascontiguousarray(lab, np.uint8)
    assert lab.ndim == 3 and lab.size <= MAX_VOXELS, (name, lab.shape)
    assert claims, name
    free = np.flatnonzero(lab.ravel() == 0)
    lab = lab.copy()
    lab.ravel()[free[5::61]] = 9
    lab.ravel()[free[17::113]] = 10
    out = []
    for ch in channels:
        full = f"{name}/{'rgb' if ch == 3 else 'lab'}"
        assert full not in CLAIMS or CLAIMS[full] == claims, full
        CLAIMS[full] = claims
        if ch == 3:
            out.append((full, PALETTE[lab], [PALETTE[k].copy() for k in range(1, K + 1)], 3))
        else:
            out.append((full, VALUES[lab], [int(VALUES[k]) for k in range(1, K + 1)], 1))
    return out


def masks(case):
    """the membership mask of every colour of a case"""
    _, grid, colours, channels = case
    return [grid == c if channels == 1 else np.all(grid == np.asarray(c, np.uint8), axis=-1) for c in colours]


# ---- window arithmetic of a mask, as the kernels see it ---------------------------------------------------------------------------
def windows(mask):
    """(rows, P, 64) bool: the 64-voxel windows of every row, padded with zeros past A2"""
    A2 = mask.shape[2]
    P = (A2 + 63) // 64
    w = np.zeros((mask.shape[0] * mask.shape[1], P * 64), bool)
    w[:, :A2] = mask.reshape(-1, A2)
    return w.reshape(-1, P, 64)


def segments_per_window(mask):
    """(rows, P): the number of segments (maximal runs inside the window) of every window"""
    w = windows(mask)
    starts = w.copy()
    starts[:, :, 1:] &= ~w[:, :, :-1]
    return starts.sum(2)


def passthrough_windows(mask):
    """(rows, P) bool: windows whose only segment starts at bit 0 and continues the run of the window before"""
    w = windows(mask)
    cont = np.zeros(w.shape[:2], bool)
    cont[:, 1:] = w[:, 1:, 0] & w[:, :-1, 63]
    return cont & (segments_per_window(mask) == 1)


def run_start_windows(mask):
    """flat indices (row * P + t) of the windows that hold the first voxel of a run"""
    w = windows(mask)
    flat = w.reshape(w.shape[0], -1)
    st = flat.copy()
    st[:, 1:] &= ~flat[:, :-1]
    return np.flatnonzero(st.reshape(w.shape).any(2).ravel())


def implied_links(mask):
    """The plane-to-plane overlaps (x, r >= 1, run of m[x, r] & m[x+1, r]) whose row above holds members in both planes inside the
    overlap: `same` counts those with such a voxel in the window of the overlap's first voxel, `other` those with one in a later
    window only; `overlaps` counts every plane-to-plane overlap run (row 0 included)."""
    same = other = overlaps = 0
    A0, A1, A2 = mask.shape
    for x in range(A0 - 1):
        for r in range(A1):
            cc = mask[x, r] & mask[x + 1, r]
            if not cc.any():
                continue
            edges = np.flatnonzero(np.diff(np.concatenate([[0], cc.view(np.int8), [0]])))
            for f, e in zip(edges[::2], edges[1::2]):
                overlaps += 1
                if r == 0:
                    continue
                z = f + np.flatnonzero(mask[x, r - 1, f:e] & mask[x + 1, r - 1, f:e])
                if z.size and (z // 64 == f // 64).any():
                    same += 1
                elif z.size:
                    other += 1
    return {"same": same, "other": other, "overlaps": overlaps}


def _rts(P):
    """the rows per plane-to-plane tile (RT) that ccl_tilecols = 0 (32 columns), 2, 8 and 64 give for rows of P windows"""
    return [max(1, min(mc, 64) // P - 1) for mc in (32, 2, 8, 64)]


# ---- 1. long rows: runs over the 1024-voxel chunk edges of k_ccl_init, rows of 17..32 windows under the tile merge --------------------
EDGES = (1024, 2048, 3072)
LONG_A2 = (1025, 1087, 1088, 1089, 1536, 2047, 2048, 2049, 2112, 3073, 4100)
LONG_PAIRS = (("full", "edge2"), ("gap", "cross"), ("hole", "cross_pt"), ("inner", "bit63"))


def _run(row, lo, hi, value=1):
    """row[lo .. hi] (inclusive), clipped to the row"""
    lo, hi = max(lo, 0), min(hi, row.shape[0] - 1)
    if lo <= hi:
        row[lo:hi + 1] = value


def _kind_row(kind, A2):
    row = np.zeros(A2, np.uint8)
    if kind == "full":
        row[:] = 1
    elif kind == "inner":
        row[1:A2 - 1] = 1
    elif kind == "hole":                                         # a gap at exactly the edge, runs on both sides of it
        row[:] = 1
        for E in EDGES:
            if E < A2:
                row[E] = 0
    else:
        for E in EDGES:
            if E > A2 - 1:
                continue
            if kind == "edge2":
                _run(row, E - 1, E)
            elif kind == "gap":                                  # ends at E - 1, the next run starts at E + 1
                _run(row, E - 40, E - 1); _run(row, E + 1, E + 30)
            elif kind == "cross":                                # [960, 1100]: the window after the edge is pass-through
                _run(row, E - 64, E + 76)
            elif kind == "cross_pt":                             # ... and the chunk's last window too
                _run(row, E - 124, E + 76)
            elif kind == "bit63":                                # starts at bit 63 of the chunk's last window
                _run(row, E - 1, E + 76)
    return row


def long_rows():
    """(3, 4, A2): the two kinds of a pair in rows (1, 1) and (1, 3); their neighbour rows and planes hold short runs that overlap
    them only inside the window after each edge, so every face link there must name the segment the carry gave its parent to"""
    out = []
    for A2 in LONG_A2:
        edges = [E for E in EDGES if E <= A2 - 1]
        for k1, k2 in LONG_PAIRS:
            lab = np.zeros((3, 4, A2), np.uint8)
            lab[1, 1] = _kind_row(k1, A2)
            lab[1, 3] = _kind_row(k2, A2)
            for E in edges:
                for (a0, a1), lo in (((1, 0), 3), ((0, 1), 3), ((2, 1), 9), ((1, 2), 9), ((0, 3), 15), ((2, 3), 20)):
                    _run(lab[a0, a1], E + lo, E + lo + 2)
            _run(lab[0, 0], 0, 5); _run(lab[2, 2], A2 - 3, A2 - 1)
            ft = {"edge2": [], "gap": [], "hole": [], "full": [E // 64 for E in edges], "inner": [E // 64 for E in edges if E <= A2 - 2],
                  "cross": [E // 64 for E in edges], "bit63": [E // 64 for E in edges], "cross_pt": [E // 64 - 1 for E in edges] + [E // 64 for E in edges]}
            claims = {"edges": edges, "ft": sorted(set(ft[k1] + ft[k2])), "chunk_through": k1 in ("full", "inner") and A2 >= 2048}
            out += _emit(f"long/{A2}/{k1}+{k2}", lab, 1, claims, channels=(3, 1))
    return out


def long_rows_multi():
    """K colours in blocks that abut at 1023 | 1024 (and 2048, 3072) with no gap: the carries are per colour"""
    out = []
    combos = [(A2, (2, 3, 5, 8)[i % 4]) for i, A2 in enumerate(LONG_A2)] + [(A2, K) for A2 in (3073, 4100) for K in (2, 3, 5, 8)]
    for A2, K in sorted(set(combos)):
        bounds = [b for b in (0, 700, 1024, 1025, 1100, 1900, 2048, 2050, 3000, 3072, 3500) if b < A2] + [A2]
        lab = np.zeros((3, 4, A2), np.uint8)
        for r in range(12):
            for j in range(len(bounds) - 1):
                lab[r // 4, r % 4, bounds[j]:bounds[j + 1]] = (r // 2 + j) % (K + 1)
        claims = {"abut": [E for E in EDGES if E <= A2 - 1]}
        if A2 >= 3073:      # colour 1 in chunks 0 and 2 of a row, absent from all of chunk 1
            lab[2, 3] = 0
            _run(lab[2, 3], 900, 1023, 1); _run(lab[2, 3], 1024, 2047, 2); _run(lab[2, 3], 2048, 2100, 1)
            claims["absent_chunk"] = True
        out += _emit(f"longmulti/{A2}/K{K}", lab, K, claims, channels=(3, 1))
    return out


# ---- 2. rows per wave: k_ccl_init packs 16, 8, 4, 2 or 1 rows into a wave ------------------------------------------------------------
ROWS_A2 = (16, 63, 64, 65, 128, 256, 512, 513, 1024)


def rows_per_wave():
    """(7, 3, A2), 21 rows: a run at the end of one row and a run at the start of the next (both ways round) are never linked"""
    out = []
    for A2 in ROWS_A2:
        for form in ("end_start", "start_end"):
            lab = np.zeros((21, A2), np.uint8)
            first = 0 if form == "end_start" else 1
            lab[first::2, A2 - 3:] = 1
            lab[1 - first::2, :3] = 1
            out += _emit(f"rows/{A2}/{form}", lab.reshape(7, 3, A2), 1, {"n6": 21}, channels=(3, 1))
        out += _emit(f"rows/{A2}/full", np.ones((7, 3, A2), np.uint8), 1, {"n6": 1, "n18": 1, "n26": 1}, channels=(3, 1))
    return out


# ---- 3. tile seams: 64 levels + a halo level per tile, RT-row groups + a halo row -----------------------------------------------------
SEAM_SHAPES = ((3, 65, 40), (3, 129, 70), (65, 3, 40), (129, 5, 70), (66, 67, 20), (5, 33, 1100))


def _spaced(cands, S, gap):
    got = []
    for p in cands:
        if 0 <= p < S and all(abs(p - q) >= gap for q in got):
            got.append(p)
    return sorted(got)


def tile_seams():
    out = []
    for shape in SEAM_SHAPES:
        A0, A1, A2 = shape
        tag = "x".join(map(str, shape))
        # a solid with single-voxel cuts: one component, almost every plane link implied
        lab = np.ones(shape, np.uint8)
        lab[0, 0, 0] = 0; lab[A0 // 2, A1 // 2, A2 // 2] = 0; lab[A0 - 1, A1 - 1, A2 - 1] = 0
        for L in (64, 128):
            if L < A0:
                lab[L - 1, 1, 5] = 0; lab[L, A1 - 2, 9] = 0
            if L < A1:
                lab[1, L - 1, 7] = 0; lab[A0 - 2, L, 11] = 0
            if L < A2:
                lab[1, 1, L - 1] = 0; lab[A0 - 2, A1 - 2, L] = 0
        out += _emit(f"seam/{tag}/solid_cuts", lab, 1, {"n6": 1, "n26": 1})
        # plates one voxel thick, two sets of positions per orientation (around the seams / on the seams' first levels)
        for ax in range(3):
            for which, cands in (("a", (0, 63, 65, 127, 129, shape[ax] - 1)), ("b", (1, 64, 128, shape[ax] - 1))):
                pos = _spaced(cands, shape[ax], 2)
                lab = np.zeros(shape, np.uint8)
                idx = [slice(None)] * 3
                idx[ax] = pos
                lab[tuple(idx)] = 1
                out += _emit(f"seam/{tag}/plates{ax}{which}", lab, 1, {"n6": len(pos), "n26": len(pos)})
        # two solids that touch at ONE voxel face across level L - 1 | L; the twin touches there by an edge diagonal only
        for ax in (0, 1):
            levels = [L for L in (64, 128) if L < shape[ax]]
            if not levels:
                continue
            for twin in (False, True):
                lab = np.zeros(shape, np.uint8)
                for L in levels:
                    for (lo, hi), (o_lo, o_hi), (z_lo, z_hi) in (((L - 3, L - 1), (0, 1), (2, 8)), ((L, L + 2), (1, 2), (9, 15) if twin else (8, 14))):
                        idx = [None, None, slice(z_lo, z_hi + 1)]
                        idx[ax] = slice(lo, hi + 1); idx[1 - ax] = slice(o_lo, o_hi + 1)
                        lab[tuple(idx)] = 1
                claims = {"n6": 2 * len(levels), "n18": len(levels)} if twin else {"n6": len(levels)}
                out += _emit(f"seam/{tag}/touch{ax}{'_diag' if twin else ''}", lab, 1, claims)
        # pairs of solids that touch only across a row a1 = g - 1 | g where g starts an RT-row group of the plane-to-plane tiles; B's
        # plane link at row g has A above it in ONE plane only (through the halo row), so it must be made
        P = (A2 + 63) // 64
        cands = [rt * m for m in (1, 2) for rt in _rts(P) if rt > 1] + [1, 8, 16, 24]        # (RT = 1: every row starts a group)
        gs = _spaced([g for g in cands if 1 <= g <= A1 - 1], A1, 7)
        za, zb = ((1003, 1030), (1020, 1060)) if A2 >= 1100 else ((3, 10), (8, 15))
        lab = np.zeros(shape, np.uint8)
        pairs = 0
        for p in (0, 62, 126):
            if p + 2 >= A0:
                continue
            for g in gs:
                lab[p:p + 2, max(0, g - 3):g, za[0]:za[1] + 1] = 1
                lab[p + 1:p + 3, g:g + 3, zb[0]:zb[1] + 1] = 1
                pairs += 1
        out += _emit(f"seam/{tag}/rt_pairs", lab, 1, {"n6": pairs, "group_rows": gs})
    return out


# ---- 4. implied plane links: k_ccl_merge_tile<1> skips a link the row above implies ---------------------------------------------------
def _implied_case(variant, twin):
    """Structures in planes 1 and 2 of a (4, 33, A2) grid.  Plane 1 holds run [a, b] in row r, plane 2 run [c, d] (they overlap on
    [c, b]); row r - 1 holds a short run in each plane.  The twin moves everything in plane 2 along a2 until no voxel of it faces
    plane 1: the two halves then touch by edge diagonals only.  Two zones along a2 hold structures at different rows r."""
    wide = variant in ("window_hi", "window_lo")
    A2, z1 = (380, 192) if wide else (250, 128)
    a, b, c, d = (40, 100, 50, 110) if wide else (10, 30, 20, 40)
    up = {"inside": ((24, 26), (25, 27)), "outside": ((12, 14), (12, 14)), "window_hi": ((80, 82), (80, 82)), "window_lo": ((55, 57), (55, 57)),
          "stack": None}[variant]
    shift = b - c + 1 if twin else 0
    P = (A2 + 63) // 64
    lab = np.zeros((4, 33, A2), np.uint8)
    if variant == "stack":
        zones = ((0, (0, 15)), (z1, (7, 21)))
    elif wide:
        zones = ((0, (1, 4, 9, 18, 28)), (z1, (0, 8, 12, 16, 27)))
    else:
        zones = ((0, (1, 7, 15, 30)), (z1, (0, 8, 21, 28)))
    nstruct = n_above = n_twin = 0
    for z0, rows in zones:
        for r in rows:
            nstruct += 1
            if variant == "stack":
                for q in range(r, r + 10):
                    _run(lab[1, q], z0 + a, z0 + b); _run(lab[2, q], z0 + c + shift, z0 + d + shift)
                n_twin += 2
                continue
            _run(lab[1, r], z0 + a, z0 + b); _run(lab[2, r], z0 + c + shift, z0 + d + shift)
            n_twin += 2
            if r >= 1:
                n_above += 1
                _run(lab[1, r - 1], z0 + up[0][0], z0 + up[0][1]); _run(lab[2, r - 1], z0 + up[1][0] + shift, z0 + up[1][1] + shift)
                if variant == "outside":                         # plane 2's short run then hangs over nothing of its own plane
                    n_twin += 1
    if twin:
        claims = {"n6": n_twin, "n18": nstruct, "implied": {"same": 0, "other": 0, "overlaps": 0}}
    else:
        same = {"inside": n_above, "outside": 0, "window_hi": 0, "window_lo": n_above, "stack": 9 * nstruct}[variant]
        other = n_above if variant == "window_hi" else 0
        claims = {"n6": nstruct, "implied": {"same": same, "other": other}, "twin_n6": n_twin}
        firsts = sorted({rt * m for rt in _rts(P) if rt > 1 for m in range(1, 33 // rt + 1)})
        claims["group_first_rows"] = firsts
    return _emit(f"implied/{variant}/{'apart' if twin else 'joined'}", lab, 1, claims)


def implied_links_cases():
    out = []
    for variant in ("inside", "outside", "window_hi", "window_lo", "stack"):
        for twin in (False, True):
            out += _implied_case(variant, twin)
    return out


# ---- 5. shapes: deep union paths, label order against root order, the three connectivities ------------------------------------------
def _serpentine2d(n, m):
    g = np.zeros((n, m), bool)
    g[::2] = True
    g[1::4, m - 1] = True
    g[3::4, 0] = True
    return g


def _spiral2d(n, m):
    """a square spiral from (0, 0) inwards, arms one voxel apart"""
    g = np.zeros((n, m), bool)
    i = j = d = turns = 0
    g[0, 0] = True
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    while turns < 2:
        di, dj = dirs[d]
        ni, nj, ai, aj = i + di, j + dj, i + 2 * di, j + 2 * dj
        if 0 <= ni < n and 0 <= nj < m and not g[ni, nj] and not (0 <= ai < n and 0 <= aj < m and g[ai, aj]):
            i, j, turns = ni, nj, 0
            g[i, j] = True
        else:
            d, turns = (d + 1) % 4, turns + 1
    return g


def _nested_u2d(n, L):
    """n nested U shapes, prongs along the second axis from 0, each joined only at its far end: 2n rows two apart"""
    g = np.zeros((4 * n - 1, L), np.uint8)
    for k in range(n):
        top, bot, far = 2 * k, 2 * (2 * n - 1 - k), L - 1 - 2 * k
        g[top, :far + 1] = 1; g[bot, :far + 1] = 1; g[top:bot + 1, far] = 1
    return g


def _w_pair2d(L):
    """a W (prongs in rows 0, 4, 8 from column 2, joined at the far end) interleaved with a U joined at the NEAR end (rows 2, 6)"""
    g = np.zeros((9, L), np.uint8)
    g[0:9:4, 2:] = 1; g[:, L - 1] = 1
    g[2:7:4, :L - 2] = 1; g[2:7, 0] = 1
    return g


def _embed(g2, plane, extrude, pad=1):
    """a 2-D shape in the axis plane `plane` = (p, q), extruded along the third axis, with `pad` empty voxels around it there"""
    p, q = plane
    e = 3 - p - q
    shape = [0, 0, 0]
    shape[p], shape[q], shape[e] = g2.shape[0], g2.shape[1], extrude + 2 * pad
    lab = np.zeros(shape, np.uint8)
    idx = [None, None, None]
    for k in range(pad, pad + extrude):
        idx[p], idx[q], idx[e] = slice(None), slice(None), k
        lab[tuple(idx)] = g2
    return lab


def shapes():
    out = []
    planes = ((0, 1), (0, 2), (1, 2))
    for plane in planes:
        for flip in (False, True):
            dims = (21, 150) if plane[1] == 2 else (41, 40)          # along a2 a shape crosses two window edges
            for kind, fn in (("serpentine", _serpentine2d), ("spiral", _spiral2d)):
                g2 = fn(*dims)
                if flip:
                    g2 = g2[::-1, ::-1]
                for ex in (1, 3):
                    claims = {"n6": 1, "n26": 1}
                    if ex == 1:
                        claims["path"] = True
                    out += _emit(f"shape/{kind}/p{plane[0]}{plane[1]}{'f' if flip else ''}/e{ex}", _embed(g2, plane, ex), 1, claims)
            for kind, g2, n in (("nested_u", _nested_u2d(4, 140), 4), ("w_pair", _w_pair2d(140), 2)):
                if flip:
                    g2 = g2.T                                           # prongs along the plane's first axis
                claims = {"n6": n, "n26": n}
                if kind == "nested_u":
                    claims["first_voxel_on_prong"] = True
                out += _emit(f"shape/{kind}/p{plane[0]}{plane[1]}{'t' if flip else ''}", _embed(g2, plane, 1), 1, claims)
    i, j, k = np.indices((12, 10, 70))
    out += _emit("shape/checkerboard", (i + j + k) % 2 == 0, 1, {"members_eq_n6": True, "n18": 1, "n26": 1})
    # two combs with interleaved teeth: planes 0 / 1, rows 0, 4, 8 / 1, 5, 9 -- the teeth run side by side by an edge diagonal ...
    lab = np.zeros((2, 11, 100), np.uint8)
    lab[0, 0:9:4, :98] = 1; lab[0, :9, 0] = 1
    lab[1, 1:10:4, 2:] = 1; lab[1, 1:10, 99] = 1
    out += _emit("shape/combs_edge", lab, 1, {"n6": 2, "n18": 1, "n26": 1})
    # ... or end where the other comb's begin, across the window edge 63 | 64: a corner diagonal each
    lab = np.zeros((2, 11, 100), np.uint8)
    lab[0, 0:9:4, :64] = 1; lab[0, :9, 0] = 1
    lab[1, 1:10:4, 64:] = 1; lab[1, 1:10, 99] = 1
    out += _emit("shape/combs_corner", lab, 1, {"n6": 2, "n18": 2, "n26": 1})
    # three nested box shells, one empty voxel between them (their bounding boxes contain one another)
    lab = np.zeros((16, 18, 80), np.uint8)
    for s in (0, 2, 4):
        box = lab[s:16 - s, s:18 - s, s:80 - s]
        box[:] = 1
        box[1:-1, 1:-1, 1:-1] = 0
    out += _emit("shape/shells", lab, 1, {"n6": 3, "n26": 3})
    # the staircase a2 = a0 + a1 + 50: one voxel thick it hangs together by edge diagonals only, two voxels thick by faces
    i, j, k = np.indices((10, 12, 75))
    out += _emit("shape/stairs_thin", k == i + j + 50, 1, {"members_eq_n6": True, "n18": 1, "n26": 1})
    out += _emit("shape/stairs_thick", (k == i + j + 50) | (k == i + j + 51), 1, {"n6": 1, "n26": 1})
    return out


# ---- 6. thresholds: kSeg = 8, kSlots = 32, kFirst = 64, 1024-window chunks, dcap ----------------------------------------------------
def _seg_window(nseg, odd):
    """a 64-voxel window with exactly nseg segments: two voxels long, one apart (32 segments: single voxels)"""
    w = np.zeros(64, np.uint8)
    if nseg == 32:
        w[int(odd)::2] = 1
    else:
        for s in range(nseg):
            w[3 * s + int(odd):3 * s + int(odd) + 2] = 1
    return w


def thresholds():
    out = []
    # (2, 8, 512): 64 windows per plane = one wave of k_ccl_finish each; plane 0 alternates 8 and 9 segments, plane 1 cycles 7, 8, 9, 32
    lab = np.zeros((2, 8, 512), np.uint8)
    for r in range(8):
        for t in range(8):
            lab[0, r, 64 * t:64 * t + 64] = _seg_window(8 + t % 2, r % 2)
            lab[1, r, 64 * t:64 * t + 64] = _seg_window((7, 8, 9, 32)[(t + r) % 4], r % 2)
    out += _emit("thr/segments", lab, 1, {"segs": [7, 8, 9, 32], "alt89": True}, channels=(3, 1))
    # (20, 60, 64): 1200 windows; isolated voxels whose windows sit on both sides of thread 63 | 64 and of block 0 | 1 of k_ccl_number
    wins = (0, 5, 251, 252, 253, 255, 256, 257, 259, 600, 1019, 1020, 1022, 1023, 1024, 1025, 1026, 1030, 1199)
    lab = np.zeros((1200, 64), np.uint8)
    for w in wins:
        lab[w, (7 * w + 3 * (w // 60)) % 62] = 1
    lab[1023, 40] = lab[1024, 50] = 1                                   # second roots in the windows at the block edge
    out += _emit("thr/root_windows", lab.reshape(20, 60, 64), 1, {"n6": len(wins) + 2, "n26": len(wins) + 2, "root_windows": list(wins)})
    # (4, 64, 64): 256 windows = one workgroup of k_ccl_finish; 40 two-voxel components, more than its 32 statistics slots
    lab = np.zeros((256, 64), np.uint8)
    for c in range(40):
        w, z = 6 * c + 1, (5 * c) % 60
        lab[w, z] = 1
        if c % 2 and w % 64 != 63:
            lab[w + 1, z] = 1                                           # along a1: the component's two voxels belong to two lanes
        else:
            lab[w, z + 1] = 1
    out += _emit("thr/slots40", lab.reshape(4, 64, 64), 1, {"n6": 40, "n26": 40, "members": 80})
    # exactly 64, 65 and 130 components: the first read-back holds 64 records per colour
    for n in (64, 65, 130):
        lat = np.zeros(3 * 3 * 35, np.uint8)
        lat[:n] = 1
        lab = np.zeros((5, 6, 70), np.uint8)
        lab[::2, ::2, ::2] = lat.reshape(3, 3, 35)
        out += _emit(f"thr/count{n}", lab, 1, {"n6": n, "n26": n})
    # eight colours, the first with more components than the 16384 / 8 records a colour then has
    lat = np.zeros(10 * 15 * 32, np.uint8)
    lat[:2100] = 1
    lab = np.zeros((20, 30, 64), np.uint8)
    lab[::2, ::2, ::2] = lat.reshape(10, 15, 32)
    for k in range(2, 9):
        lab[2 * k + 1, 1, 1:4] = k; lab[2 * k + 1, 5, 7] = k; lab[1, 2 * k + 1, 61:64] = k
    out += _emit("thr/dcap", lab, 8, {"ncomp": [2100] + [3] * 7}, channels=(3, 1))
    return out


BUILDERS = {"long_rows": long_rows, "long_rows_multi": long_rows_multi, "rows_per_wave": rows_per_wave, "tile_seams": tile_seams,
            "implied_links": implied_links_cases, "shapes": shapes, "thresholds": thresholds}
_built = {}


def cases(builder):
    """the cases of a builder, built once per process; nobody writes to them"""
    if builder not in _built:
        _built[builder] = BUILDERS[builder]()
        for _, grid, _, _ in _built[builder]:
            grid.setflags(write=False)
    return _built[builder]
