"""meshify_colored_voxel_grid (csrc/mesh.hip) pinned on constructed inputs (tests/meshify_cases.py) against the NumPy restatement
(tests/mesh_restate.py): verts, faces and normals bit for bit, and colours exactly.  Every lattice voxel has a colour of its own,
so a colour names the voxel the nearest search chose and the published tie rule ("ties go to the smallest lattice index",
include/pb3d.h) is asserted, not only membership of the tie set.

The CPU tests state the conditions that keep the GPU tests from being vacuous: the inputs hold every (cube case, zbits) pair, the
block-seam lattices cross a seam with a shared vertex, each nearest-search case reaches the seam it is named for, the tie cases
hold ties between different colours, and two plausible wrong tie rules change their colours."""
import time

import numpy as np
import pytest

import mesh_restate as mr
import meshify_cases as mc

COVERAGE = [(name, s) for name, (_, strides) in mc.coverage_cases().items() if not name.startswith("corner") for s in strides]


def exact(got, want):
    assert len(got) == len(want) == 4
    for what, g, w in zip(("verts", "faces", "colours", "normals"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), f"{what}: {int(np.any(g != w, axis=-1).sum())} of {len(w)} rows differ"


def unravel(mask, index):
    return tuple(int(x) for x in np.unravel_index(index, mask.shape))


# ---- CPU: the inputs reach what they are built for ----------------------------------------------------------------------------
def test_inputs_hold_every_case_and_zbits_pair():
    seen = set()
    for occ, _ in mc.coverage_cases().values():
        seen |= mc.case_zbits_pairs(occ)
    missing = sorted({(cs, z) for cs in range(1, 255) for z in range(8)} - seen)
    assert not missing, f"{len(missing)} (case, zbits) pairs no input reaches: {missing[:20]}"
    assert len(seen) == 254 * 8


@pytest.mark.parametrize("axis,zbits", [(0, 6), (1, 5), (2, 3)])
def test_lines_hold_every_case_once(axis, zbits):
    occ = mc.line_lattice(axis)
    cases = mc.case_volume(occ).ravel()
    assert occ.shape[axis] == 257 and len(cases) == 256 and sorted(cases) == list(range(256))
    assert {z for _, z in mc.case_zbits_pairs(occ)} == {zbits}


def test_corner_lattices_are_the_254_cases():
    lat = mc.corner_lattices()
    assert [int(mc.case_volume(occ)[0, 0, 0]) for occ in lat] == list(range(1, 255))


def test_seam_lattices_share_vertices_across_blocks():
    cubes = {}
    for name, occ in mc.seam_lattices().items():
        _, _, (_, faces, _, _) = mc.reference(name)
        n = cubes[name] = (occ.shape[0] - 1) * (occ.shape[1] - 1) * (occ.shape[2] - 1)
        refs = mc.seam_references(occ, faces)
        assert len(refs) == (n - 1) // 256 and all(r > 0 for r in refs), (name, refs)
    assert sorted(cubes.values()) == [255, 256, 256, 257, 258, 258]


def test_word_seam_cases_reach_the_word_seams():
    """over the (n, 3, n) cases: winners 128 and more steps to either side of floor(q2), queries at the last bit of a word whose
    winner lies to the left and to the right, winners in a partial last word, and floor(q2) + 1 == n2 at n = 64"""
    seen = set()
    for n, pairs in mc.WORD_SEAMS.items():
        for ks, kw in pairs:
            mask, q, best, ties = mc.winners(f"words{n}_{ks}_{kw}")
            assert (q[:, 1] >= 0).all() and (q[:, 1] <= 2).all() and (q[:, 2] >= 0).all() and (q[:, 2] <= n - 1).all()
            for qq, b, t in zip(q, best, ties):
                i, j, k = unravel(mask, b)
                kf = int(np.floor(qq[2]))
                if i != n - 1:
                    continue                                     # a vertex of the far voxel, answered by the near one
                assert (i, j, k) == (n - 1, 1, kw) and len(t) == 1
                seen |= {("left128", kf - k >= 128), ("right128", k - kf >= 128), ("mask63_left", kf % 64 == 63 and k <= kf),
                         ("mask0_right", (kf + 1) % 64 == 0 and k > kf), ("first_bit_of_word", k == kf + 1 and k % 64 == 0),
                         ("last_bit_of_word", k == kf and k % 64 == 63), ("partial_word", n % 64 != 0 and k >> 6 == (n - 1) >> 6),
                         ("no_right_scan_64", n == 64 and kf + 1 == n and k < kf), ("no_right_scan_128", n == 128 and kf + 1 == n),
                         ("outside", qq[0] > n - 1), ("inside", qq[0] <= n - 1)}
    want = {"left128", "right128", "mask63_left", "mask0_right", "first_bit_of_word", "last_bit_of_word", "partial_word",
            "no_right_scan_64", "no_right_scan_128", "outside", "inside"}
    assert {name for name, hit in seen if hit} == want


@pytest.mark.parametrize("name,axis,low,high", [("ring_tie0", 0, (1, 1, 2), (6, 1, 2)), ("ring_tie1", 1, (10, 1, 5), (10, 6, 5))])
def test_ring_tie_cases_tie_across_a_ring_boundary(name, axis, low, high):
    """a query half-way between two voxels 5 apart: the higher in ring 2, the lower (the winner) in ring 3, whose lower bound
    (3 - 1/2)^2 equals the best distance"""
    mask, q, best, ties = mc.winners(name)
    pair = sorted(np.ravel_multi_index(p, mask.shape) for p in (low, high))
    hits = [v for v in range(len(q)) if sorted(ties[v]) == pair]
    assert hits
    for v in hits:
        assert q[v][axis] == low[axis] + 2.5 and ((q[v] - np.array(low)) ** 2).sum() == 6.25 == ((q[v] - np.array(high)) ** 2).sum()
        assert mc.ring_of(mask, q[v], pair[1]) == 2 and mc.ring_of(mask, q[v], pair[0]) == 3 and best[v] == pair[0]


@pytest.mark.parametrize("name", list(mc.LIMIT_TIES))
def test_limit_tie_cases_tie_in_the_last_word_of_the_scan(name):
    """the ring-1 voxel ties with the ring-0 one and lies in another word than floor(q2), on the named side: exactly as far as
    sqrt(best - row distance) lets that row's scan go"""
    mask, q, best, ties = mc.winners(name)
    src, near, far = mc.LIMIT_TIES[name]
    a, b = np.ravel_multi_index(far, mask.shape), np.ravel_multi_index(near, mask.shape)
    hits = [v for v in range(len(q)) if sorted(ties[v]) == [a, b]]
    assert hits and all(best[v] == a and tuple(q[v]) == (100.5, 1.0, float(src[2])) for v in hits)
    assert mc.ring_of(mask, q[hits[0]], b) == 0 and mc.ring_of(mask, q[hits[0]], a) == 1
    assert (far[2] > src[2]) == name.endswith("right") and far[2] >> 6 != src[2] >> 6


@pytest.mark.parametrize("name", list(mc.long_search_cases()))
def test_long_search_cases_run_many_rings(name):
    mask, q, best, ties = mc.winners(name)
    rings = [mc.ring_of(mask, qq, b) for qq, b, t in zip(q, best, ties) if len(t) == 1]
    assert max(rings) >= 6, rings


@pytest.mark.parametrize("name", list(mc.outside_cases()))
def test_outside_cases_leave_the_box_and_the_clamped_plane(name):
    grid, s, _ = mc.reference(name)
    assert s == 3 and grid.shape[2] % 3 == int(name[-1]) and (grid.shape[0] > grid.shape[2]) == name.startswith("below")
    mask, q, best, ties = mc.winners(name)
    n0 = mask.shape[0]
    hits = 0
    for qq, b, t in zip(q, best, ties):
        out = qq[0] < 0 if name.startswith("below") else qq[0] > n0 - 1
        if out and qq[0] * 2 != np.floor(qq[0] * 2) and len(t) == 1 and unravel(mask, b)[0] != mc.cell(qq[0], n0):
            hits += 1
    assert hits


@pytest.mark.parametrize("name", list(mc.tie_cases()))
def test_tie_cases_tie_between_colours_and_wrong_rules_show(name):
    """each tie case holds a vertex tied between two colours (and, as labels, between two labels); the restated search equals the
    restatement under the published rule, and differs from it under "largest index" and under "first candidate met\""""
    grid, s, (v, _, c, _) = mc.reference(name)
    occ, _, tail = mc.tie_cases()[name]
    mask, q, best, ties = mc.winners(name)
    flat = grid[::s, ::s, ::s].reshape(-1, 3)
    lab = mc.label_grid(occ, s, tail)[::s, ::s, ::s].ravel()
    assert any(len(np.unique(flat[t], axis=0)) > 1 for t in ties)
    assert any(len(np.unique(lab[t])) > 1 for t in ties)
    assert np.array_equal(mc.voxel_of(c), best)
    got = {rule: mc.colors_by_rule(grid, s, v, rule) for rule in ("smallest", "largest", "first")}
    assert got["smallest"].dtype == c.dtype and np.array_equal(got["smallest"], c)
    for rule in ("largest", "first"):
        assert np.any(got[rule] != c), f"the rule '{rule}' gives the same colours"


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_corner_lattices_match_restatement():
    """one cube, zbits 7, every case: 254 count + fill calls"""
    import pb3d
    grids = [mc.index_grid(occ) for occ in mc.corner_lattices()]
    want = [mr.meshify(g, 1) for g in grids]
    t0 = time.perf_counter()
    got = [pb3d.meshify_colored_voxel_grid(g) for g in grids]
    print(f"254 meshify calls on 2x2x2 lattices: {time.perf_counter() - t0:.3f} s")
    for g, w in zip(got, want):
        exact(g, w)


@pytest.mark.gpu
@pytest.mark.parametrize("name,stride", COVERAGE, ids=[f"{n}-s{s}" for n, s in COVERAGE])
def test_every_case_and_zbits_pair_matches_restatement(name, stride):
    import pb3d
    grid, s, want = mc.reference(name, stride)
    got = pb3d.meshify_colored_voxel_grid(grid, stride=s)
    exact(got, want)
    off = np.array(mc.OFF) / 255.0
    assert (grid == mc.OFF).all(-1).any() == (s > 1) and not (got[2] == off).all(-1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(mc.seam_lattices()))
def test_block_seams_match_restatement(name):
    import pb3d
    grid, s, want = mc.reference(name)
    exact(pb3d.meshify_colored_voxel_grid(grid, stride=s), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(mc.search_cases()))
def test_nearest_search_seams_match_restatement(name):
    import pb3d
    grid, s, want = mc.reference(name)
    got = pb3d.meshify_colored_voxel_grid(grid, stride=s)
    exact(got, want)
    assert not (got[2] == np.array(mc.OFF) / 255.0).all(-1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(mc.tie_cases()))
def test_tie_cases_label_twin_matches_restatement(name):
    """the C = 1 path: neighbouring voxels carry different labels, the off-lattice label never shows"""
    from pb3d import labels
    occ, s, tail = mc.tie_cases()[name]
    lab = mc.label_grid(occ, s, tail)
    got = labels.meshify_colored_voxel_grid_labels(lab, mc.PALETTE, stride=s)
    exact(got, mr.meshify(mc.label_rgb(lab), s))
    assert not (got[2] == mc.PALETTE[mc.OFF_LABEL - 1] / 255.0).all(-1).any()
