"""Fixtures of perspective_carve: tests/golden/pcarve_synth.npz + .json (inputs, carved grids and counts of the small synthetic cases)
and pcarve_charminar.npz + .json (the stored Charminar grid under its stored final front and drone cameras: counts, SHA-256 of the
carved grid and its keep bits at every second voxel per axis, packed, for every occupied voxel and for the minaret colours alone).

Every result is computed by tests/perspective_restate.py.  Before anything is written, the restatement's per-point pixels are tied
to the reference: for every case, view and the case's subject points, the image built from those pixels (last writer wins) must
equal the image of the reference's own project_colored_voxels, imported through tools/ref_import.py.  Data only; nothing of the
reference's text is copied.

Every case not built to be trivial must have each view remove at least 1 % of the subject voxels and leave at least 1 % of them.
The real-data case is Charminar, not Akbar: Akbar's front view removes 0.31 % of its whole grid (the grid was carved from that
mask), Charminar's views remove 1.67 % and 10.4 % of the whole grid and 1.74 % and 25.1 % of the minaret voxels.
Run: python tools/gen_golden_perspective.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "part-based-3d-reconstruction_amd"))

import ref_import  # noqa: E402
import perspective_restate as pr  # noqa: E402


def tie_to_reference(pu, grid, views, colors, what):
    """the restatement's pixels of the case's subject points give the reference's image, for every view"""
    pts, _ = pr.points_of(pr.subject(grid, colors))
    idx = np.arange(len(pts), dtype=np.int64) + 1
    cols = np.stack([idx & 0xff, (idx >> 8) & 0xff, (idx >> 16) & 0xff], axis=1).astype(np.uint8)      # a point's own colour, never black
    for k, (mask, cam) in enumerate(views):
        H, W = pr.mask_set(mask).shape
        with np.errstate(all="ignore"):
            want = pu.project_colored_voxels(pts, cols, cam["cam_pos"], cam["target"], cam["f"], cam["cx"], cam["cy"], H, W)
        ui, vi, valid = pr.pixels(pts, cam, H, W)
        got = np.zeros((H, W, 3), np.uint8)
        got[vi[valid], ui[valid]] = cols[valid]
        assert np.array_equal(got, want), (what, k, int((got != want).any(axis=-1).sum()))
        assert valid.any(), (what, k, "no point lands inside the image")


def one_percent(n_subject, removed, left, what):
    for k, r in enumerate(removed):
        assert r >= 0.01 * n_subject, (what, f"view {k} removes {r} of {n_subject}")
    assert left >= 0.01 * n_subject, (what, f"{left} of {n_subject} left")


def main():
    pu = ref_import.load_reference()[2]

    arrays, meta = {}, {}
    for name, case in pr.synthetic_cases().items():
        grid, views, colors, outside = case["grid"], case["views"], case["colors"], case["outside"]
        tie_to_reference(pu, grid, views, colors, name)
        out, removed = pr.carve(grid, views, colors, outside)
        n = int(pr.subject(grid, colors).sum())
        left = int(pr.subject(out, colors).sum())
        assert left + int(removed.sum()) == n
        if not case["trivial"]:
            one_percent(n, removed, left, name)
        assert np.array_equal(out[~pr.subject(grid, colors)], grid[~pr.subject(grid, colors)])
        arrays[f"{name}/grid"] = grid; arrays[f"{name}/out"] = out; arrays[f"{name}/removed"] = removed
        for k, (mask, _) in enumerate(views):
            arrays[f"{name}/mask{k}"] = np.asarray(mask)
        meta[name] = {"cams": [pr.cam_record(c) for _, c in views], "colors": None if colors is None else [list(map(int, np.atleast_1d(c))) if np.ndim(c) else int(c) for c in colors],
                      "outside": outside, "trivial": case["trivial"], "subject": n, "left": left}
        print(name, grid.shape, n, removed.tolist(), left, file=sys.stderr)
    # what the half-to-even case is there for: many pixels exactly on .5 before rint
    case = pr.synthetic_cases()["half_even"]
    pts, _ = pr.points_of(pr.subject(case["grid"]))
    cam = case["views"][0][1]
    halves = int((((pts[:, 0] - cam["cam_pos"][0]) % 2 == 1) & (pts[:, 2] == 0)).sum())
    assert halves > 50, halves
    meta["half_even"]["points_on_half"] = halves
    np.savez_compressed(os.path.join(GOLDEN, "pcarve_synth.npz"), **arrays)
    json.dump({"cases": meta}, open(os.path.join(GOLDEN, "pcarve_synth.json"), "w"), indent=1)

    # ---- the stored Charminar grid: its final front and drone cameras, the silhouettes of its two masks -----------------------------
    from pb3d.config import PART_COLORS
    mon = "Charminar"
    grid, views = pr.stored_case(mon)
    bg = np.array(PART_COLORS["background"], np.uint8)
    views = [(np.any(m != bg, axis=-1), c) for m, c in views]
    minarets = [list(PART_COLORS["front_minarets"]), list(PART_COLORS["back_minarets"])]
    rec, arrays = {"monument": mon, "instead_of": "Akbar, whose front view removes 0.31 % of its whole grid: under the 1 % every view must remove",
                   "shape": list(grid.shape), "views": ["front", "drone"], "cameras": f"stored_{mon}_camera_params_final.json",
                   "silhouette": "any(resize_mask_to_voxel_grid(mask) != PART_COLORS['background'], axis=-1)",
                   "keep_bits": "np.packbits(occupied[::2, ::2, ::2].reshape(-1)) of the carved grid", "runs": {}}, {}
    for run, colors in (("all", None), ("minarets", minarets)):
        tie_to_reference(pu, grid, views, colors, run)
        out, removed = pr.carve(grid, views, colors)
        n, left = int(pr.subject(grid, colors).sum()), int(pr.subject(out, colors).sum())
        one_percent(n, removed, left, run)
        arrays[f"{run}/keep_bits"] = pr.keep_bits(out)
        rec["runs"][run] = {"colors": colors, "outside": "carve", "subject": n, "left": left, "removed": removed.tolist(), "sha256": pr.sha(out)}
        print(mon, run, n, removed.tolist(), left, file=sys.stderr)
    np.savez_compressed(os.path.join(GOLDEN, "pcarve_charminar.npz"), **arrays)
    json.dump(rec, open(os.path.join(GOLDEN, "pcarve_charminar.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
