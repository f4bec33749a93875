"""Fixtures of perspective_paint: tests/golden/ppaint_synth.npz + .json (inputs, painted grids and counts of the small synthetic cases)
and ppaint_charminar.npz + .json (the stored Charminar grid under its stored final front and drone cameras and its two committed
masks, skip = the masks' background: counts, SHA-256 of the painted grid, and the voxels painting changed among every second index
per axis).

Every result is computed by tests/paint_restate.py.  Before anything is written, the restatement is tied to the reference, imported
through tools/ref_import.py, for every case and view:
  1. the z-buffer the restatement paints against equals the reference's compute_global_depth_buffer of the same grid;
  2. the pixels at which the restatement sees a subject voxel are the reference's project_part_visible of the same points.
Every synthetic case must have each view decide at least 5 % of the subject voxels and leave at least 5 % of them undecided; in at
least one case a later view decides voxels an earlier view saw but skipped, and in at least one a later view decides voxels no
earlier view saw.  Each view of the real-data case must decide at least 1000 voxels.  Data only; nothing of the reference's text is
copied.  Run: python tools/gen_golden_paint.py"""
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
import paint_restate as pt  # noqa: E402
import perspective_restate as pr  # noqa: E402


def tie_to_reference(eh, grid, views, colors, eps, zbufs, own_zbufs, trace, what):
    g4 = grid if grid.ndim == 4 else grid[..., None]
    pts, _ = pr.points_of(pr.subject(grid, colors))
    for k, ((image, cam), zb) in enumerate(zip(views, zbufs)):
        H, W = image.shape[:2]
        if own_zbufs:
            want = eh.compute_global_depth_buffer(g4, cam, H, W)
            assert want.dtype == zb.dtype and np.array_equal(want, zb), (what, k, "z-buffer", int((want != zb).sum()))
        seen, _, ui, vi = trace[k]
        got = np.zeros((H, W), bool)
        got[vi, ui] = True
        want = eh.project_part_visible(pts, cam, zb, H, W, eps)
        assert np.array_equal(got, want), (what, k, "seen pixels", int((got != want).sum()))
        assert seen.any(), (what, k, "no subject voxel is seen")


def later_view_stats(trace):
    """(voxels a later view decides that an earlier one saw but skipped, voxels a later view decides that no earlier view saw)"""
    skipped = fresh = 0
    seen_before = np.zeros_like(trace[0][0])
    for k, (seen, paints, _, _) in enumerate(trace):
        if k:
            skipped += int((paints & seen_before).sum())
            fresh += int((paints & ~seen_before).sum())
        seen_before = seen_before | seen
    return skipped, fresh


def main():
    ref_import.load_reference()
    import utils.eval_helpers_intra as eh

    arrays, meta = {}, {}
    any_skipped = any_fresh = False
    for name, case in pt.synthetic_cases().items():
        grid, views, colors, skip, eps = case["grid"], case["views"], case["colors"], case["skip"], case["eps"]
        zbufs = case["zbufs"] if case["zbufs"] is not None else pt.zbuffers(grid, views)
        trace = []
        out, decided = pt.paint(grid, views, colors, skip, eps, zbufs, trace)
        tie_to_reference(eh, grid, views, colors, eps, zbufs, case["zbufs"] is None, trace, name)
        sel = pr.subject(grid, colors)
        n = int(sel.sum())
        left = n - int(decided.sum())
        for k, d in enumerate(decided):
            assert d >= 0.05 * n, (name, f"view {k} decides {d} of {n}")
        assert left >= 0.05 * n, (name, f"{left} of {n} undecided")
        skipped, fresh = later_view_stats(trace)
        any_skipped |= skipped > 0; any_fresh |= fresh > 0
        assert np.array_equal(out[~sel], grid[~sel]) and np.array_equal(pr.subject(out), pr.subject(grid))
        arrays[f"{name}/grid"] = grid; arrays[f"{name}/out"] = out; arrays[f"{name}/decided"] = decided
        for k, (image, _) in enumerate(views):
            arrays[f"{name}/image{k}"] = image
            if case["zbufs"] is not None:
                arrays[f"{name}/zbuf{k}"] = zbufs[k]
        plain = (lambda c: [int(x) for x in c] if np.ndim(c) else int(c))
        meta[name] = {"cams": [pt.cam_record(c) for _, c in views], "colors": None if colors is None else [plain(c) for c in colors],
                      "skip": [plain(c) for c in skip], "eps": pt.eps_record(eps), "zbufs": case["zbufs"] is not None, "subject": n,
                      "undecided": left, "changed": int(((out != grid).any(axis=-1) if grid.ndim == 4 else out != grid).sum()),
                      "later_view_decides_seen_but_skipped": skipped, "later_view_decides_unseen_before": fresh}
        print(name, grid.shape, n, decided.tolist(), left, skipped, fresh, file=sys.stderr)
    assert any_skipped and any_fresh
    cs = pt.synthetic_cases()
    on, off = pt.paint(cs["skip_on"]["grid"], cs["skip_on"]["views"], None, cs["skip_on"]["skip"])[0], pt.paint(cs["skip_off"]["grid"], cs["skip_off"]["views"])[0]
    assert not np.array_equal(on, off), "the skip list does not matter"
    own = pt.paint(cs["zbuf_other"]["grid"], cs["zbuf_other"]["views"], None, cs["zbuf_other"]["skip"])[0]
    assert not np.array_equal(own, arrays["zbuf_other/out"]), "the supplied z-buffers do not matter"
    np.savez_compressed(os.path.join(GOLDEN, "ppaint_synth.npz"), **arrays)
    json.dump({"cases": meta}, open(os.path.join(GOLDEN, "ppaint_synth.json"), "w"), indent=1)

    # ---- the stored Charminar grid: its final front and drone cameras, its two masks, the background skipped ---------------------------
    mon = "Charminar"
    grid, views = pt.stored_case(mon)
    skip = [pt.BACKGROUND]
    zbufs = pt.zbuffers(grid, views)
    trace = []
    out, decided = pt.paint(grid, views, None, skip, 1e-3, zbufs, trace)
    tie_to_reference(eh, grid, views, None, 1e-3, zbufs, True, trace, mon)
    assert decided.min() >= 1000, decided
    at, vals = pt.changed_sample(grid, out)
    rec = {"monument": mon, "shape": list(grid.shape), "views": ["front", "drone"], "cameras": f"stored_{mon}_camera_params_final.json",
           "images": "resize_mask_to_voxel_grid(mask)", "skip": [list(pt.BACKGROUND)], "eps": pt.eps_record(1e-3),
           "sample": "flat indices into out[::2, ::2, ::2] of the voxels whose value differs from the input's, and their values",
           "subject": int(pr.subject(grid).sum()), "decided": decided.tolist(), "changed": int((out != grid).any(axis=-1).sum()),
           "sha256": pt.sha(out)}
    print(mon, rec["subject"], rec["decided"], rec["changed"], len(at), file=sys.stderr)
    np.savez_compressed(os.path.join(GOLDEN, "ppaint_charminar.npz"), **{"sample/index": at, "sample/value": vals})
    json.dump(rec, open(os.path.join(GOLDEN, "ppaint_charminar.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
