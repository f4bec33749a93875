"""Fixtures of notebook 2's bbox camera init, keypoint fit and projection-IoU overlays (reference utils/camera_estimation.py:56-170,
:346-477): tests/golden/overlay_synth.npz + .json, overlay_akbar.json, overlay_init_fit.json.

Runs the reference's own three functions through tools/ref_import.py.  The arrays handed to plt.imshow and the titles are captured by
standing a recorder in for the module's `plt`; scikit-image is not a dependency of this project, so skimage.measure's label /
regionprops are stood in by scipy.ndimage.label (8-connected, raster order) for the reference's own extract_minaret_kps_for_view.  Every captured image, title
and bound is asserted equal to tests/overlay_restate.py before anything is written.  Data only; nothing of the reference's text is
copied.  Full images for the small synthetic cases; SHA-256, IoU and outline-pixel counts for the stored Akbar grid under its
stored init / kp / final cameras.
Run: python tools/gen_golden_overlays.py"""
import hashlib
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "part-based-3d-reconstruction_amd"))

import ref_import  # noqa: E402
import overlay_restate as ovr  # noqa: E402

MODES = ("part_on_whole", "whole_on_whole", "whole_on_whole_color")
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class Recorder:
    """stands in for matplotlib.pyplot inside the reference module"""

    def __init__(self):
        self.images, self.titles = [], []

    def imshow(self, a, *args, **kw):
        self.images.append(np.array(a, copy=True))

    def title(self, t, *args, **kw):
        self.titles.append(t)

    def __getattr__(self, name):
        return lambda *a, **k: None


def capture(ce, grid, part_colors, image, cam, mode):
    rec = Recorder()
    keep, ce.plt = ce.plt, rec
    try:
        with redirect_stdout(io.StringIO()):
            ce.visualize_voxel_projection_iou(grid, part_colors, image, cam, mode=mode)
    finally:
        ce.plt = keep
    assert len(rec.images) == len(rec.titles)
    return rec.titles, rec.images


def hexs(v):
    return [float(x).hex() for x in np.asarray(v, np.float64).reshape(-1)]


def cam_record(cam):
    return {k: {"hex": hexs(v), "dtype": str(np.asarray(v).dtype) if isinstance(v, (np.ndarray, np.generic)) else "py"} for k, v in cam.items()}


def checked(ce, grid, pc, image, cam, mode):
    """the reference's titles and images, asserted equal to the restatement; + the restatement's IoUs and outline counts"""
    titles, images = capture(ce, grid, pc, image, cam, mode)
    mine, outlines = ovr.overlays(grid, pc, image, cam, mode)
    assert [t for t, _, _ in mine] == titles, (mode, titles, [t for t, _, _ in mine])
    for (t, v, _), im in zip(mine, images):
        assert v.dtype == im.dtype == np.uint8 and np.array_equal(v, im), (mode, t)
    return mine, outlines


def stored_cameras(mon):
    from pb3d import eval_helpers_intra as ev
    cams = {}
    for stage in ("init", "kp", "final"):
        path = os.path.join(GOLDEN, f"stored_{mon}_camera_params_{stage}.json")
        for view in json.load(open(path)):              # the keypoint stage stores only the views that had keypoints
            if view in ("front", "drone"):
                cams[(stage, view)] = ev.load_camera_json(path, view)
    return cams


def stored_mask(mon, view, grid):
    from pb3d import eval_helpers_intra as ev
    with redirect_stdout(io.StringIO()):
        return np.ascontiguousarray(ev.resize_mask_to_voxel_grid(ev.load_mask(os.path.join(GOLDEN, f"data_{mon}_{view}_mask.png")), grid)[:, :, :3])


def stand_in_skimage():
    """label (8-connected, raster numbering) and regionprops (label, area, centroid) for extract_minaret_masks_by_label"""
    from scipy.ndimage import label as nd_label

    def label(mask):
        return nd_label(np.asarray(mask) != 0, structure=np.ones((3, 3)))[0]

    class Region:
        def __init__(self, lab, k):
            ys, xs = np.nonzero(lab == k)
            self.label, self.area, self.centroid = k, len(ys), (ys.mean(), xs.mean())

    def regionprops(lab):
        return [Region(lab, k) for k in range(1, int(lab.max()) + 1)]
    return label, regionprops


class _PtpArray(np.ndarray):        # ndarray.ptp left NumPy 2; the reference still calls it (tools/gen_golden_minarets.py)
    def ptp(self, axis=None):
        return np.ptp(np.asarray(self), axis=axis)


def main():
    vc, vu, pu, cg, ce, cfg = ref_import.load_reference()
    PC = cfg.PART_COLORS

    # ---- small synthetic cases: full images ---------------------------------------------------------------------------------------
    arrays, meta = {}, {}
    for name, (grid, pc, image, cam) in ovr.synthetic_cases().items():
        arrays[f"{name}/grid"] = grid; arrays[f"{name}/image"] = image
        meta[name] = {"part_colors": {k: [int(x) for x in v] for k, v in pc.items()}, "cam": cam_record(cam), "modes": {}}
        for mode in MODES:
            mine, outlines = checked(ce, grid, pc, image, cam, mode)
            for i, (t, v, _) in enumerate(mine):
                arrays[f"{name}/{mode}/{i}"] = v
            meta[name]["modes"][mode] = {"titles": [t for t, _, _ in mine], "iou": [None if i is None else float(i).hex() for _, _, i in mine],
                                         "outline_pixels": outlines}
        try:
            capture(ce, grid, pc, image, cam, "part_on_part")
            raise AssertionError("part_on_part ran")
        except NameError as e:
            meta[name]["part_on_part"] = str(e)
            assert str(e) == "name 'proj_f' is not defined"
        n, lo, hi = ovr.bounds(grid, [c for c in pc.values() if max(c) <= 255 and any(c)])
        pts = vu.get_voxel_points_by_parts(grid, pc, [k for k, c in pc.items() if max(c) <= 255 and any(c)])[0]
        assert n == len(pts) and np.array_equal(pts.min(0), lo[::-1]) and np.array_equal(pts.max(0), hi[::-1])
    np.savez_compressed(os.path.join(GOLDEN, "overlay_synth.npz"), **arrays)
    json.dump(meta, open(os.path.join(GOLDEN, "overlay_synth.json"), "w"), indent=1)

    # ---- the stored Akbar grid under its six stored cameras: digests -----------------------------------------------------------------
    grid = np.load(os.path.join(GOLDEN, "stored_Akbar_voxel_grid.npz"))["voxel_grid"]
    dig = {}
    for (stage, view), cam in stored_cameras("Akbar").items():
        image = stored_mask("Akbar", view, grid)
        rec = {}
        for mode in MODES:
            mine, outlines = checked(ce, grid, PC, image, cam, mode)
            rec[mode] = {"titles": [t for t, _, _ in mine], "sha256": [sha(v) for _, v, _ in mine],
                         "iou": [None if i is None else float(i).hex() for _, _, i in mine], "outline_pixels": outlines}
        dig[f"{stage}_{view}"] = rec
        print("Akbar", stage, view, rec["whole_on_whole"]["titles"], file=sys.stderr)
    json.dump({"shape": list(grid.shape), "cameras": dig}, open(os.path.join(GOLDEN, "overlay_akbar.json"), "w"), indent=1)

    # ---- bbox init and keypoint fit on Akbar and Bibi -------------------------------------------------------------------------------
    import utils.camera_estimation as ce_mod
    ce_mod.label2d, ce_mod.regionprops = stand_in_skimage()
    minaret_colors = [PC["front_minarets"], PC["back_minarets"]]
    out = {}
    for mon in ("Akbar", "Bibi"):
        grid = np.load(os.path.join(GOLDEN, f"stored_{mon}_voxel_grid.npz"))["voxel_grid"]
        out[mon] = {}
        for view in ("front", "drone"):
            image = stored_mask(mon, view, grid)
            rec = {"inits": {}}
            for parts in (["plinth", "front_minarets", "back_minarets"], ["dome"], list(PC)):
                try:
                    with redirect_stdout(io.StringIO()) as so:
                        init = ce.auto_compute_initial_params_matching_bbox(grid, image, PC, parts, fov_deg=30)
                except ValueError as e:                     # no voxel or no pixel of these parts
                    rec["inits"][",".join(parts)] = {"error": str(e)}
                    continue
                n, lo, hi = ovr.bounds(grid, [PC[p] for p in parts])
                ys, xs = np.where(np.any(np.isin(ovr_keys(image), [key(PC[p]) for p in parts])[..., None], axis=-1))
                rec["inits"][",".join(parts)] = {"count": int(n), "lo": [int(v) for v in lo], "hi": [int(v) for v in hi],
                                                 "img_bbox": [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())],
                                                 "H": int(image.shape[0]), "W": int(image.shape[1]), "params": cam_record(init),
                                                 "prints": so.getvalue()}
            argwhere = np.argwhere
            np.argwhere = lambda *a, **k: argwhere(*a, **k).view(_PtpArray)
            try:
                vk, ik = ce.extract_minaret_kps_for_view(grid, image, minaret_colors)
            except ValueError as e:
                rec["fit"] = None
                print(mon, view, "no keypoints:", e, file=sys.stderr)
                out[mon][view] = rec
                continue
            finally:
                np.argwhere = argwhere
            with redirect_stdout(io.StringIO()):
                init = ce.auto_compute_initial_params_matching_bbox(grid, image, PC, ["plinth", "front_minarets", "back_minarets"])
            fit = {"keys": list(ik), "voxel_kps": {k: hexs(v) for k, v in vk.items()}, "image_kps": {k: hexs(v) for k, v in ik.items()},
                   "init": "plinth,front_minarets,back_minarets", "x": {}}
            for loss in ("L2", "L1"):
                keep = {k: np.array(v, copy=True) for k, v in vk.items()}
                with redirect_stdout(io.StringIO()):
                    final = ce.optimize_camera_with_keypoints(vk, ik, image, init, loss_type=loss)
                assert all(np.array_equal(keep[k], vk[k]) for k in vk)
                fit["x"][loss] = hexs(list(final["cam_pos"]) + list(final["target"]) + [final["f"], final["cx"], final["cy"]])
            rec["fit"] = fit
            out[mon][view] = rec
            print(mon, view, "fit", [float.fromhex(h) for h in fit["x"]["L2"]][:3], file=sys.stderr)
    json.dump(out, open(os.path.join(GOLDEN, "overlay_init_fit.json"), "w"), indent=1)


def key(c):
    return int(c[0]) | (int(c[1]) << 8) | (int(c[2]) << 16)


def ovr_keys(image):
    im = image.astype(np.uint32)
    return im[..., 0] | (im[..., 1] << 8) | (im[..., 2] << 16)


if __name__ == "__main__":
    main()
