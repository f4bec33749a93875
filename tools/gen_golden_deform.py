"""Golden vectors of the notebook-3 deformation closures on the constructed edge cases of tests/deform_restate.py (rounding ties,
sign(0), fused multiply-add and float32 sensitive clouds, rounded means, duplicates, bounds, paint order), captured by driving
launch_deform_viewer_fixed_camera headlessly as tools/gen_golden_f8.py does (THIS CONTAINER ONLY).

Every case is checked against the restatement before anything is written: the closure's unique rows, save_params' IoU and
save_deformed_grid's grid must equal deform_restate's."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "part-based-3d-reconstruction_amd")):
    sys.path.insert(0, p)
import ref_widgets  # noqa: E402

ref_widgets.install()
import ref_import  # noqa: E402  (its ipywidgets/IPython stubs are skipped: already registered above)

sys.modules.setdefault("cv2", None)
_orig_stub = ref_import._stub


def _keep_widgets(name, **attrs):
    if name in ("ipywidgets", "IPython", "IPython.display"):
        return sys.modules[name]
    return _orig_stub(name, **attrs)


ref_import._stub = _keep_widgets
del sys.modules["cv2"]
vc, vu, pu, cg, ce, cfg = ref_import.load_reference()
import matplotlib.pyplot as plt  # noqa: E402
plt.show = lambda *a, **k: None
import utils.deformation_estimation as de  # noqa: E402

import deform_restate as dr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def launch(scene):
    """(saved_params, grid store, sliders, save button, save-grid button, the deform_coords closure) of a viewer on `scene`"""
    ref_widgets.install()
    saved, store = de.launch_deform_viewer_fixed_camera(scene["grid"], scene["labels"], image=scene["image"], cam_params=scene["cam"],
                                                        part_names=list(scene["labels"]))
    S, B = ref_widgets.CREATED["sliders"], ref_widgets.CREATED["buttons"]
    return saved, store, S, B[0], B[1], ref_widgets.closure_of(B[0]._clicks[0], "deform_coords")


arrays, meta = {}, {"clouds": {}, "scenes": {}}
all_scenes = dr.scenes()

# ---- clouds through the raw closure ---------------------------------------------------------------------------------------------------
closure = launch(all_scenes["ties"])[5]
for name, c in dr.cloud_cases().items():
    got = closure(c["pts"].copy(), c["image_shape"], c["voxel_shape"], c["deform"])
    want = dr.deform_coords(c["pts"], c["image_shape"], c["voxel_shape"], c["deform"])
    assert got.dtype == np.int64 and np.array_equal(got, want), name
    if c["kind"] == "fma":
        assert not np.array_equal(got, dr.deform_coords(c["pts"], c["image_shape"], c["voxel_shape"], c["deform"], "fma")), name
    arrays[f"cloud/{name}/pts"] = c["pts"]
    arrays[f"cloud/{name}/coords"] = got
    meta["clouds"][name] = {"image_shape": list(c["image_shape"]), "voxel_shape": list(c["voxel_shape"]), "deform": dr.deform_record(c["deform"]),
                            "kind": c["kind"]}

# ---- scenes through save_params and save_deformed_grid ----------------------------------------------------------------------------------
for name, sc in all_scenes.items():
    saved, store, S, save_btn, save_grid_btn, closure = launch(sc)
    shape, ishape = sc["grid"].shape[:3], sc["image"].shape[:2]
    rec = {"labels": [[p, list(c)] for p, c in sc["labels"].items()], "cam": dr.cam_record(sc["cam"]),
           "saved": {p: dr.deform_record(d) for p, d in sc["saved"].items()}, "iou": {}}
    for part, d in sc["saved"].items():
        S["Part"].set_silently(part)
        for k, v in d.items():
            S[k].set_silently(v)
        save_btn.click()
        assert saved[part]["deform"] == d
        pts, _ = vu.get_voxel_points_by_parts(sc["grid"], sc["labels"], [part])
        rows = closure(pts.copy(), ishape, shape, d)
        rpts, _ = dr.part_points(sc["grid"], sc["labels"], part)
        assert np.array_equal(pts, rpts) and np.array_equal(rows, dr.deform_coords(rpts, ishape, shape, d)), (name, part)
        inter, uni, _ = dr.iou_counts(rpts, shape, d, sc["image"], sc["cam"], sc["labels"][part])
        assert float(saved[part]["iou"]) == dr.iou(inter, uni), (name, part, saved[part]["iou"], inter, uni)
        arrays[f"scene/{name}/coords/{part}"] = rows
        rec["iou"][part] = float(saved[part]["iou"]).hex()
    save_grid_btn.click()
    full = store["grid"]
    assert np.array_equal(full, dr.build_deformed_grid(sc["grid"], sc["labels"], {p: {"deform": d} for p, d in sc["saved"].items()}, ishape)), name
    arrays[f"scene/{name}/grid"] = sc["grid"]
    arrays[f"scene/{name}/image"] = sc["image"]
    arrays[f"scene/{name}/out"] = full
    meta["scenes"][name] = rec

np.savez_compressed(os.path.join(OUT, "deform_edges.npz"), **arrays)
json.dump(meta, open(os.path.join(OUT, "deform_edges.json"), "w"), indent=1)
print(len(meta["clouds"]), "clouds,", len(meta["scenes"]), "scenes; KB",
      os.path.getsize(os.path.join(OUT, "deform_edges.npz")) / 1024, os.path.getsize(os.path.join(OUT, "deform_edges.json")) / 1024)
