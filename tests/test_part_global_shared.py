"""part_carve and global_carve on RGB and on 1-byte label grids run ONE job loop and ONE composed global carve (csrc/carve.hip, kernels
templated on the bytes per voxel; the apply pass keeps a 1-byte kernel of its own behind the shared routine): every branch of that
loop and the composed pipeline, both forms, on small and ragged shapes, byte for byte against the CPU oracle."""
import functools

import numpy as np
import pytest

NAMES = ["full_building", "chhatris", "plinth", "front_minarets", "small_minarets", "dome"]
# test_gpu_parity.py's JOBS_MIXED: the fused sweep of the 90-degree jobs, then the other two merged into it
JOBS_MIXED = [(["full_building", "plinth"], 90), (["chhatris"], 45), (["dome"], 60), (["front_minarets", "small_minarets"], 90)]

# (W, H, D)
SHAPES = [(16, 3, 17), (48, 2, 21),                 # D >= 16, D % 16 != 0, nvox % 16 == 0: the merged pass with groups that straddle two columns
          (21, 2, 19), (17, 5, 17), (37, 9, 51),    # D >= 16, nvox % 16 != 0: per-job 16-voxel kernels plus the scalar tail (14, 5, 7 voxels)
          (33, 3, 16), (16, 7, 48),                 # whole groups, one or three per column
          (5, 3, 7)]                                # D < 16: scalar kernels only
DENSITIES = (0.3, 0.9)

JOBS_TWO = [(["full_building", "plinth"], 45), (["chhatris", "dome"], 60)]          # no 90-degree job: no fused base, the final pass
JOBS_NINE = [([n], a) for n, a in zip(NAMES, (45, 60, 30, 45, 60, 30))] + [(["dome"], 15), (["plinth"], 20), (["chhatris"], 75)]   # past the eight-job merged pass
JOBS_SKIPPED = [(["windows"], 45)]                                                  # the mask holds no such colour: every job skipped
JOBS_33 = [([NAMES[j % 6]], 90) for j in range(33)]                                 # njobs > 32: no fused sweep
JOB_LISTS = {"mixed": JOBS_MIXED, "two": JOBS_TWO, "nine": JOBS_NINE, "skipped": JOBS_SKIPPED}


@functools.lru_cache(maxsize=None)
def _inputs():
    """{(shape, density): (ids (W,H,D) labels 0..6, mask (H,W) labels 0..6)}, drawn in this order from one generator"""
    rng = np.random.default_rng(7)
    out = {}
    for (W, H, D) in SHAPES:
        for dens in DENSITIES:
            ids = (rng.integers(1, 7, (W, H, D)) * (rng.random((W, H, D)) < dens)).astype(np.uint8)
            mask = rng.integers(0, 7, (H, W)).astype(np.uint8)
            out[((W, H, D), dens)] = (ids, mask)
    return out


def _palette(pb3d_gpu, oracle):
    names = NAMES + ["windows"]                     # label 7: in the palette so that the skipped job can name it, in no grid or mask
    return pb3d_gpu.Palette([oracle.PART_COLORS[n] for n in names], names)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_part_carve_rgb_and_labels_every_branch(pb3d_gpu, oracle, shape):
    """Fused 90-degree sweep then merge (mixed), final pass without a fused base (two), job by job past eight merged jobs (nine), the
    all-skipped memset of nvox * C bytes, more than 32 jobs; each also with knob per_job = 1 (no fused sweep, no merged pass)."""
    lpal = _palette(pb3d_gpu, oracle)
    tab = lpal.table()
    lists = dict(JOB_LISTS, **({"33 x 90": JOBS_33} if shape == (16, 3, 17) else {}))
    for dens in DENSITIES:
        ids, mask = _inputs()[(shape, dens)]
        colored, sem = tab[ids], tab[mask]
        for name, jobs in lists.items():
            want = oracle.part_carve(colored, sem, jobs)
            kept, held = int(want.any(axis=-1).sum()), int((ids != 0).sum())
            if name == "skipped":
                assert kept == 0, (shape, dens, name)
            elif dens == 0.9:       # a kernel that zeroes or copies everything cannot pass
                assert 1 <= kept < held, (shape, dens, name, kept, held)
            for per_job in (0, 1):
                pb3d_gpu._lib.set_tuning("per_job", per_job)
                try:
                    got = pb3d_gpu.part_carve(colored, sem, jobs)
                    got_l = pb3d_gpu.part_carve_labels(ids, mask, jobs, lpal)
                finally:
                    pb3d_gpu._lib.set_tuning("per_job", 0)
                assert np.array_equal(got, want), (shape, dens, name, per_job, "rgb", int((got != want).sum()))
                got_l = pb3d_gpu.label_to_rgb(got_l, lpal)
                assert np.array_equal(got_l, want), (shape, dens, name, per_job, "labels", int((got_l != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(3, 7), (5, 17), (4, 16), (2, 33), (6, 40)], ids=lambda s: "x".join(map(str, s)))   # D < 16, straddling groups, exact groups, a tail
def test_global_carve_labels_composed_small_and_ragged(pb3d_gpu, oracle, hw):
    """global_carve at angle steps other than 90 on a label image (ones -> process -> apply, the RGB form's composed routine with
    k_label_apply16 as its last pass) and the RGB form's own composed pipeline (knob global_composed = 1)."""
    h, w = hw
    lpal = _palette(pb3d_gpu, oracle)
    tab = lpal.table()
    rng = np.random.default_rng([7, h, w])
    for ai in (45, 30):
        lab = (rng.integers(1, 7, (h, w)) * (rng.random((h, w)) < 0.6)).astype(np.uint8)
        binary = (lab != 0).astype(np.uint8)
        want = oracle.global_carve(binary, tab[lab], ai)
        kept = int(want.any(axis=-1).sum())
        assert 0 < kept < w * h * w, (h, w, ai, kept)
        got_l = pb3d_gpu.label_to_rgb(pb3d_gpu.global_carve_labels(binary, lab, ai), lpal)
        assert np.array_equal(got_l, want), (h, w, ai, "labels", int((got_l != want).sum()))
        pb3d_gpu._lib.set_tuning("global_composed", 1)
        try:
            got = pb3d_gpu.global_carve(binary, tab[lab], ai)
        finally:
            pb3d_gpu._lib.set_tuning("global_composed", 0)
        assert np.array_equal(got, want), (h, w, ai, "rgb, composed", int((got != want).sum()))
