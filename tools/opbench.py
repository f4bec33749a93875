"""Device-resident timing of every op of the path (M1..M8 of SURVEY.md 8(d), plus the N1/N2 kernels of the notebook-1 chain) on
synthetic inputs.  Development/measurement tool: python tools/opbench.py [--size 1024] [--shape WxHxD] [--ops M1,M3,...,N2,overlays,ICP,PLANE,MESHD,CLUSTER,DOWNSAMPLE,SMOOTH,SIMPLIFY,VOXELIZE,EDT,RENDER,ISO,MESHCOMP,ORIENT,WELD,INSIDE,RAYCAST]; one JSON
line per op.  Pricing: `alg_B_per_voxel` is SURVEY 8(d)'s algorithmic figure for the sweeps that are EXECUTED (a folded 0-degree step
moves nothing and is not priced); ops whose intermediates are not bytes (the bit-sliced chains) also carry `moved_B_per_voxel`, the
bytes that cross the HBM by design, and their `frac_of_8TBs` is computed from THAT (never from bytes that are not moved)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "part-based-3d-reconstruction_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

import pb3d  # noqa: E402
from pb3d import device as dev  # noqa: E402

PEAK = 8000.0


def timeit(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    dev.sync()
    e0, e1 = dev.Event(), dev.Event()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    return e1.elapsed_ms_since(e0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--ops", default="M1,M2,M3,M4,M5,M6,M7,M8,A2,A6,A9,N2,TK")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tune", default="", help="development knobs, e.g. rot90_fill=6 (pb3d_set_tuning)")
    ap.add_argument("--no-cpu-ref", action="store_true", help="I5: skip the cKDTree timings of the same inputs")
    a = ap.parse_args()
    for kv in [t for t in a.tune.split(',') if t]:
        pb3d._lib.set_tuning(kv.split('=')[0], int(kv.split('=')[1]))
    S = a.size
    nvox = S ** 3
    ops = a.ops.split(",")
    lib, L = pb3d._lib.load(), pb3d._lib
    d_mwh = dev.DeviceBuffer(S * S); d_bhw = dev.DeviceBuffer(S * S); d_rgb = dev.DeviceBuffer(S * S * 3)
    dev.synth_mask16(S, d_binary_hw=d_bhw, d_rgb_hw3=d_rgb, d_binary_wh=d_mwh)
    res = []

    def report(op, name, ms, bpv, extra=None):
        r = {"op": op, "name": name, "size": S, "ms": round(ms, 4), "Mvoxel_s": round(nvox / ms / 1e3, 1),
             "alg_B_per_voxel": bpv, "alg_GB_s": round(bpv * nvox / ms / 1e6, 1), "frac_of_8TBs": round(bpv * nvox / ms / 1e6 / PEAK, 4)}
        if extra:
            r.update(extra)
        print(json.dumps(r), flush=True)
        res.append(r)

    if "M1" in ops:
        d_in = dev.DeviceBuffer(nvox * 3); d_out = dev.DeviceBuffer(nvox * 3)
        dev.synth_sem(0, S, S, S, 1, d_in)
        report("M1", "carve_voxel_grid_with_masks(sem,binary)", timeit(lambda: dev.carve_mask(d_in, S, S, S, 3, d_mwh, d_out), 20), 6)
        for parts in (2, 4, 8):      # what one rank of an N-GPU run does (X-slab of S/N planes); ideal = ms(M1) / N
            ms = timeit(lambda: dev.carve_mask(d_in, S // parts, S, S, 3, d_mwh, d_out), 50)
            print(json.dumps({"op": "M1/slab", "planes": S // parts, "ms": round(ms, 4), "alg_GB_s": round(6 * nvox / parts / ms / 1e6, 1)}), flush=True)
        d_in.free(); d_out.free()
    if "A2" in ops or "A6" in ops:      # the two elementwise helpers of the path (not in SURVEY's M list): 4 B/voxel each
        d_c = dev.DeviceBuffer(nvox * 3); d_o = dev.DeviceBuffer(nvox); d_o2 = dev.DeviceBuffer(nvox)
        dev.synth_sem(0, S, S, S, 1, d_c)
        report("A2", "_occupancy(rgb grid)", timeit(lambda: dev.occupancy(d_c, nvox, d_o), 10), 4)
        dev.carve_mask(d_o, S, S, S, 1, d_mwh, d_o2)
        report("A6", "apply_colored_mask_to_voxel_grid", timeit(lambda: dev.color_apply(d_o2, S, S, S, d_rgb, d_c), 10), 4)
        d_c.free(); d_o.free(); d_o2.free()
    d_occ = dev.DeviceBuffer(nvox); d_o1 = dev.DeviceBuffer(nvox); d_tmp = dev.DeviceBuffer(nvox)
    dev.synth_occ(0, S, S, S, 0, d_occ)
    if "M2" in ops:
        report("M2", "carve_voxel_grid_with_masks(occ,binary)", timeit(lambda: dev.carve_mask(d_occ, S, S, S, 1, d_mwh, d_o1), 20), 2)
    if "M3" in ops:
        report("M3", "process_voxel_grid(occ,binary,90)", timeit(lambda: dev.process_grid(d_occ, S, S, S, d_mwh, 90, d_o1, d_tmp), a.reps), 2)
    if "M3" in ops:
        for ai in (45, 60, 30, 5):     # chained: len(range(0, 91, ai)) steps; the 0-degree carve is folded (it moves nothing): 90 // ai sweeps
            nrot = 90 // ai
            ms = timeit(lambda: dev.process_grid(d_occ, S, S, S, d_mwh, ai, d_o1, d_tmp), a.reps)
            # two and more rotation steps run bit-sliced (csrc/sliced.hip): 1 B in, 1/8 out; nrot x (1/8 + 1/8); 1/8 in, 1 B out
            moved = 2.0 * nrot if nrot < 2 else 2.25 + 0.25 * nrot
            r = {"op": "M3+", "name": f"process_voxel_grid(occ,binary,{ai}): {nrot} rotation sweeps (0 deg folded)", "size": S, "ms": round(ms, 4),
                 "ms_per_sweep": round(ms / nrot, 4), "alg_B_per_voxel": 2 * nrot, "alg_GB_s": round(2 * nrot * nvox / ms / 1e6, 1),
                 "moved_B_per_voxel": moved, "moved_GB_s": round(moved * nvox / ms / 1e6, 1), "frac_of_8TBs": round(moved * nvox / ms / 1e6 / PEAK, 4)}
            print(json.dumps(r), flush=True)
    if "M4" in ops:
        M = np.empty(9); off = np.empty(3)
        for ang in (45, 5):
            L.check(lib.pb3d_rotinv(ang, L.p_dbl(M))); L.check(lib.pb3d_offset(L.p_dbl(M), (C.c_int64 * 3)(S, S, S), L.p_dbl(off)))
            report("M4", f"one rotate+carve step, {ang} deg", timeit(lambda: dev.rotate_carve(d_occ, S, S, S, M, off, d_mwh, d_o1), a.reps), 2)
    d_occ.free(); d_o1.free(); d_tmp.free()
    d_col = None
    if any(o in ops for o in ("M5", "M6", "M7", "M8", "A9", "N2", "TK")):
        d_col = dev.DeviceBuffer(nvox * 3)
        ms = timeit(lambda: dev.global_carve(d_bhw, d_rgb, S, S, 90, d_col), a.reps)
        if "M5" in ops:
            report("M5", "global_carve(binary,rgb,90)", ms, 3)
            for ai in (45, 60):
                report("M5+", f"global_carve(binary,rgb,{ai})", timeit(lambda: dev.global_carve(d_bhw, d_rgb, S, S, ai, d_col), a.reps), 3)
            dev.global_carve(d_bhw, d_rgb, S, S, 90, d_col)
    if "M6" in ops:
        # six 90-degree part jobs of notebook 1 on the structured grid (labels 1..9 of the synthetic mask are the part colours)
        import synth_host
        lab, binary, rgb = synth_host.mask16(S)
        names = ["full_building", "chhatris", "plinth", "front_minarets", "small_minarets", "dome"]
        msub = np.zeros((len(names), S, S), np.uint8)
        for j, nm in enumerate(names):
            msub[j] = np.all(rgb == np.array(pb3d.PART_COLORS[nm], np.uint8), axis=-1).T
        mcarve = np.ascontiguousarray(msub.transpose(0, 2, 1))      # W == H: _mask_to_wh transposes again
        d_ms = dev.from_numpy(msub); d_mc = dev.from_numpy(mcarve); d_out = dev.DeviceBuffer(nvox * 3)
        ang = (C.c_int * 6)(*([90] * 6)); skip = (C.c_int * 6)(*[0 if msub[j].any() else 1 for j in range(6)])
        fn = lambda: L.check(lib.pb3d_part_carve_dev(L.ctx(), C.c_void_p(d_col.ptr), S, S, S, C.c_void_p(d_ms.ptr), C.c_void_p(d_mc.ptr),
                                                      ang, skip, 6, C.c_void_p(d_out.ptr)))
        ms = timeit(fn, max(2, a.reps // 2), warm=1)
        # the six jobs run as ONE fused sweep (k_part90): it owes a read of the colour grid as occupancy source (3 B), a read of
        # the kept rows as output source (<= 3 B) and the write (3 B) -- <= 9 B/voxel whatever the number of jobs.  (SURVEY's
        # 6 B/voxel PER JOB prices the reference's job-by-job execution, which this sweep does not perform.)
        # priced at what the sweep really moves (PMC, profiles/r02_opbench_pmc_traffic.json: 3.26 GB read + 3.22 GB written = 6.0 B/voxel;
        # an upper bound of 9 B/voxel flattered the figure in round 2)
        report("M6", "part_carve, six 90-degree jobs (one fused sweep)", ms, 6, {"jobs": 6, "ms_per_job": round(ms / 6, 4),
                                                                                 "reference_execution_B_per_voxel": 36})
        for b in (d_ms, d_mc, d_out):
            b.free()
    if "A9" in ops:
        # connected components of one part colour on the carved 1024^3 colour grid (left_right_guided_carve / recolor set-up):
        # label + per-component statistics; labels are int32 (4 B/voxel written), the grid is read once (3 B/voxel)
        col = np.array(pb3d.PART_COLORS["full_building"], np.uint8)
        d_lab = dev.DeviceBuffer(nvox * 4)
        ncomp = C.c_int64(0)
        lab_fn = lambda: L.check(lib.pb3d_label_color_dev(L.ctx(), C.c_void_p(d_col.ptr), S, S, S, L.p_u8(col), C.c_void_p(d_lab.ptr), C.byref(ncomp)))
        ms = timeit(lab_fn, 2, warm=1)
        report("A9", "connected components of one colour (label)", ms, 7, {"components": ncomp.value})
        nc = max(1, ncomp.value)
        bbox = (C.c_int64 * (6 * nc))(); cnt = (C.c_int64 * nc)(); csum = (C.c_int64 * (3 * nc))()
        st_fn = lambda: L.check(lib.pb3d_component_stats_dev(L.ctx(), C.c_void_p(d_lab.ptr), S, S, S, ncomp.value, bbox, cnt, csum))
        report("A9", "component statistics (bbox, count, coordinate sums)", timeit(st_fn, 2, warm=1), 4)
        d_lab.free()
    if "N2" in ops:
        # the N1 / N2 kernels of the notebook-1 chain on the carved colour grid: orientation (transpose + flip: 3 B read, 3 B written),
        # the four in-place extrusions (a column scan reads at most the 3 B/voxel it crosses and writes `depth` cells), labelling WITH the
        # component statistics (3 B read + 4 B of int32 labels written), recolouring (4 B of labels read, flagged voxels written)
        d_o = dev.DeviceBuffer(nvox * 3)
        report("N2", "orient (transpose(2,1,0,3) + flip)", timeit(lambda: L.check(lib.pb3d_orient_dev(L.ctx(), C.c_void_p(d_col.ptr), S, S, S, C.c_void_p(d_o.ptr))), a.reps), 6)
        d_v = dev.DeviceBuffer(S * S)
        L.check(lib.pb3d_dev_memset(L.ctx(), C.c_void_p(d_v.ptr), 1, S * S))
        fc = np.array(pb3d.PART_COLORS["windows"], np.uint8)
        for axis, nm in ((2, "z"), (0, "x")):
            for plus in (1, 0):
                fn = lambda: L.check(lib.pb3d_extrude_dev(L.ctx(), C.c_void_p(d_o.ptr), S, S, S, C.c_void_p(d_v.ptr), S, axis, plus, 10, L.p_u8(fc), C.c_void_p(d_o.ptr)))
                # the bytes an extrusion needs depend on the data (a column is scanned up to its first occupied voxel, then `depth` cells are
                # written): no algorithmic-byte figure, the time only
                ms = timeit(fn, a.reps)
                print(json.dumps({"op": "N2", "name": f"extrude_from_surface axis {axis} {'+' if plus else '-'} depth 10, in place (k_extrude_{nm})", "size": S,
                                  "ms": round(ms, 4), "alg_B_per_voxel": None, "note": "data-dependent traffic: scan to the first occupied voxel of every column under the mask"}), flush=True)
        from pb3d.voxel_carving_utils import _label_stats
        col = np.array(pb3d.PART_COLORS["full_building"], np.uint8)
        d_lab = dev.DeviceBuffer(nvox * 4)
        out = {}
        def lab_fn():
            out["n"] = _label_stats(d_col, (S, S, S), col, d_lab)[0]
        report("N2", "connected components of one colour + statistics (one pass, one round trip)", timeit(lab_fn, 2, warm=1), 7, {"components": out["n"]})
        def lab_fn2():
            out["n"] = _label_stats(d_col, (S, S, S), col, d_lab, members_only=True)[0]
        members = int(np.count_nonzero(np.all(dev.DeviceGrid(d_col, (S, S, S, 3)).numpy() == col, axis=-1))) if S <= 512 else None
        report("N2", "... labels written for the colour's voxels only (members_only: what the notebook-1 chain uses)", timeit(lab_fn2, 2, warm=1), 3,
               {"components": out["n"], "member_voxels": members, "note": "3 B/voxel read + 4 B per MEMBER voxel written (not priced)"})
        lab_fn()
        flags = np.ones(max(1, out["n"]), np.uint8)
        fn = lambda: L.check(lib.pb3d_recolor_components_dev(L.ctx(), C.c_void_p(d_lab.ptr), nvox, L.p_u8(flags), max(1, out["n"]), L.p_u8(fc), C.c_void_p(d_o.ptr)))
        report("N2", "recolor_backward_components: recolour pass over the label volume (k_recolor_flagged)", timeit(fn, 2, warm=1), 4)
        fn2 = lambda: L.check(lib.pb3d_recolor_last_labelled_dev(L.ctx(), C.c_void_p(d_lab.ptr), nvox, L.p_u8(flags), max(1, out["n"]), L.p_u8(fc), C.c_void_p(d_o.ptr), 3))
        ms = timeit(fn2, 2, warm=1)
        print(json.dumps({"op": "N2", "name": "recolor_backward_components: recolour pass over the labelling's membership bits (k_recolor_bits)", "size": S, "ms": round(ms, 4),
                          "alg_B_per_voxel": 0.125, "note": "1 bit/voxel read + 4 B label and 3 B colour per member voxel"}), flush=True)
        for b in (d_o, d_v, d_lab):
            b.free()
    if "TK" in ops:
        # extract_top_k_components (reference utils/voxel_utils.py:24-33) on the carved colour grid: the 26-connected labelling of one
        # colour, members only (3 B/voxel read; labels written at the member voxels, not priced), against the 6-connected one; then the
        # whole in-place op (labelling + ranking + zeroing over the membership bits: 3 B/voxel + the members' bytes, not priced)
        from pb3d.voxel_utils import _label_stats_conn
        col = np.array(pb3d.PART_COLORS["full_building"], np.uint8)
        d_lab = dev.DeviceBuffer(nvox * 4)
        out = {}
        for conn in (6, 26):
            def lab_conn():
                out["n"] = _label_stats_conn(d_col, (S, S, S), [col], d_lab, conn, members_only=True)[0][0]
            report("TK", f"connected components of one colour, {conn}-connected, members only (+ statistics)", timeit(lab_conn, a.reps, warm=1), 3,
                   {"components": out["n"], "connectivity": conn})
        d_g = dev.DeviceBuffer(nvox * 3); d_st = dev.DeviceBuffer(16)
        L.check(lib.pb3d_d2d(L.ctx(), C.c_void_p(d_g.ptr), C.c_void_p(d_col.ptr), nvox * 3))
        # in place on a copy: the first call zeroes what k = 4 drops, the later ones find the same components minus those (same work)
        tk = lambda: L.check(lib.pb3d_top_k_components_dev(L.ctx(), C.c_void_p(d_g.ptr), S, S, S, L.p_u8(col), 3, 4, 26, C.c_void_p(d_lab.ptr), C.c_void_p(d_st.ptr)))
        ms = timeit(tk, a.reps, warm=1)
        report("TK", "extract_top_k_components(k=4), in place on the device (pb3d_top_k_components_dev)", ms, 3,
               {"components": int(d_st.download((2,), np.int64)[0])})
        for b in (d_lab, d_g, d_st):
            b.free()
    if "M7" in ops or "M8" in ops:
        cols = np.ascontiguousarray(np.array(list(pb3d.PART_COLORS.values()), np.uint8))
        n = C.c_int64(0)
        cnt = lambda: L.check(lib.pb3d_points_count_dev(L.ctx(), C.c_void_p(d_col.ptr), S, S, S, 3, L.p_u8(cols), len(cols), 1, C.byref(n)))
        cnt()
        npts = n.value
        d_pts = dev.DeviceBuffer(max(1, npts) * 12); d_pc = dev.DeviceBuffer(max(1, npts) * 3)
        fill = lambda: L.check(lib.pb3d_points_fill_dev(L.ctx(), C.c_void_p(d_col.ptr), S, S, S, 3, L.p_u8(cols), len(cols), 1, npts,
                                                        C.c_void_p(d_pts.ptr), C.c_void_p(d_pc.ptr)))
        def both():
            cnt(); fill()
        ms = timeit(both, max(2, a.reps // 2), warm=1)
        fillfrac = npts / nvox
        if "M7" in ops:
            ms_fill = timeit(fill, max(3, a.reps), warm=1)          # the fill pass alone (the scanned offsets of the last count stay in the context)
            ms_cnt = timeit(cnt, max(3, a.reps), warm=1)            # the count pass alone, with its host round trip
            report("M7", "get_voxel_points_by_parts (10 parts): count + fill", ms, round(3 + 15 * fillfrac, 3),
                   {"points": npts, "fill": round(fillfrac, 4), "count_pass_ms": round(ms_cnt, 4), "fill_pass_ms": round(ms_fill, 4)})
            n1 = C.c_int64(0)
            one = lambda: L.check(lib.pb3d_points_extract_dev(L.ctx(), C.c_void_p(d_col.ptr), S, S, S, 3, L.p_u8(cols), len(cols), npts,
                                                              C.c_void_p(d_pts.ptr), C.c_void_p(d_pc.ptr), C.byref(n1)))
            ms1 = timeit(one, max(2, a.reps // 2), warm=1)
            assert n1.value == npts
            report("M7", "get_voxel_points_by_parts (10 parts): count + fill in one call (pb3d_points_extract_dev)", ms1,
                   round(3 + 15 * fillfrac, 3), {"points": npts, "fill": round(fillfrac, 4)})
        if "M8" in ops and npts:
            from pb3d.camera_geometry import look_at_rotation
            cam = np.array([S / 2, S / 2, -2.5 * S], np.float32); tgt = np.array([S / 2, S / 2, S / 2], np.float32)
            R = np.ascontiguousarray(look_at_rotation(cam, tgt), np.float64); cd = np.ascontiguousarray(cam, np.float64)
            Hi = Wi = S
            d_img = dev.DeviceBuffer(Hi * Wi * 3)
            prec = (C.c_int * 4)(0, 0, 0, 0)
            fn = lambda: L.check(lib.pb3d_project_dev(L.ctx(), C.c_void_p(d_pts.ptr), 0, C.c_void_p(d_pc.ptr), npts, L.p_dbl(R), L.p_dbl(cd),
                                                      float(1.2 * S), S / 2.0, S / 2.0, prec, Hi, Wi, C.c_void_p(d_img.ptr)))
            ms = timeit(fn, max(2, a.reps // 2), warm=1)
            # 12 B of coordinates per point are read by the point kernel; colours are only read for the <= H*W winners
            r = {"op": "M8", "name": "project_colored_voxels (f32 camera)", "size": S, "ms": round(ms, 4), "points": npts,
                 "Mpts_s": round(npts / ms / 1e3, 1), "alg_B_per_point": 12, "alg_GB_s": round(12 * npts / ms / 1e6, 1),
                 "frac_of_8TBs": round(12 * npts / ms / 1e6 / PEAK, 4)}
            print(json.dumps(r), flush=True)
            d_img.free()
        d_pts.free(); d_pc.free()
    if "MN" in ops:
        minarets(a.reps, res)
    if "N6" in ops:
        intra_eval(a.reps, res)
    if "I5" in ops:
        inter_eval(a.reps, res, cpu_ref=not a.no_cpu_ref)
    if "ICP" in ops:
        icp(a.reps, res, cpu_ref=not a.no_cpu_ref)
    if "PLANE" in ops:
        plane(a.reps, res, cpu_ref=not a.no_cpu_ref)
    if "CLUSTER" in ops:
        cluster(a.reps, res, cpu_ref=not a.no_cpu_ref)
    if "DOWNSAMPLE" in ops:
        downsample(a.reps, res, cpu_ref=not a.no_cpu_ref)
    if "SMOOTH" in ops:
        smooth(a.reps, res, cpu_ref=not a.no_cpu_ref)
    if "SIMPLIFY" in ops:
        simplify(a.reps, res, cpu_ref=not a.no_cpu_ref)
    if "VOXELIZE" in ops:
        voxelize(a.reps, res, cpu_ref=not a.no_cpu_ref)
    if "EDT" in ops:
        edt(a.reps, res, cpu_ref=not a.no_cpu_ref)
    if "RENDER" in ops:
        render(a.reps, res, cpu_ref=not a.no_cpu_ref)
    if "MESH" in ops:
        meshify(a.reps, res)
    if "DENS" in ops:
        density(a.reps, res, cpu_ref=not a.no_cpu_ref)
    if "ISO" in ops:
        isosurface(a.reps, res)
    if "MESHD" in ops:
        mesh_target(a.reps, res)
    if "MESHCOMP" in ops:
        mesh_components(a.reps, res)
    if "ORIENT" in ops or "WELD" in ops:
        mesh_repair(a.reps, res, "ORIENT" in ops, "WELD" in ops)
    if "INSIDE" in ops:
        inside(a.reps, res)
    if "RAYCAST" in ops:
        raycast(a.reps, res)
    if "overlays" in ops:
        overlays(a.reps, res)
    if d_col is not None:
        d_col.free()
    return res


def minarets(reps, res):
    """extract_minaret_voxels_by_label (reference utils/camera_estimation.py:176-216) on the stored Taj grid (512 x 278 x 512) and on a
    1024^3 grid with four tall components: the labelling of the two minaret colours (6-connected, members only, statistics, one host
    round trip) and the member pass over the four chosen boxes (pb3d_component_members_dev: coordinates; row sums only) timed apart,
    then the whole NumPy-signature call (host wall time, upload and download included)."""
    from pb3d import minarets as mn
    lib, L = pb3d._lib.load(), pb3d._lib
    colors = [pb3d.PART_COLORS["front_minarets"], pb3d.PART_COLORS["back_minarets"]]
    taj = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    S = 1024
    for name, shape3 in (("Taj 512x278x512", taj.shape[:3]), ("synthetic 1024^3, four tall components", (S, S, S))):
        nvox = int(np.prod(shape3))
        d_g = dev.DeviceBuffer(nvox * 3)
        if name.startswith("Taj"):
            d_g.upload(taj)
        else:
            d_g.zero()
            for x0, cols4 in ((100, ((100, 900, colors[0]), (800, 880, colors[1]))), (800, ((100, 860, colors[1]), (800, 840, colors[0])))):
                plane = np.zeros((S, S, 3), np.uint8)          # one (a1, a2) plane of the columns at a0 in [x0, x0 + 32)
                for z0, h, col in cols4:
                    plane[50:50 + h, z0:z0 + 32] = col
                for x in range(x0, x0 + 32):
                    d_g.upload(plane, x * S * S * 3)
        d_lab = dev.DeviceBuffer(nvox * 4)
        cols, where = mn._distinct(colors)
        labs = {}
        lab_fn = lambda: labs.__setitem__("lab", mn._Labelling(d_g, shape3, cols, d_lab, 6, 1024))
        ms_lab = timeit(lab_fn, reps, warm=1)
        lab = labs["lab"]
        sel = mn._four_minarets(lab, where)
        counts = np.array([s[3] for s in sel], np.int64)
        ccols = np.ascontiguousarray(np.stack([cols[s[0]] for s in sel]))
        labels = np.ascontiguousarray([s[1] for s in sel], np.int32)
        bbox = np.ascontiguousarray(np.stack([s[2] for s in sel]), np.int64)
        d_xyz = dev.DeviceBuffer(int(counts.sum()) * 24); d_rows = dev.DeviceBuffer(4 * 64)

        def members(outputs):
            L.check(lib.pb3d_component_members_dev(L.ctx(), C.c_void_p(d_g.ptr), *shape3, 3, C.c_void_p(d_lab.ptr), 4, L.p_u8(ccols),
                                                   labels.ctypes.data_as(C.POINTER(C.c_int32)), bbox.ctypes.data_as(L.i64p),
                                                   counts.ctypes.data_as(L.i64p), outputs, C.c_void_p(d_xyz.ptr), C.c_void_p(d_rows.ptr), None))
        ms_coords = timeit(lambda: members(1), reps, warm=1)
        ms_rows = timeit(lambda: members(2), reps, warm=1)
        box_vox = int(sum(np.prod(b[3:] - b[:3]) for b in bbox))
        r = {"op": "MN", "name": f"extract_minaret_voxels_by_label, {name}", "shape": list(shape3), "labelling_ms": round(ms_lab, 4),
             "members_coords_ms": round(ms_coords, 4), "members_rows_ms": round(ms_rows, 4), "members": int(counts.sum()),
             "box_voxels": box_vox, "box_fraction": round(box_vox / nvox, 5),
             "components": int(sum(lab.recs[ci][0] for ci in range(len(cols))))}
        if name.startswith("Taj"):
            t = []
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                pb3d.extract_minaret_voxels_by_label(taj, colors)
                t.append(time.perf_counter() - t0)
            r["numpy_api_ms"] = round(1e3 * float(np.median(t[1:])), 3)
            grid = dev.DeviceGrid(d_g, taj.shape)
            t = []
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                pb3d.extract_minaret_voxels_by_label(grid, colors)
                t.append(time.perf_counter() - t0)
            r["device_grid_api_ms"] = round(1e3 * float(np.median(t[1:])), 3)
        print(json.dumps(r), flush=True)
        res.append(r)
        for b in (d_g, d_lab, d_xyz, d_rows):
            b.free()


def intra_eval(reps, res):
    """Notebook 4's resident evaluation of one monument and camera (reference utils/eval_helpers_intra.py:605-738): (a) grid z-buffer,
    (b) visible-part bits (7 colours + any), (d) colour set + ground-truth bits, (e) the 19 IoU rows -- each timed alone, then the whole
    monument (two z-buffers, three bit passes, d, e) -- beside the point path it replaces: count + fill of the occupied points +
    pb3d_depth_buffer_dev, and count + fill + pb3d_visible_mask_dev per colour and for all occupied voxels.  Itimad's deformed grid
    (512 x 381 x 512, the largest stored) under its final front and drone cameras, and a 1024^3 synthetic semantic grid."""
    from pb3d import eval_helpers_intra as ev
    lib, L = pb3d._lib.load(), pb3d._lib
    g = os.path.join(ROOT, "tests", "golden")
    PC = pb3d.PART_COLORS
    real = ev.load_voxel_grid(os.path.join(g, "stored_Itimad_deformed_voxel_grid.npz"))
    S = 1024
    pal = [tuple(int(v) for v in c) for c in dev.synth_palette16() if c.any()][:7]
    cases = []
    for view in ("front", "drone"):
        cam = ev.load_camera_json(os.path.join(g, "stored_Itimad_camera_params_final.json"), view)
        mask = ev.resize_mask_to_voxel_grid(ev.load_mask(os.path.join(g, f"data_Itimad_{view}_mask.png")), real)
        cases.append((f"Itimad deformed {'x'.join(map(str, real.shape[:3]))}, {view}", real, cam, mask,
                      [PC[p] for p in ev.PARTS] + [PC["front_minarets"], PC["back_minarets"]]))
    rng = np.random.default_rng(0)
    smask = np.array(pal, np.uint8)[rng.integers(0, len(pal), (S // 8, S // 8))].repeat(8, 0).repeat(8, 1)
    for view, cp in (("front", [S / 2, S / 2, -1.5 * S]), ("drone", [S / 2, 2.2 * S, -1.2 * S])):
        cam = {"cam_pos": np.array(cp, np.float32), "target": np.array([S / 2, S / 2, S / 2], np.float32), "f": 1.0 * S, "cx": S / 2,
               "cy": S / 2}
        cases.append((f"synthetic {S}^3, {view}", None, cam, smask, pal))
    for name, grid, cam, mask, colours in cases:
        if grid is None:
            d_g = dev.DeviceBuffer(S ** 3 * 3)
            dev.synth_sem(0, S, S, S, 7, d_g)
            shape = (S, S, S, 3)
        else:
            d_g = dev.from_numpy(grid); shape = grid.shape
        H, W = mask.shape[:2]
        d_m = dev.from_numpy(np.ascontiguousarray(mask[:, :, :3]))
        z1, z2 = dev.DeviceBuffer(H * W * 4), dev.DeviceBuffer(H * W * 4)
        b1, b2, b3, gt = (dev.DeviceBuffer(H * W * 4) for _ in range(4))
        bm, cnt = dev.DeviceBuffer(L.PRESENCE_BYTES), dev.DeviceBuffer(19 * 16 + 8)
        rows = [(b1, 1 << (k % 5), gt, 1 << (k % 5), None, 0) for k in range(15)] + [(b1, 96, gt, 96, None, 0), (b3, 3, gt, 96, None, 0),
                                                                                      (b1, 1 << 31, gt, 1 << 31, None, 0), (b2, 1 << 31, gt, 1 << 31, None, 0)]
        a_ms = timeit(lambda: ev.depth_buffer_resident(d_g, shape, cam, H, W, out=z1), reps)
        b_ms = timeit(lambda: ev.visible_bits_resident(d_g, shape, colours, cam, z1, (H, W), H, W, out=b1), reps)

        def d_pass():
            ev.presence_resident(d_g, shape, colours, cnt.at(19 * 16), out=bm)
            ev.mask_bits_resident(d_m, H * W, colours, bm, out=gt)
        d_ms = timeit(d_pass, reps)
        e_ms = timeit(lambda: ev.iou_rows_resident(rows, H * W, cnt), reps)

        def monument():
            d_pass()
            ev.depth_buffer_resident(d_g, shape, cam, H, W, out=z1)
            ev.depth_buffer_resident(d_g, shape, cam, H, W, out=z2)
            ev.visible_bits_resident(d_g, shape, colours, cam, z1, (H, W), H, W, out=b1)
            ev.visible_bits_resident(d_g, shape, colours, cam, z2, (H, W), H, W, out=b2)
            ev.visible_bits_resident(d_g, shape, colours[5:], cam, z2, (H, W), H, W, out=b3)
            ev.iou_rows_resident(rows, H * W, cnt)
            cnt.download((19 * 2 + 1,), np.int64)
        mon_ms = timeit(monument, reps)
        # the point path: every pass extracts its points on the device first (count: one host round trip)
        _, _, R, cpos, prec = pb3d.projection_utils.camera_args(np.zeros((1, 3), np.float32), cam["cam_pos"], cam["target"], cam["f"],
                                                               cam["cx"], cam["cy"])
        n0 = C.c_int64(0)
        L.check(lib.pb3d_points_count_dev(L.ctx(), C.c_void_p(d_g.ptr), *shape[:3], 3, None, 0, 1, C.byref(n0)))
        d_pts, d_pc, d_vm = dev.DeviceBuffer(max(1, n0.value) * 12), dev.DeviceBuffer(max(1, n0.value) * 3), dev.DeviceBuffer(H * W)

        def extract(col):
            n = C.c_int64(0)
            tab = None if col is None else np.ascontiguousarray(np.array(col, np.uint8).reshape(1, 3))
            pc = None if tab is None else L.p_u8(tab)
            L.check(lib.pb3d_points_count_dev(L.ctx(), C.c_void_p(d_g.ptr), *shape[:3], 3, pc, 0 if tab is None else 1, 1, C.byref(n)))
            assert n.value * 12 <= d_pts.nbytes, "point buffer too small"
            L.check(lib.pb3d_points_fill_dev(L.ctx(), C.c_void_p(d_g.ptr), *shape[:3], 3, pc, 0 if tab is None else 1, 1, n.value,
                                             C.c_void_p(d_pts.ptr), C.c_void_p(d_pc.ptr)))
            return n.value

        def point_zbuf():
            n = extract(None)
            L.check(lib.pb3d_depth_buffer_dev(L.ctx(), C.c_void_p(d_pts.ptr), 0, n, L.p_dbl(R), L.p_dbl(cpos), float(cam["f"]), float(cam["cx"]),
                                              float(cam["cy"]), prec, H, W, C.c_void_p(z1.ptr)))

        def point_bits():
            for col in list(colours) + [None]:
                n = extract(col)
                L.check(lib.pb3d_visible_mask_dev(L.ctx(), C.c_void_p(d_pts.ptr), 0, n, L.p_dbl(R), L.p_dbl(cpos), float(cam["f"]),
                                                  float(cam["cx"]), float(cam["cy"]), prec, C.c_void_p(z1.ptr), H, W, 1e-3, 1, C.c_void_p(d_vm.ptr)))
        pa_ms = timeit(point_zbuf, reps)
        pb_ms = timeit(point_bits, reps)
        nocc = extract(None)
        r = {"op": "N6", "name": f"notebook-4 evaluation, {name}", "shape": list(shape[:3]), "image": [H, W], "occupied": nocc,
             "colours": len(colours), "a_grid_zbuf_ms": round(a_ms, 4), "b_visible_bits_ms": round(b_ms, 4),
             "d_presence_and_gt_ms": round(d_ms, 4), "e_iou_rows_ms": round(e_ms, 4), "monument_resident_ms": round(mon_ms, 4),
             "point_path_zbuf_ms": round(pa_ms, 4), "point_path_bits_ms": round(pb_ms, 4)}
        print(json.dumps(r), flush=True)
        res.append(r)
        for b in (d_g, d_m, z1, z2, b1, b2, b3, gt, bm, cnt, d_pts, d_pc, d_vm):
            b.free()



def inter_eval(reps, res, cpu_ref=True):
    """I5, the inter-method metrics (reference utils/eval_helpers.py): pb3d_nn_dist_dev at the reference's sizes (20 k x 20 k both
    directions, the 50 k k = 2 self-query of compute_nn_stats), the full Taj grid's points (pb3d_points_extract_dev, float32) against
    the 20 k SfM sample and a 52 032-point cloud (the SfM cloud's size: the sample resampled with 1e-3 jitter) in both directions, and
    voxel_iou's device counts at 96 and 512.  The SfM clouds are mapped into the grid's frame by the inverse of
    tests/golden/inter_ref.json's transform.  Every nn time includes the index build and the one host wait for the box; `cells` is
    the index (cells per axis) built on the reference set.  With cpu_ref, cKDTree(workers=16) build + query of the same float64
    inputs on this host."""
    from pb3d.eval_helpers import nn_distances_resident, points_bounds_resident, voxel_iou_counts_resident
    lib, L = pb3d._lib.load(), pb3d._lib
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "inter_ref.json")))
    scale = float.fromhex(meta["taj_transform"]["scale"])
    offset = np.array([float.fromhex(v) for v in meta["taj_transform"]["offset"]])
    sfm = np.load(os.path.join(ROOT, "tests", "golden", "inter_sfm20k.npz"))["sfm"]
    sfm_vox = np.ascontiguousarray(((sfm - offset) / scale)[:, ::-1])          # extracted points are (a2, a1, a0)
    rng = np.random.default_rng(0)
    sfm52 = sfm_vox[rng.integers(0, len(sfm_vox), 52032)] + rng.normal(0, 1e-3 / scale, (52032, 3))
    taj = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    nvox = int(np.prod(taj.shape[:3]))
    d_g = dev.from_numpy(taj)
    d_tp, d_tc = dev.DeviceBuffer(nvox * 12), dev.DeviceBuffer(nvox * 3)
    n = C.c_int64(0)
    L.check(lib.pb3d_points_extract_dev(L.ctx(), C.c_void_p(d_g.ptr), *taj.shape[:3], 3, None, 0, nvox, C.c_void_p(d_tp.ptr),
                                        C.c_void_p(d_tc.ptr), C.byref(n)))
    ntaj = n.value
    taj_pts = d_tp.download((ntaj, 3), np.float32)
    taj20 = np.ascontiguousarray(taj_pts[rng.choice(ntaj, 20000, replace=False)], np.float64)
    taj50 = np.ascontiguousarray(taj_pts[rng.choice(ntaj, 50000, replace=False)], np.float64)
    clouds = {"taj_full": (d_tp, ntaj, False, taj_pts), "sfm20k": (dev.from_numpy(sfm_vox), 20000, True, sfm_vox),
              "sfm52k": (dev.from_numpy(sfm52), 52032, True, sfm52), "taj20k": (dev.from_numpy(taj20), 20000, True, taj20),
              "taj50k": (dev.from_numpy(taj50), 50000, True, taj50)}
    d_out = dev.DeviceBuffer(ntaj * 8)

    def cells_of(name):
        d, m, f64, host = clouds[name]
        bb = points_bounds_resident(d, m, f64).download((6,), np.float64)
        c = (C.c_int64 * 3)()
        L.check(lib.pb3d_nn_grid_shape(L.p_dbl(bb), m, c))
        return list(c)

    def ckdtree_ms(q, r, k):
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            return None
        q, r = np.asarray(q, np.float64), np.asarray(r, np.float64)
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            cKDTree(r).query(q, k=k, workers=16)
            t = (time.perf_counter() - t0) * 1e3
            best = t if best is None else min(best, t)
        return best

    cases = [("sfm20k", "taj20k", 1), ("taj20k", "sfm20k", 1), ("taj50k", "taj50k", 2), ("taj_full", "sfm20k", 1),
             ("sfm20k", "taj_full", 1), ("taj_full", "sfm52k", 1), ("sfm52k", "taj_full", 1)]
    for qn, rn, k in cases:
        dq, nq, qf, hq = clouds[qn]
        dr, nr, rf, hr = clouds[rn]
        ms = timeit(lambda: nn_distances_resident(dq, nq, dr, nr, k, qf, rf, out=d_out), reps)
        r = {"op": "I5", "name": f"nn_dist k={k}: {qn} -> {rn}", "nq": nq, "nr": nr, "ms": round(ms, 4), "cells": cells_of(rn),
             "Mquery_s": round(nq / ms / 1e3, 1)}
        if cpu_ref:
            t = ckdtree_ms(hq, hr, k)
            if t is not None:
                r["ckdtree_w16_ms"] = round(t, 2)
                r["speedup_vs_ckdtree"] = round(t / ms, 1)
        print(json.dumps(r), flush=True)
        res.append(r)
    d_bb = dev.DeviceBuffer(2 * 48)
    d_cnt = dev.DeviceBuffer(16)
    for resolution, frac in ((96, 0.01), (512, 0.01)):
        both = np.concatenate([taj_pts.astype(np.float64), sfm_vox])
        lo, hi = both.min(0), both.max(0)
        step = (hi - lo).max() / resolution
        iters = max(1, int(round((frac * np.linalg.norm(hi - lo)) / step)))
        d_sf = clouds["sfm20k"][0]

        def run():
            points_bounds_resident(d_tp, ntaj, False, out=d_bb)
            points_bounds_resident(d_sf, 20000, True, out=d_bb)
            voxel_iou_counts_resident(d_tp, ntaj, d_sf, 20000, lo, step, resolution, iters, False, True, out=d_cnt)
        ms = timeit(run, reps)
        r = {"op": "I5", "name": f"voxel_iou counts (bounds, occupancy, {iters} dilation passes, counts): taj_full vs sfm20k",
             "resolution": resolution, "iters": iters, "ms": round(ms, 4), "counts": d_cnt.download((2,), np.int64).tolist()}
        print(json.dumps(r), flush=True)
        res.append(r)
    for b in [d_g, d_tc, d_out, d_bb, d_cnt] + [c[0] for c in clouds.values()]:
        b.free()


def icp(reps, res, cpu_ref=True):
    """ICP, icp_align (csrc/icp.hip on the search of csrc/nn.hip) between every point of the stored Taj grid (float32) and the 20 k SfM
    sample in voxel coordinates (float64), both ways, the source displaced by 5 degrees about the target's centre and 2 % of its
    extent.  ICP/step: the index build (with its one host wait) and one enqueued step, device events.  ICP/align: icp_align_resident
    with max_iterations 1 and 10 (tolerance 0: no early stop; index build, steps and the 17-value downloads; host wall clock, best of
    reps) -- the difference over 9 is what an iteration costs once the target is binned.  With cpu_ref, 10 iterations of a host ICP
    on the same clouds (one cKDTree of the target, query with 16 workers, the same 3 x 3 solve) as context, not as a threshold.
    ICP/step_trimmed: the trimmed step with rho = 0.75 on the same index and inputs, device events, beside the plain step of the same
    run.  ICP/normals: the target's normals from its 20 nearest neighbours (search and csrc/normals.hip; host wall clock, and the normals
    entry alone on ready rows by device events).  ICP/step_plane: the point-to-plane step on those normals, untrimmed and with rho = 0.75,
    device events, beside the plain step.  SELECT/kth: the selection alone (csrc/select.hip) on the step's keys.  ICP/align_trimmed: the
    whole alignments with rho = 0.75."""
    import math
    from pb3d import preprocess_helpers as ph
    lib, L = pb3d._lib.load(), pb3d._lib
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "inter_ref.json")))
    scale = float.fromhex(meta["taj_transform"]["scale"])
    offset = np.array([float.fromhex(v) for v in meta["taj_transform"]["offset"]])
    sfm = np.load(os.path.join(ROOT, "tests", "golden", "inter_sfm20k.npz"))["sfm"]
    sfm_vox = np.ascontiguousarray(((sfm - offset) / scale)[:, ::-1])
    taj = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    nvox = int(np.prod(taj.shape[:3]))
    d_g = dev.from_numpy(taj)
    d_tp, d_tc = dev.DeviceBuffer(nvox * 12), dev.DeviceBuffer(nvox * 3)
    n = C.c_int64(0)
    L.check(lib.pb3d_points_extract_dev(L.ctx(), C.c_void_p(d_g.ptr), *taj.shape[:3], 3, None, 0, nvox, C.c_void_p(d_tp.ptr),
                                        C.c_void_p(d_tc.ptr), C.byref(n)))
    ntaj = n.value
    taj_pts = d_tp.download((ntaj, 3), np.float32)
    clouds = {"taj_full": (d_tp, ntaj, False, taj_pts), "sfm20k": (dev.from_numpy(sfm_vox), 20000, True, sfm_vox)}
    d_out, d_out20, d_out32 = dev.DeviceBuffer(17 * 8), dev.DeviceBuffer(20 * 8), dev.DeviceBuffer(32 * 8)

    def displaced(host):
        lo, hi = host.min(0).astype(np.float64), host.max(0).astype(np.float64)
        c, ext = 0.5 * (lo + hi), float((hi - lo).max())
        a = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
        K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        th = math.radians(5.0)
        M = np.eye(4)
        M[:3, :3] = np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)
        M[:3, 3] = c - M[:3, :3] @ c + np.array([0.02, -0.03, 0.01]) * ext
        return M

    def wall(fn):
        fn()
        t = []
        for _ in range(max(3, reps)):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return round(1e3 * min(t), 3)

    def host_icp(src, tgt, init, iters):
        from scipy.spatial import cKDTree
        src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
        tree = cKDTree(tgt)
        c = 0.5 * (tgt.min(0) + tgt.max(0))
        T = init.copy()
        for _ in range(iters):
            p = src @ T[:3, :3].T + T[:3, 3]
            d, j = tree.query(p, workers=16)
            P, Q = p - c, tgt[j] - c
            sums = np.concatenate([P.sum(0), Q.sum(0), (P.T @ Q).reshape(9), [(d * d).sum()]])
            T = ph.best_fit_transform_from_sums(len(p), sums, c, c) @ T
        return T

    for sn, tn in (("taj_full", "sfm20k"), ("sfm20k", "taj_full")):
        ds, ns, sf, hs = clouds[sn]
        dt, nt, tf, ht = clouds[tn]
        init = displaced(ht)
        index_ms = timeit(lambda: ph.icp_index_resident(dt, nt, tf), reps)
        box = ph.icp_index_resident(dt, nt, tf)
        c = 0.5 * (box[:3] + box[3:])
        step_ms = timeit(lambda: ph.icp_step_resident(ds, ns, dt, nt, init, -1.0, c, c, sf, tf, out=d_out), reps)
        raw = d_out.download((17,), np.float64)
        r = {"op": "ICP/step", "name": f"icp step: {sn} -> {tn}", "ns": ns, "nt": nt, "index_ms": round(index_ms, 4), "step_ms": round(step_ms, 4),
             "Mpoint_s": round(ns / step_ms / 1e3, 1), "rmse": math.sqrt(raw[16] / ns)}
        print(json.dumps(r), flush=True)
        res.append(r)
        # the target's normals (exact 20-neighbour rows, then csrc/normals.hip; two host waits, so host wall clock) and the
        # point-to-plane step on them beside the plain step: same index, same inputs, untrimmed and with rho = 0.75
        normals_ms = wall(lambda: ph.estimate_normals_resident(dt, nt, 20, None, tf).free())
        d_nrm = ph.estimate_normals_resident(dt, nt, 20, None, tf)
        d_idx = pb3d.eval_helpers.knn_resident(dt, nt, dt, nt, 20, tf, tf, dist=False)[1]
        kernel_ms = timeit(lambda: L.check(lib.pb3d_point_normals_resident(L.ctx(), C.c_void_p(dt.ptr), int(tf), nt, C.c_void_p(d_idx.ptr), 20,
                                                                           None, C.c_void_p(d_nrm.ptr))), reps)
        r = {"op": "ICP/normals", "name": f"estimate_normals_resident, k 20: {tn}", "n": nt, "wall_ms": normals_ms,
             "normals_entry_ms": round(kernel_ms, 4), "Mpoint_s": round(nt / normals_ms / 1e3, 2)}
        print(json.dumps(r), flush=True)
        res.append(r)
        plane_ms = timeit(lambda: ph.icp_step_plane_resident(ds, ns, dt, nt, d_nrm, init, -1.0, None, c, sf, tf, out=d_out32), reps)
        raw = d_out32.download((32,), np.float64)
        plane_trim_ms = timeit(lambda: ph.icp_step_plane_resident(ds, ns, dt, nt, d_nrm, init, -1.0, 0.75, c, sf, tf, out=d_out32), reps)
        r = {"op": "ICP/step_plane", "name": f"icp point-to-plane step: {sn} -> {tn}", "ns": ns, "nt": nt, "step_ms": round(step_ms, 4),
             "step_plane_ms": round(plane_ms, 4), "plane_over_plain": round(plane_ms / step_ms, 3), "step_plane_trimmed_ms": round(plane_trim_ms, 4),
             "Mpoint_s": round(ns / plane_ms / 1e3, 1), "rmse_plane": math.sqrt(raw[28] / ns), "rmse_point": math.sqrt(raw[29] / ns)}
        print(json.dumps(r), flush=True)
        res.append(r)
        d_nrm.free()
        d_idx.free()
        # the trimmed step beside it (same index, same inputs, rho = 0.75), and the selection alone on the step's keys: the squared
        # nearest distances of the moved source (nn_distances squared: the step's d2 up to the rounding of the square root)
        trim_ms = timeit(lambda: ph.icp_step_trimmed_resident(ds, ns, dt, nt, init, -1.0, 0.75, c, c, sf, tf, out=d_out20), reps)
        raw = d_out20.download((20,), np.float64)
        count, m = (int(v) for v in raw[[0, 18]].view(np.int64))
        r = {"op": "ICP/step_trimmed", "name": f"icp trimmed step, rho 0.75: {sn} -> {tn}", "ns": ns, "nt": nt, "step_ms": round(step_ms, 4),
             "step_trimmed_ms": round(trim_ms, 4), "trimmed_over_plain": round(trim_ms / step_ms, 3), "count": count, "candidates": m,
             "tau": float(raw[19])}
        print(json.dumps(r), flush=True)
        res.append(r)
        d_moved = ph.transform_points_resident(ds, ns, init, sf)
        d_keys = pb3d.eval_helpers.nn_distances_resident(d_moved, ns, dt, nt, 1, True, tf)
        keys = d_keys.download((ns,), np.float64)
        d_keys.upload(keys * keys)
        d_tau = dev.DeviceBuffer(8)
        kth_ms = timeit(lambda: pb3d.kth_smallest_resident(d_keys, ns, (3 * ns) // 4, out=d_tau), reps)
        passes, hist_bytes = 8, 8 * 256 * 4
        r = {"op": "SELECT/kth", "name": f"k-th smallest of the step's keys: {sn} -> {tn}", "n": ns, "rank": (3 * ns) // 4, "ms": round(kth_ms, 4),
             "passes": passes, "launches": 2 * passes + 1, "bytes_read": passes * 8 * ns + passes * hist_bytes,
             "GB_s": round((passes * 8 * ns + passes * hist_bytes) / kth_ms / 1e6, 2), "value": float(d_tau.download((1,), np.float64)[0])}
        print(json.dumps(r), flush=True)
        res.append(r)
        for b in (d_moved, d_keys, d_tau):
            b.free()
        t1 = wall(lambda: ph.icp_align_resident(ds, ns, dt, nt, 1, 0.0, None, init, False, sf, tf))
        t10 = wall(lambda: ph.icp_align_resident(ds, ns, dt, nt, 10, 0.0, None, init, False, sf, tf))
        _, hist, _ = ph.icp_align_resident(ds, ns, dt, nt, 10, 0.0, None, init, True, sf, tf)
        r = {"op": "ICP/align", "name": f"icp_align_resident: {sn} -> {tn}", "ns": ns, "nt": nt, "max_iterations_1_ms": t1,
             "max_iterations_10_ms": t10, "per_further_iteration_ms": round((t10 - t1) / 9, 3), "rmse_first_last": [hist[0][1], hist[-1][1]]}
        if cpu_ref:
            try:
                r["ckdtree_w16_icp_10_iterations_ms"] = wall(lambda: host_icp(hs, ht, init, 10))
            except ImportError:
                pass
        print(json.dumps(r), flush=True)
        res.append(r)
        t1 = wall(lambda: ph.icp_align_resident(ds, ns, dt, nt, 1, 0.0, None, init, False, sf, tf, 0.75))
        t10 = wall(lambda: ph.icp_align_resident(ds, ns, dt, nt, 10, 0.0, None, init, False, sf, tf, 0.75))
        _, hist, _ = ph.icp_align_resident(ds, ns, dt, nt, 10, 0.0, None, init, True, sf, tf, 0.75)
        r = {"op": "ICP/align_trimmed", "name": f"icp_align_resident, rho 0.75: {sn} -> {tn}", "ns": ns, "nt": nt, "max_iterations_1_ms": t1,
             "max_iterations_10_ms": t10, "per_further_iteration_ms": round((t10 - t1) / 9, 3), "rmse_first_last": [hist[0][1], hist[-1][1]],
             "count_last": hist[-1][0]}
        print(json.dumps(r), flush=True)
        res.append(r)
    for b in [d_g, d_tc, d_out, d_out20, d_out32] + [c[0] for c in clouds.values()]:
        b.free()


FP64_VECTOR_PEAK = 78.6e12     # the spec sheet's vector FP64 rate of the MI355X, FLOP/s with a fused multiply-add counted as two


def plane(reps, res, cpu_ref=True):
    """PLANE, fit_plane_ransac's device entries (csrc/plane.hip) on every point of the stored Taj grid (float32) and on the 20 k SfM
    sample in voxel coordinates (float64), K = 1024 hypotheses, tau = 1 % of the extent, device events.  PLANE/score: hypotheses +
    score enqueued together, the score alone, and one refit (moments) about the box centre with the best hypothesis.  The score's
    float64 operations are 6 n K (three products and three sums per point and plane; fabs and the compare are not counted); their
    rate is set against the spec sheet's vector FP64 rate, which counts a fused multiply-add as two -- the stated arithmetic rounds
    every product and sum on its own, so half of that rate is this kernel's ceiling.  PLANE/crop: the Taj points cropped to the SfM
    sample's box.  With cpu_ref, the wall time of the same scoring in NumPy on this host (the restatement's loop: all 1024 planes of
    the 20 k cloud; 16 planes of the Taj cloud, named as such) as context, not as a threshold."""
    from pb3d import preprocess_helpers as ph
    lib, L = pb3d._lib.load(), pb3d._lib
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "inter_ref.json")))
    scale = float.fromhex(meta["taj_transform"]["scale"])
    offset = np.array([float.fromhex(v) for v in meta["taj_transform"]["offset"]])
    sfm = np.load(os.path.join(ROOT, "tests", "golden", "inter_sfm20k.npz"))["sfm"]
    sfm_vox = np.ascontiguousarray(((sfm - offset) / scale)[:, ::-1])
    taj = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    nvox = int(np.prod(taj.shape[:3]))
    d_g = dev.from_numpy(taj)
    d_tp, d_tc = dev.DeviceBuffer(nvox * 12), dev.DeviceBuffer(nvox * 3)
    cnt = C.c_int64(0)
    L.check(lib.pb3d_points_extract_dev(L.ctx(), C.c_void_p(d_g.ptr), *taj.shape[:3], 3, None, 0, nvox, C.c_void_p(d_tp.ptr),
                                        C.c_void_p(d_tc.ptr), C.byref(cnt)))
    ntaj = cnt.value
    taj_pts = d_tp.download((ntaj, 3), np.float32)
    clouds = {"taj_full": (d_tp, ntaj, False, taj_pts), "sfm20k": (dev.from_numpy(sfm_vox), 20000, True, sfm_vox)}
    K = 1024

    def numpy_score(host, planes, tau):
        p = np.ascontiguousarray(host, dtype=np.float64)
        x, y, z = (np.ascontiguousarray(p[:, a])[None, :] for a in range(3))
        step = max(1, (1 << 22) // len(p))
        counts = np.zeros(len(planes), np.int64)
        with np.errstate(invalid="ignore"):
            for k in range(0, len(planes), step):
                q = planes[k:k + step]
                r = q[:, 0:1] * x
                r += q[:, 1:2] * y
                r += q[:, 2:3] * z
                r += q[:, 3:4]
                np.abs(r, out=r)
                counts[k:k + step] = (r <= tau).sum(1)
        return counts

    for name, (d_p, n, f64, host) in clouds.items():
        lo, hi = host.min(0).astype(np.float64), host.max(0).astype(np.float64)
        tau, pivot = 0.01 * float((hi - lo).max()), 0.5 * (lo + hi)
        trip = np.random.default_rng(0).integers(0, n, size=(K, 3), dtype=np.int64)
        d_trip = dev.from_numpy(trip)
        d_planes, d_counts, d_mom = dev.DeviceBuffer(K * 32), dev.DeviceBuffer(K * 8), dev.DeviceBuffer(12 * 8)

        def both():
            ph.plane_hypotheses_resident(d_p, n, d_trip, K, f64, out=d_planes)
            ph.plane_score_resident(d_p, n, d_planes, K, tau, f64, out=d_counts)

        both_ms = timeit(both, reps)
        score_ms = timeit(lambda: ph.plane_score_resident(d_p, n, d_planes, K, tau, f64, out=d_counts), reps)
        counts = d_counts.download((K,), np.int64)
        planes = d_planes.download((K, 4), np.float64)
        best = int(np.argmax(counts))
        refit_ms = timeit(lambda: ph.plane_moments_resident(d_p, n, planes[best], tau, pivot, f64, out=d_mom), reps)
        raw = d_mom.download((12,), np.float64)
        flops = 6.0 * n * K
        r = {"op": "PLANE/score", "name": f"plane hypotheses + score + one refit: {name}", "n": n, "K": K, "dtype": "float64" if f64 else "float32",
             "hypotheses_and_score_ms": round(both_ms, 4), "score_ms": round(score_ms, 4), "refit_moments_ms": round(refit_ms, 4),
             "score_fp64_TFLOP_s": round(flops / score_ms / 1e9, 3), "score_frac_of_fp64_vector_peak": round(flops / (score_ms * 1e-3) / FP64_VECTOR_PEAK, 4),
             "score_point_GB_s": round(n * (24 if f64 else 12) / score_ms / 1e6, 2), "best_inlier_share": round(int(counts[best]) / n, 4),
             "refit_count": int(raw[:1].view(np.int64)[0])}
        if cpu_ref:
            kk = K if n <= 100000 else 16
            t0 = time.perf_counter()
            ref = numpy_score(host, planes[:kk], tau)
            r[f"numpy_score_{kk}_planes_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            r["numpy_counts_equal"] = bool(np.array_equal(ref, counts[:kk]))
        print(json.dumps(r), flush=True)
        res.append(r)
        for b in (d_trip, d_planes, d_counts, d_mom):
            b.free()
    # the dense cloud cropped to the sparse cloud's box
    lo, hi = sfm_vox.min(0), sfm_vox.max(0)
    d_out, d_idx, d_count = dev.DeviceBuffer(ntaj * 12), dev.DeviceBuffer(ntaj * 4), dev.DeviceBuffer(8)
    fn = lambda: L.check(lib.pb3d_points_crop_box_resident(L.ctx(), C.c_void_p(d_tp.ptr), 0, ntaj, L.p_dbl(lo), L.p_dbl(hi), C.c_void_p(d_out.ptr),
                                                           C.c_void_p(d_idx.ptr), C.c_void_p(d_count.ptr)))
    crop_ms = timeit(fn, reps)
    kept = int(d_count.download((1,), np.int64)[0])
    moved = ntaj * 12 * 2 + kept * 16             # two reads of the points (count, fill), the surviving rows and their positions written
    r = {"op": "PLANE/crop", "name": "crop_to_box: taj_full to the sfm20k box", "n": ntaj, "kept": kept, "ms": round(crop_ms, 4),
         "alg_GB_s": round(moved / crop_ms / 1e6, 1), "frac_of_8TBs": round(moved / crop_ms / 1e6 / PEAK, 4)}
    if cpu_ref:
        t0 = time.perf_counter()
        m = ((lo <= taj_pts) & (taj_pts <= hi)).all(1)
        got = taj_pts[m]
        r["numpy_mask_and_take_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        r["numpy_count_equal"] = bool(len(got) == kept)
    print(json.dumps(r), flush=True)
    res.append(r)
    for b in [d_g, d_tc, d_out, d_idx, d_count] + [c[0] for c in clouds.values()]:
        b.free()


def cluster(reps, res, cpu_ref=True):
    """CLUSTER, cluster_points (csrc/cluster.hip): the 20 k SfM sample at (eps 0.06, min_samples 10) in the frame the fixture is stored
    in (float64), and every point of the stored Taj grid (float32) at eps = 1.5 and 2.5 voxels with min_samples 10.  Per case and per
    cell-edge choice of the index (knob cluster_cell: 1 = two points per cell, 2 = cells wider than eps): the whole resident call and
    the counts alone by device events (best mean of reps), and the call's passes from its own events under knob cluster_timing (index,
    count, union + flatten, ranks with the host wait, labels).  keep_largest_clusters_resident (k = 1) under the built-in rule.  With
    cpu_ref, scikit-learn's DBSCAN(algorithm="kd_tree") on the SfM sample on this host, where it is installed (the 12 M Taj points
    are beyond what it clusters in a benchmark's time)."""
    from pb3d import cluster as cl
    lib, L = pb3d._lib.load(), pb3d._lib
    sfm = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "inter_sfm20k.npz"))["sfm"])
    taj = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    nvox = int(np.prod(taj.shape[:3]))
    d_g = dev.from_numpy(taj)
    d_tp, d_tc = dev.DeviceBuffer(nvox * 12), dev.DeviceBuffer(nvox * 3)
    cnt = C.c_int64(0)
    L.check(lib.pb3d_points_extract_dev(L.ctx(), C.c_void_p(d_g.ptr), *taj.shape[:3], 3, None, 0, nvox, C.c_void_p(d_tp.ptr),
                                        C.c_void_p(d_tc.ptr), C.byref(cnt)))
    ntaj = cnt.value
    d_g.free(); d_tc.free()
    d_sfm = dev.from_numpy(sfm)
    cases = [("sfm20k", d_sfm, 20000, True, 0.06, 10), ("taj_full", d_tp, ntaj, False, 1.5, 10), ("taj_full", d_tp, ntaj, False, 2.5, 10)]

    def call(d_p, n, f64, eps, ms):
        bufs = cl.cluster_points_resident(d_p, n, eps, ms, f64)
        for b in bufs[:4]:
            b.free()
        return bufs[4]

    for name, d_p, n, f64, eps, ms in cases:
        r = {"op": "CLUSTER", "name": f"cluster_points: {name}", "n": n, "dtype": "float64" if f64 else "float32", "eps": eps, "min_samples": ms}
        d_cnt = dev.DeviceBuffer(n * 4)
        try:
            for knob, tag in ((1, "cells_2_per_cell"), (2, "cells_above_eps")):
                L.set_tuning("cluster_cell", knob)
                L.set_tuning("cluster_timing", 1)
                call(d_p, n, f64, eps, ms)
                best = None
                for _ in range(max(2, reps)):
                    call(d_p, n, f64, eps, ms)
                    cells, pm = (C.c_int64 * 3)(), (C.c_double * 5)()
                    L.check(lib.pb3d_cluster_last(L.ctx(), cells, pm))
                    if best is None or sum(pm) < sum(best):
                        best = list(pm)
                L.set_tuning("cluster_timing", 0)
                whole = min(timeit(lambda: call(d_p, n, f64, eps, ms), reps, warm=1) for _ in range(2))
                counts = min(timeit(lambda: cl.radius_neighbor_counts_resident(d_p, n, eps, f64, out=d_cnt), reps, warm=1) for _ in range(2))
                r[tag] = {"cells": list(cells), "call_ms": round(whole, 4), "radius_count_call_ms": round(counts, 4),
                          "pass_ms": dict(zip(("index", "count", "union_flatten", "ranks_and_wait", "labels"), (round(v, 4) for v in best)))}
        finally:
            L.set_tuning("cluster_cell", 0)
            L.set_tuning("cluster_timing", 0)
        d_lab, d_core, d_c, d_sz, nc = cl.cluster_points_resident(d_p, n, eps, ms, f64)
        labels = d_lab.download((n,), np.int32)
        sizes = d_sz.download((nc,), np.int64) if nc else np.zeros(0, np.int64)
        r.update({"clusters": nc, "largest": sorted(sizes.tolist(), reverse=True)[:5], "noise": int((labels < 0).sum()),
                  "core": int(np.count_nonzero(d_core.download((n,), np.uint8)))})
        for b in (d_lab, d_core, d_c, d_sz, d_cnt):
            b.free()

        def keep():
            d_o, d_i, _, _ = cl.keep_largest_clusters_resident(d_p, n, eps, ms, 1, f64)
            d_o.free(); d_i.free()

        r["keep_largest_k1_call_ms"] = round(timeit(keep, reps, warm=1), 4)
        if cpu_ref and n <= 100000:
            try:
                from sklearn.cluster import DBSCAN
            except ImportError:
                DBSCAN = None
            if DBSCAN is not None:
                host = sfm
                t = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    ref = DBSCAN(eps=eps, min_samples=ms, algorithm="kd_tree").fit(host)
                    t.append(time.perf_counter() - t0)
                r["sklearn_kd_tree_ms"] = round(1e3 * min(t), 1)
                r["sklearn_labels_equal"] = bool(np.array_equal(ref.labels_, labels))
        print(json.dumps(r), flush=True)
        res.append(r)
    d_sfm.free(); d_tp.free()


def downsample(reps, res, cpu_ref=True):
    """DOWNSAMPLE, voxel_downsample (csrc/downsample.hip): the 20 k SfM sample (float64) at voxel_size 0.05 and 0.5, and every point of
    the stored Taj grid (float32, voxel units) at 2, 4 and 8 voxels, both reductions.  The whole resident call by device events (best
    mean of reps; its two host waits are inside).  reduce="first" runs the hash, the numbering and a gather; "centroid" adds the
    stable sort of the (voxel, position) pairs and the ordered sums, so their difference is what the order costs.  With cpu_ref, the
    NumPy restatement of tests/downsample_restate.py on this host's CPU, and whether the device's arrays equal it."""
    import downsample_restate as dr
    from pb3d import downsample as ds
    lib, L = pb3d._lib.load(), pb3d._lib
    sfm = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "inter_sfm20k.npz"))["sfm"])
    taj = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    nvox = int(np.prod(taj.shape[:3]))
    d_g = dev.from_numpy(taj)
    d_tp, d_tc = dev.DeviceBuffer(nvox * 12), dev.DeviceBuffer(nvox * 3)
    cnt = C.c_int64(0)
    L.check(lib.pb3d_points_extract_dev(L.ctx(), C.c_void_p(d_g.ptr), *taj.shape[:3], 3, None, 0, nvox, C.c_void_p(d_tp.ptr),
                                        C.c_void_p(d_tc.ptr), C.byref(cnt)))
    ntaj = cnt.value
    d_g.free(); d_tc.free()
    taj_pts = d_tp.download((ntaj, 3), np.float32).copy() if cpu_ref else None
    d_sfm = dev.from_numpy(sfm)
    cases = [("sfm20k", d_sfm, sfm, 20000, True, 0.05), ("sfm20k", d_sfm, sfm, 20000, True, 0.5)]
    cases += [("taj_full", d_tp, taj_pts, ntaj, False, float(v)) for v in (2, 4, 8)]
    for name, d_p, host, n, f64, vs in cases:
        r = {"op": "DOWNSAMPLE", "name": f"voxel_downsample: {name}", "n": n, "dtype": "float64" if f64 else "float32", "voxel_size": vs}
        bufs = [dev.DeviceBuffer(n * w) for w in (24 if f64 else 12, 4, 4, 4)]
        m = C.c_int64(0)
        for reduce in ("centroid", "first"):
            def call():
                L.check(lib.pb3d_voxel_downsample_resident(L.ctx(), C.c_void_p(d_p.ptr), int(f64), n, vs, None, ds.REDUCE[reduce],
                                                           *(C.c_void_p(b.ptr) for b in bufs), C.byref(m)))
            r[f"{reduce}_call_ms"] = round(min(timeit(call, reps, warm=1) for _ in range(2)), 4)
            if reduce == "centroid":
                counts = bufs[3].download((m.value,), np.uint32)
                r.update({"voxels": int(m.value), "largest_voxel": int(counts.max()), "mean_points_per_voxel": round(n / m.value, 2)})
            if cpu_ref:
                t = []
                for _ in range(2):
                    t0 = time.perf_counter()
                    ref = dr.restate(host, vs, None, reduce)
                    t.append(time.perf_counter() - t0)
                r[f"numpy_{reduce}_ms"] = round(1e3 * min(t), 1)
                got = (bufs[0].download((m.value, 3), host.dtype), bufs[1].download((m.value,), np.int32),
                       bufs[2].download((n,), np.int32), bufs[3].download((m.value,), np.uint32))
                r[f"numpy_{reduce}_equal"] = bool(all(np.array_equal(g, w) for g, w in zip(got, ref)))
        for b in bufs:
            b.free()
        print(json.dumps(r), flush=True)
        res.append(r)
    d_sfm.free(); d_tp.free()


def smooth(reps, res, cpu_ref=True):
    """SMOOTH, mesh_vertex_adjacency and smooth_mesh (csrc/smooth.hip) on the stride-1 mesh of the stored Taj grid (float32 vertices, int32
    faces).  Resident, by device events (best mean of reps, host waits inside): the adjacency build alone, then 10 Taubin rounds and 1
    Taubin round, each with its own adjacency build -- their difference over 18 is one step.  Beside a step, the time a plain
    device-to-device copy of its bytes takes (positions read once per neighbour and once per vertex, the lists once, positions written
    once), measured here with pb3d_d2d.  Then both through the NumPy API (upload, call, download; host wall clock, best of reps) and,
    with cpu_ref, the restatement of tests/smooth_restate.py in NumPy on this host and whether the device's arrays equal it."""
    import smooth_restate as sr
    lib, L = pb3d._lib.load(), pb3d._lib
    taj = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    v, f = pb3d.meshify_colored_voxel_grid(taj, stride=1)[:2]
    nv, nf = len(v), len(f)
    d_v, d_f = dev.from_numpy(v), dev.from_numpy(f)
    bufs = [dev.DeviceBuffer((nv + 1) * 8), dev.DeviceBuffer(6 * nf * 4), dev.DeviceBuffer(6 * nf * 4), dev.DeviceBuffer(nv), dev.DeviceBuffer(nv * 12)]
    d_st, d_nb, d_mu, d_bd, d_out = (C.c_void_p(b.ptr) for b in bufs)
    total = C.c_int64(0)

    def adjacency():
        L.check(lib.pb3d_mesh_adjacency_resident(L.ctx(), C.c_void_p(d_f.ptr), 0, nv, nf, d_st, d_nb, d_mu, d_bd, C.byref(total)))

    def taubin(iterations):
        return lambda: L.check(lib.pb3d_mesh_smooth_resident(L.ctx(), C.c_void_p(d_v.ptr), 0, nv, C.c_void_p(d_f.ptr), 0, nf, iterations, 0.5, -0.53,
                                                             None, 0, d_out))

    def best(fn):
        return min(timeit(fn, reps, warm=1) for _ in range(2))

    t_adj, t10, t1 = best(adjacency), best(taubin(10)), best(taubin(1))
    starts = bufs[0].download((nv + 1,), np.int64)
    step_bytes = int(total.value) * (24 + 4) + nv * (24 + 24) + (nv + 1) * 8
    d_a, d_b = dev.DeviceBuffer(step_bytes // 2), dev.DeviceBuffer(step_bytes // 2)       # a copy reads and writes: half the bytes each way
    t_copy = best(lambda: L.check(lib.pb3d_d2d(L.ctx(), C.c_void_p(d_b.ptr), C.c_void_p(d_a.ptr), step_bytes // 2)))
    d_a.free(); d_b.free()
    step = (t10 - t1) / 18.0
    r = {"op": "SMOOTH", "name": "mesh smoothing: stored Taj, stride 1", "nverts": nv, "nfaces": nf, "pairs": 6 * nf, "unique_pairs": int(total.value),
         "max_degree": int(np.diff(starts).max()), "adjacency_ms": round(t_adj, 4), "taubin10_ms": round(t10, 4), "taubin1_ms": round(t1, 4),
         "step_ms": round(step, 4), "step_bytes": step_bytes, "step_GB_s": round(step_bytes / step / 1e6, 1), "copy_of_step_bytes_ms": round(t_copy, 4),
         "step_over_copy": round(step / t_copy, 2), "adjacency_share_of_taubin10": round(t_adj / t10, 3)}
    wall = {"adjacency": [], "taubin10": []}
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        got_adj = pb3d.mesh_vertex_adjacency(f, nv, return_multiplicity=True, return_boundary=True)
        wall["adjacency"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        got = pb3d.smooth_mesh(v, f)
        wall["taubin10"].append(time.perf_counter() - t0)
    r["numpy_api_adjacency_ms"] = round(1e3 * min(wall["adjacency"][1:]), 2)
    r["numpy_api_taubin10_ms"] = round(1e3 * min(wall["taubin10"][1:]), 2)
    if cpu_ref:
        t0 = time.perf_counter()
        ref_adj = sr.adjacency(f, nv)
        r["numpy_restatement_adjacency_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        t0 = time.perf_counter()
        ref = sr.restate(v, f)
        r["numpy_restatement_taubin10_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        r["adjacency_equal"] = bool(all(np.array_equal(g, w) for g, w in zip(got_adj, ref_adj)))
        r["taubin10_equal"] = bool(got.tobytes() == ref.tobytes())
    for b in bufs + [d_v, d_f]:
        b.free()
    print(json.dumps(r), flush=True)
    res.append(r)


def simplify(reps, res, cpu_ref=True):
    """SIMPLIFY, simplify_mesh and compact_mesh (csrc/simplify.hip) on the stride-1 mesh of the stored Taj grid as
    pb3d.device.meshify(download=False) leaves it (float32 vertices, int32 faces, nearest-voxel bytes).  Resident, by device events (best
    mean of reps, host waits inside): simplify_mesh at voxel_size 2 and 4 and compact_mesh, each with duplicate_faces drop and keep.
    Per row the five passes from the call's own events under knob simplify_timing (clusters, map, sorts + repeats, scans, gathers) and
    pb3d_simplify_last's counts.  The yardsticks are the same library's own operations on the same data: (a) voxel_downsample of the same
    vertex list at the same voxel_size (the call contains it), (b) the adjacency build of smooth_mesh on the same faces (two sorts of
    6 nf pairs), (c) a plain device-to-device copy of the bytes the face half must move (faces, cluster numbers and rows in; faces,
    positions, rows, index, inverse and colours out).  With cpu_ref, the restatement of tests/simplify_restate.py in NumPy on this host
    and whether the device's six arrays equal it."""
    import simplify_restate as sr
    from pb3d import simplify as sm
    lib, L = pb3d._lib.load(), pb3d._lib
    taj = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    d_g = dev.from_numpy(taj)
    (d_v, d_f, d_n, d_c), (nv, nf) = dev.meshify(d_g, taj.shape, download=False)
    d_g.free(); d_n.free()
    host = (d_v.download((nv, 3), np.float32), d_f.download((nf, 3), np.int32), d_c.download((nv, 3))) if cpu_ref else None
    outs = [dev.DeviceBuffer(n) for n in (nv * 12, nf * 12, nv * 3, nv * 4, nv * 4, nf * 4)]
    po = [C.c_void_p(b.ptr) for b in outs]
    counts, last, ms = (C.c_int64 * 2)(), (C.c_int64 * 3)(), (C.c_double * 5)()
    head = (C.c_void_p(d_v.ptr), 0, nv, C.c_void_p(d_f.ptr), 0, nf)

    def best(fn):
        return min(timeit(fn, reps, warm=1) for _ in range(2))

    # (b): the adjacency build on the same faces
    adj = [dev.DeviceBuffer((nv + 1) * 8), dev.DeviceBuffer(6 * nf * 4)]
    total = C.c_int64(0)
    t_adj = best(lambda: L.check(lib.pb3d_mesh_adjacency_resident(L.ctx(), C.c_void_p(d_f.ptr), 0, nv, nf, C.c_void_p(adj[0].ptr),
                                                                  C.c_void_p(adj[1].ptr), None, None, C.byref(total))))
    for b in adj:
        b.free()
    ds_bufs = [dev.DeviceBuffer(nv * w) for w in (12, 4, 4)]
    t_down = {}
    for vs, dup in [(2.0, "drop"), (2.0, "keep"), (4.0, "drop"), (4.0, "keep"), (None, "drop"), (None, "keep")]:
        d = sm.DUPLICATE_FACES[dup]
        if vs is None:
            call = lambda: L.check(lib.pb3d_mesh_compact_resident(L.ctx(), *head, d, C.c_void_p(d_c.ptr), 3, *po, counts))
        else:
            call = lambda: L.check(lib.pb3d_mesh_simplify_resident(L.ctx(), *head, vs, None, 0, d, C.c_void_p(d_c.ptr), 3, *po, counts))
            if vs not in t_down:        # (a): voxel_downsample of the same list
                m = C.c_int64(0)
                t_down[vs] = best(lambda: L.check(lib.pb3d_voxel_downsample_resident(L.ctx(), C.c_void_p(d_v.ptr), 0, nv, vs, None, 0,
                                                                                     *(C.c_void_p(b.ptr) for b in ds_bufs), None, C.byref(m))))
        r = {"op": "SIMPLIFY", "name": ("compact_mesh" if vs is None else "simplify_mesh") + ": stored Taj, stride 1", "nverts": nv, "nfaces": nf,
             "voxel_size": vs, "duplicate_faces": dup, "call_ms": round(best(call), 4)}
        L.set_tuning("simplify_timing", 1)
        try:
            passes = []
            for _ in range(max(2, reps)):
                call()
                L.check(lib.pb3d_simplify_last(L.ctx(), last, ms))
                passes.append(list(ms))
        finally:
            L.set_tuning("simplify_timing", 0)
        p = min(passes, key=sum)
        n_out, m_out, clusters = int(last[1]), int(last[2]), int(last[0])
        face_half = sum(p[1:])
        moved = (12 * nf + 4 * nv + 12 * clusters + 3 * nv) + (16 * m_out + 16 * n_out + 4 * nv + 3 * n_out)
        d_a, d_b = dev.DeviceBuffer(moved // 2), dev.DeviceBuffer(moved // 2)           # a copy reads and writes: half the bytes each way
        t_copy = best(lambda: L.check(lib.pb3d_d2d(L.ctx(), C.c_void_p(d_b.ptr), C.c_void_p(d_a.ptr), moved // 2)))
        d_a.free(); d_b.free()
        r.update({"clusters": clusters, "nverts_out": n_out, "nfaces_out": m_out,
                  "pass_ms": {k: round(t, 4) for k, t in zip(("clusters", "map", "sorts_repeats", "scans", "gathers"), p)},
                  "face_half_ms": round(face_half, 4), "adjacency_ms": round(t_adj, 4), "face_half_over_adjacency": round(face_half / t_adj, 2),
                  "face_half_bytes": moved, "copy_of_face_half_bytes_ms": round(t_copy, 4), "face_half_over_copy": round(face_half / t_copy, 2)})
        if vs is not None:
            r.update({"voxel_downsample_ms": round(t_down[vs], 4), "call_over_voxel_downsample": round(r["call_ms"] / t_down[vs], 2)})
        if cpu_ref:
            call()
            got = (outs[0].download((n_out, 3), np.float32), outs[1].download((m_out, 3), np.int32), outs[2].download((n_out, 3)),
                   outs[3].download((n_out,), np.int32), outs[4].download((nv,), np.int32), outs[5].download((m_out,), np.int32))
            t0 = time.perf_counter()
            ref = sr.restate(host[0], host[1], vs, None, "centroid", dup, host[2])
            r["numpy_restatement_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            r["numpy_equal"] = bool((int(counts[0]), int(counts[1])) == (len(ref[0]), len(ref[1]))
                                    and all(np.array_equal(g, w) for g, w in zip(got, ref)) and got[0].tobytes() == ref[0].tobytes())
        print(json.dumps(r), flush=True)
        res.append(r)
    for b in outs + ds_bufs + [d_v, d_f, d_c]:
        b.free()


def voxelize(reps, res, cpu_ref=True):
    """VOXELIZE, voxelize_mesh (csrc/voxelize.hip): the stride-1 mesh of the stored Taj grid (float32 vertices, int32 faces, meshify's frame)
    back into its 512 x 278 x 512 grid.  Resident, by device events (best mean of reps, the check's host wait inside): the whole call;
    under knob voxelize_timing the call's own events give the crossing pass (the bit volume's clear included) and the scan pass.  Beside
    the scan pass the time of a plain fill of the same output bytes (pb3d_dev_memset), the only roof it has; for the crossing pass the
    crossings per second.  Then whether the bytes equal the grid's occupancy and, with cpu_ref, the restatement of
    tests/voxelize_restate.py in NumPy on this host and whether the device's bytes equal it."""
    import voxelize_restate as vr
    lib, L = pb3d._lib.load(), pb3d._lib
    taj = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    shape = taj.shape[:3]
    nvox = int(np.prod(shape))
    occ = np.any(taj > 0, axis=-1)
    v, f = pb3d.meshify_colored_voxel_grid(taj, stride=1)[:2]
    nv, nf = len(v), len(f)
    d_v, d_f, d_out = dev.from_numpy(v), dev.from_numpy(f), dev.DeviceBuffer(nvox)

    def call(**kw):
        return pb3d.voxelize_mesh_resident(d_v, nv, d_f, nf, shape, frame="meshify", out=d_out, **kw)

    def best(fn):
        return min(timeit(fn, reps, warm=1) for _ in range(2))

    t_all = best(call)
    t_fill = best(lambda: L.check(lib.pb3d_dev_memset(L.ctx(), C.c_void_p(d_out.ptr), 0, nvox)))
    L.set_tuning("voxelize_timing", 1)
    passes = []
    try:
        for _ in range(reps + 1):
            call()
            pm = (C.c_double * 2)()
            L.check(lib.pb3d_voxelize_last(L.ctx(), pm))
            passes.append((pm[0], pm[1]))
    finally:
        L.set_tuning("voxelize_timing", 0)
    t_cross, t_scan = min(p[0] for p in passes[1:]), min(p[1] for p in passes[1:])
    _, stats = call(return_stats=True)
    got = d_out.download(shape)
    r = {"op": "VOXELIZE", "name": "voxelize_mesh: stored Taj, stride-1 mesh back into its grid", "shape": list(shape), "nverts": nv, "nfaces": nf,
         "ms": round(t_all, 4), "crossing_pass_ms": round(t_cross, 4), "scan_pass_ms": round(t_scan, 4), "fill_of_output_bytes_ms": round(t_fill, 4),
         "scan_over_fill": round(t_scan / t_fill, 2), "output_GB_s_of_scan": round(nvox / t_scan / 1e6, 1),
         "Mcrossings_s": round(stats["crossings"] / t_cross / 1e3, 1), **stats,
         "equals_occupancy": bool(np.array_equal(got, occ.view(np.uint8))), "voxels_differing_from_occupancy": int(np.count_nonzero(got != occ))}
    if cpu_ref:
        t0 = time.perf_counter()
        ref, ref_stats = vr.restate(v, f, shape, frame="meshify")
        r["numpy_restatement_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        r["equals_restatement"] = bool(np.array_equal(got, ref) and stats == ref_stats)
    for b in (d_v, d_f, d_out):
        b.free()
    print(json.dumps(r), flush=True)
    res.append(r)


def edt(reps, res, cpu_ref=True):
    """EDT, distance_transform (csrc/edt.hip) on the stored Taj grid (512 x 278 x 512 RGB), resident, by device events (best mean of reps):
    to="background" without and with indices, to="surface", close_grid at radius 2, and grid_surface_metrics of the grid against
    voxelize_mesh of its own smoothed mesh (wall clock: it has four host waits).  Then to="background" on two adversarial contents of
    the same shape and channel count: a full grid with one empty corner voxel (one target: the longest distances, every column's
    envelope a single parabola found late) and a 3-D checkerboard (every other voxel a parabola vertex), with their ratio to the Taj
    content.  Yardsticks: the time a plain device copy (pb3d_d2d) needs for the bytes the three passes must move -- the grid's bytes and
    4 (sq) or 8 (sq and index) bytes per voxel written by every pass and read by the next -- from the rate of a copy of 4 bytes per
    voxel; and, with cpu_ref, scipy.ndimage.distance_transform_edt of the same occupancy on this host's CPU (and whether the device's
    distances equal it bit for bit)."""
    import scipy.ndimage as ndi
    import pb3d.distance as pd
    lib, L = pb3d._lib.load(), pb3d._lib
    taj = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"])
    shape, ch = taj.shape[:3], taj.shape[3]
    nvox = int(np.prod(shape))
    d_grid, d_sq, d_ix, d_tmp = dev.from_numpy(taj), dev.DeviceBuffer(4 * nvox), dev.DeviceBuffer(4 * nvox), dev.DeviceBuffer(4 * nvox)

    def best(fn):
        return min(timeit(fn, reps, warm=1) for _ in range(2))

    def transform(target, index, grid=None):
        L.check(lib.pb3d_edt_resident(L.ctx(), C.c_void_p((grid or d_grid).ptr), ch, *shape, target, 0, C.c_void_p(d_sq.ptr),
                                      C.c_void_p(d_ix.ptr) if index else None, None))

    t_copy = best(lambda: L.check(lib.pb3d_d2d(L.ctx(), C.c_void_p(d_tmp.ptr), C.c_void_p(d_sq.ptr), 4 * nvox)))
    copy_GB_s = 8 * nvox / t_copy / 1e6                   # a copy of n bytes moves 2 n
    moved = {False: ch + 4 + 8 + 8, True: ch + 8 + 16 + 16}  # bytes per voxel the three passes read and write, without / with index

    def row(name, ms, index):
        yard = moved[index] * nvox / copy_GB_s / 1e6
        return {name + "_ms": round(ms, 4), name + "_copy_yardstick_ms": round(yard, 4), name + "_over_copy": round(ms / yard, 2)}

    r = {"op": "EDT", "name": "distance_transform: stored Taj grid, resident", "shape": list(shape), "channels": ch,
         "copy_GB_s": round(copy_GB_s, 1), "moved_B_per_voxel": [moved[False], moved[True]]}
    t_bg = best(lambda: transform(0, False))
    r.update(row("background", t_bg, False))
    r.update(row("background_indices", best(lambda: transform(0, True)), True))
    r.update(row("surface", best(lambda: transform(2, False)), False))
    g = dev.DeviceGrid(d_grid, taj.shape)
    out = dev.DeviceGrid(dev.DeviceBuffer(nvox * ch), taj.shape)
    r["close_radius2_ms"] = round(best(lambda: pb3d.close_grid_resident(g, 2, out=out)), 4)
    v, f = pb3d.meshify_colored_voxel_grid(taj, stride=1)[:2]
    vs = pb3d.smooth_mesh(v, f)
    d_v, d_f = dev.from_numpy(vs), dev.from_numpy(f)
    d_m = pb3d.voxelize_mesh_resident(d_v, len(vs), d_f, len(f), shape, frame="meshify")
    gm = dev.DeviceGrid(d_m, shape)
    walls = []
    for _ in range(reps + 1):
        dev.sync()
        t0 = time.perf_counter()
        m = pb3d.grid_surface_metrics(g, gm, thresholds=(1.0, 2.0))
        walls.append(1e3 * (time.perf_counter() - t0))
    r["surface_metrics_vs_smoothed_mesh_wall_ms"] = round(min(walls[1:]), 3)
    r["surface_metrics"] = m
    transform(0, False)
    got = d_sq.download(shape, np.int32)
    if cpu_ref:
        occ = np.any(taj > 0, axis=-1)
        t0 = time.perf_counter()
        ref = ndi.distance_transform_edt(occ)
        r["scipy_edt_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        r["scipy_over_device"] = round(r["scipy_edt_ms"] / t_bg, 1)
        r["equals_scipy_bitwise"] = bool(np.array_equal(np.sqrt(got.astype(np.float64)), ref))
    print(json.dumps(r), flush=True)
    res.append(r)
    adversarial = {"full_but_one_corner": np.ones(shape, bool), "checkerboard": np.indices(shape).sum(axis=0) % 2 == 0}
    adversarial["full_but_one_corner"][0, 0, 0] = False
    for name, occ in adversarial.items():
        d_a = dev.from_numpy(np.repeat(occ.view(np.uint8)[..., None], ch, axis=-1))
        ra = {"op": "EDT", "name": "distance_transform: adversarial content " + name, "shape": list(shape), "channels": ch}
        for index in (False, True):
            key = "background_indices" if index else "background"
            ms = best(lambda: transform(0, index, d_a))
            ra.update(row(key, ms, index))
            ra[key + "_over_taj"] = round(ms / r[key + "_ms"], 2)
        if cpu_ref:
            transform(0, False, d_a)
            got = d_sq.download(shape, np.int32)
            t0 = time.perf_counter()
            ref = ndi.distance_transform_edt(occ)
            ra["scipy_edt_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            ra["equals_scipy_bitwise"] = bool(np.array_equal(np.sqrt(got.astype(np.float64)), ref))
        d_a.free()
        print(json.dumps(ra), flush=True)
        res.append(ra)
    for b in (d_grid, d_sq, d_ix, d_tmp, out, d_v, d_f, d_m):
        b.free()


def render(reps, res, cpu_ref=True):
    """RENDER, render_mesh (csrc/render.hip), resident, by device events (best mean of reps, the two host waits inside).  (a) The
    stride-1 mesh of the stored Taj grid as pb3d.device.meshify(download=False) hands it out (float32 vertices, int32 faces,
    nearest-voxel bytes, meshify's frame) under the stored final front camera at the size of that camera's mask: depth, face and colour
    image; depth alone; and under knob render_timing the call's own events per pass.  (b) One triangle that fills a 1024 x 768 image.
    (c) For context: a plain fill (pb3d_dev_memset) of 20 bytes per pixel (the depth image written twice, by the pre-fill and by the
    walk, and the face image once) and of the 36 of all three images (8 + 4 + 24), the grid-direct z-buffer of the same grid under the same camera, and with
    cpu_ref the NumPy restatement of tests/render_restate.py on a 64 x 48 crop of (a) on this host, and whether the device's crop equals it."""
    import render_restate as rr
    import pb3d.eval_helpers_intra as ev
    import pb3d.render as rd
    lib, L = pb3d._lib.load(), pb3d._lib
    g = os.path.join(ROOT, "tests", "golden")
    taj = np.ascontiguousarray(np.load(os.path.join(g, "stored_Taj_voxel_grid.npz"))["voxel_grid"])
    cam = ev.load_camera_json(os.path.join(g, "stored_Taj_camera_params_final.json"), "front")
    H, W = ev.resize_mask_to_voxel_grid(ev.load_mask(os.path.join(g, "data_Taj_front_mask.png")), taj).shape[:2]
    d_g = dev.from_numpy(taj)
    (dv, df, dn, dc), (nv, nf) = dev.meshify(d_g, taj.shape, stride=1, download=False)
    view = (cam["cam_pos"], cam["target"], cam["f"], cam["cx"], cam["cy"])

    def best(fn):
        return min(timeit(fn, reps, warm=1) for _ in range(2))

    def free(bufs):
        for b in bufs:
            b.free()

    def taj_call(colors=True, **kw):
        return rd.render_mesh_resident(dv, nv, df, nf, *view, H, W, dc if colors else None, 3, frame="meshify", depth=taj.shape[2], **kw)

    def passes(fn):
        L.set_tuning("render_timing", 1)
        rows = []
        try:
            for _ in range(reps + 1):
                free(fn())
                pm = (C.c_double * 5)()
                L.check(lib.pb3d_render_last_ms(L.ctx(), pm))
                rows.append(list(pm))
        finally:
            L.set_tuning("render_timing", 0)
        return dict(zip(("faces_depth_scan_wait_ms", "tiles_depth_ms", "faces_face_ms", "tiles_face_ms", "resolve_ms"),
                        (round(min(r[k] for r in rows[1:]), 4) for k in range(5))))

    def fill_ms(npix, bytes_per_pixel):
        d = dev.DeviceBuffer(npix * bytes_per_pixel)
        t = best(lambda: L.check(lib.pb3d_dev_memset(L.ctx(), C.c_void_p(d.ptr), 0, d.nbytes)))
        d.free()
        return round(t, 4)

    r = {"op": "RENDER", "name": "render_mesh: stored Taj, stride-1 mesh, final front camera", "image": [H, W], "nverts": int(nv), "nfaces": int(nf),
         "depth_face_image_ms": round(best(lambda: free(taj_call())), 4), "depth_face_ms": round(best(lambda: free(taj_call(False))), 4),
         **passes(lambda: taj_call(False, return_bary=True)), **rd.render_last(), "fill_20B_per_pixel_ms": fill_ms(H * W, 20),
         "fill_36B_per_pixel_ms": fill_ms(H * W, 36)}
    d_z = dev.DeviceBuffer(H * W * 4)
    r["grid_zbuffer_ms"] = round(best(lambda: ev.depth_buffer_resident(d_g, taj.shape, cam, H, W, out=d_z)), 4)
    res_d = taj_call()
    depth, face = res_d[0].download((H, W), np.float64), res_d[1].download((H, W), np.int32)
    free(res_d)
    zb = d_z.download((H, W), np.float32)
    both = np.isfinite(depth) & np.isfinite(zb)
    r.update(covered_pixels=int((face >= 0).sum()), zbuffer_pixels=int(np.isfinite(zb).sum()), covered_by_both=int(both.sum()),
             max_abs_depth_minus_zbuffer=round(float(np.abs(depth[both] - zb[both]).max()), 4))
    if cpu_ref:
        y0, x0 = int(np.argmax((face >= 0).any(axis=1))) + 40, W // 2 - 32        # a 64 x 48 window on the monument
        v, f = dv.download((nv, 3), np.float32), df.download((nf, 3), np.int32)
        R, c = rr.look_at(cam["cam_pos"], cam["target"])
        t0 = time.perf_counter()
        ref = rr.restate(v, f, R, c, cam["f"], cam["cx"] - x0, cam["cy"] - y0, 48, 64, frame=1, depth=float(taj.shape[2]))
        r["numpy_restatement_64x48_crop_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        crop = rd.render_mesh_resident(dv, nv, df, nf, cam["cam_pos"], cam["target"], cam["f"], cam["cx"] - x0, cam["cy"] - y0, 48, 64,
                                       frame="meshify", depth=taj.shape[2], return_bary=True)
        got = (crop[0].download((48, 64), np.float64), crop[1].download((48, 64), np.int32), crop[2].download((48, 64, 3), np.float64))
        free(crop)
        r["crop_covered_pixels"] = int((ref[1] >= 0).sum())
        r["crop_equals_restatement"] = bool(np.array_equal(rr.bits(got[0]), rr.bits(ref[0])) and np.array_equal(got[1], ref[1])
                                            and np.array_equal(got[2], ref[2]))
    print(json.dumps(r), flush=True)
    res.append(r)
    free((d_g, dv, df, dn, dc, d_z))

    Hb, Wb = 768, 1024
    tri = np.array([(-3.0, 3.0, 1.0), (9.0, 3.0, 1.0), (-3.0, -9.0, 1.0)], np.float32)       # covers u in [0, 1024), v in [0, 768) at f = 512
    d_t, d_i = dev.from_numpy(tri), dev.from_numpy(np.array([(0, 1, 2)], np.int32))
    d_c = dev.from_numpy(np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255)], np.uint8))
    origin = ((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 512.0, 511.5, 383.5)

    def tri_call(colors=True, **kw):
        return rd.render_mesh_resident(d_t, 3, d_i, 1, *origin, Hb, Wb, d_c if colors else None, 3, **kw)

    rb = {"op": "RENDER", "name": "render_mesh: one triangle filling the image", "image": [Hb, Wb], "nverts": 3, "nfaces": 1,
          "depth_face_image_ms": round(best(lambda: free(tri_call())), 4), "depth_face_ms": round(best(lambda: free(tri_call(False))), 4),
          **passes(lambda: tri_call(False, return_bary=True)), **rd.render_last(), "fill_20B_per_pixel_ms": fill_ms(Hb * Wb, 20),
          "fill_36B_per_pixel_ms": fill_ms(Hb * Wb, 36)}
    out = tri_call(False)
    rb["covered_pixels"] = int((out[1].download((Hb, Wb), np.int32) == 0).sum())
    free(out)
    free((d_t, d_i, d_c))
    print(json.dumps(rb), flush=True)
    res.append(rb)


def meshify(reps, res):
    """MESH, meshify_colored_voxel_grid (csrc/mesh.hip) on the stored Taj and Charminar grids at strides 1, 2 and 4: the resident
    form (count with its one host wait + fill into device buffers; device events) and the NumPy API (upload, count, fill, the four
    downloads; host wall clock, best of reps)."""
    import time
    for mon in ("Taj", "Charminar"):
        g = np.load(os.path.join(ROOT, "tests", "golden", f"stored_{mon}_voxel_grid.npz"))["voxel_grid"]
        d = dev.from_numpy(g)
        for s in (1, 2, 4):
            keep = []

            def run():
                bufs, counts = dev.meshify(d, g.shape, stride=s, download=False)
                keep.append((bufs, counts))
            ms = timeit(run, reps)
            nv, nf = keep[-1][1]
            for bufs, _ in keep:
                for b in bufs:
                    b.free()
            pb3d.meshify_colored_voxel_grid(g, stride=s)
            wall = []
            for _ in range(reps):
                t0 = time.perf_counter()
                pb3d.meshify_colored_voxel_grid(g, stride=s)
                wall.append(time.perf_counter() - t0)
            r = {"op": "MESH", "name": f"meshify_colored_voxel_grid, stored {mon}", "shape": list(g.shape), "stride": s,
                 "nverts": int(nv), "nfaces": int(nf), "resident_ms": round(ms, 4), "numpy_api_ms": round(1e3 * min(wall), 3)}
            print(json.dumps(r), flush=True)
            res.append(r)
        d.free()


def mesh_target(reps, res):
    """MESHD, a mesh as a comparison target (csrc/meshdist.hip) on the stored Taj grid at stride 1: every point of the grid
    (pb3d_points_extract_dev, float32, mapped into the mesh's frame) against the mesh meshify_colored_voxel_grid makes of it (float32 vertices, int32 faces, resident).
    MESHD/index: pb3d_mesh_dist_resident with ONE query -- the index check, the corner table, the box, the entry count(s), count / scan /
    scatter, with their host waits.  MESHD/dist: all points, index build included, and beside it the yardstick pb3d_nn_dist_dev (k = 1) of
    the same points against the mesh's VERTICES, its index build included too: the two are timed in turn, rep by rep, in the same run
    (device events; median and min / max of reps after one warm-up of each).  MESHD/sample: 1 M samples, the prefix and its two waits
    included."""
    from pb3d.eval_helpers import (mesh_grid_shape, nn_distances_resident, point_to_mesh_distances_resident, sample_mesh_points_resident)
    lib, L = pb3d._lib.load(), pb3d._lib
    taj = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    nvox = int(np.prod(taj.shape[:3]))
    d_g = dev.from_numpy(taj)
    d_tp, d_tc = dev.DeviceBuffer(nvox * 12), dev.DeviceBuffer(nvox * 3)
    n = C.c_int64(0)
    L.check(lib.pb3d_points_extract_dev(L.ctx(), C.c_void_p(d_g.ptr), *taj.shape[:3], 3, None, 0, nvox, C.c_void_p(d_tp.ptr),
                                        C.c_void_p(d_tc.ptr), C.byref(n)))
    npts = n.value
    pts = d_tp.download((npts, 3), np.float32)              # (a2, a1, a0); the mesh's frame is (a2, a1, shape[2] - a0) (csrc/mesh.hip)
    pts[:, 2] = np.float32(taj.shape[2]) - pts[:, 2]
    d_tp.upload(pts)
    (dv, df, dn, dc), (nv, nf) = dev.meshify(d_g, taj.shape, stride=1, download=False)
    d_nn = dev.DeviceBuffer(npts * 8)

    def once(fn):
        def run():
            for b in fn():
                if b is not None:
                    b.free()
        return timeit(run, 1, warm=0)

    def mesh_dist(nq):
        return lambda: point_to_mesh_distances_resident(d_tp, nq, dv, nv, df, nf, False, False, False, True, True)

    def vertex_nn():
        nn_distances_resident(d_tp, npts, dv, nv, 1, False, False, out=d_nn)
        return []

    def stats(t):
        return {"ms": round(float(np.median(t)), 4), "min_max_ms": [round(min(t), 4), round(max(t), 4)]}

    once(mesh_dist(1)); once(mesh_dist(npts)); once(vertex_nn)
    t_index, t_dist, t_nn = [], [], []
    for _ in range(reps):
        t_index.append(once(mesh_dist(1)))
        t_dist.append(once(mesh_dist(npts)))
        t_nn.append(once(vertex_nn))
    cells, entries, halvings = mesh_grid_shape()
    base = {"op": "MESHD", "grid_shape": list(taj.shape[:3]), "points": int(npts), "nverts": int(nv), "nfaces": int(nf), "reps": reps}
    rows = [dict(base, name="index build + one query (pb3d_mesh_dist_resident, nq = 1)", cells=list(cells), entries=int(entries),
                 entries_per_face=round(entries / nf, 3), halvings=int(halvings), **stats(t_index)),
            dict(base, name="point_to_mesh_distances_resident: every grid point -> its own mesh (distance, face, closest point)",
                 Mquery_s=round(npts / float(np.median(t_dist)) / 1e3, 1), **stats(t_dist)),
            dict(base, name="yardstick: pb3d_nn_dist_dev k = 1, the same points -> the mesh's vertices", Mquery_s=round(npts / float(np.median(t_nn)) / 1e3, 1),
                 **stats(t_nn))]
    rows[1]["ratio_to_vertex_nn"] = round(float(np.median(t_dist)) / float(np.median(t_nn)), 2)
    once(lambda: sample_mesh_points_resident(dv, nv, df, nf, 1000000, 0, False, False))
    t_s = [once(lambda: sample_mesh_points_resident(dv, nv, df, nf, 1000000, 0, False, False)) for _ in range(reps)]
    rows.append(dict(base, name="sample_mesh_points_resident: 1 000 000 samples with their faces", Msample_s=round(1e3 / float(np.median(t_s)), 1),
                     **stats(t_s)))
    for r in rows:
        print(json.dumps(r), flush=True)
        res.append(r)
    for b in (d_g, d_tp, d_tc, dv, df, dn, dc, d_nn):
        b.free()


def inside(reps, res):
    """INSIDE, points_in_mesh (csrc/inside.hip) against the stride-1 mesh of the stored Taj grid (float32 vertices, int32 faces, resident,
    meshify's frame), every call whole: index build and host waits included, by device events, the variants of a row timed in turn, rep
    by rep, in the same run (median and min / max of reps after one warm-up of each).
    INSIDE/lattice: every sample point of the grid (the points voxelize_mesh decides), mapped into the mesh's frame, in the grid's order;
      the flags must equal the grid's occupancy or the op stops.  In that frame the rays run along the grid's first axis, so a wavefront
      of consecutive queries holds 64 columns: timed in input order and in cell order (knob inside_order), each with the call's own
      index / query split (knob inside_timing), beside the yardstick voxelize_mesh of the same mesh into the same grid.
    INSIDE/lattice_a2: the same with the mesh mapped into the lattice frame instead, rays along a2 as the voxelization's: a wavefront
      shares one column, and the flags must equal voxelize_mesh's bytes.
    INSIDE/points: the grid's own points (the queries of MESHD) -- containment in both orders beside point_to_mesh_distances and the
      signed distance on the same queries.
    INSIDE/sfm20k: the 20 k SfM sample in the mesh's frame -- containment with its stats, the unsigned and the signed distance.
    INSIDE/order: shuffled samples of the grid's points from 20 k to all of them, input order against cell order: where the query
      binning starts to pay.
    Set-ups recomputed from the corner rows against the table of finished set-ups (knob inside_table) beside every lattice row."""
    from pb3d.eval_helpers import point_to_mesh_distances_resident
    lib, L = pb3d._lib.load(), pb3d._lib
    taj = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    shape = taj.shape[:3]
    nvox = int(np.prod(shape))
    occ = np.any(taj > 0, axis=-1)
    D = np.float32(shape[2])
    d_g = dev.from_numpy(taj)
    (dv, df, dn, dc), (nv, nf) = dev.meshify(d_g, taj.shape, stride=1, download=False)
    for b in (d_g, dn, dc):
        b.free()
    verts = dv.download((nv, 3), np.float32)
    ijk = np.indices(shape, dtype=np.float32).reshape(3, -1).T
    q_mesh = np.ascontiguousarray(np.stack([ijk[:, 2], ijk[:, 1], D - ijk[:, 0]], axis=1))      # voxel (i, j, k) in meshify's frame
    d_lattice, d_ijk = dev.from_numpy(q_mesh), dev.from_numpy(np.ascontiguousarray(ijk))
    d_vl = dev.from_numpy(np.ascontiguousarray(np.stack([D - verts[:, 2], verts[:, 1], verts[:, 0]], axis=1)))   # the mesh in the lattice frame
    pts = q_mesh[occ.reshape(-1)]
    d_pts = dev.from_numpy(pts)
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "inter_ref.json")))
    scale = float.fromhex(meta["taj_transform"]["scale"])
    offset = np.array([float.fromhex(v) for v in meta["taj_transform"]["offset"]])
    sfm = np.load(os.path.join(ROOT, "tests", "golden", "inter_sfm20k.npz"))["sfm"]
    sfm_vox = ((sfm - offset) / scale)[:, ::-1]                                                   # (a2, a1, a0)
    sfm_mesh = np.ascontiguousarray(np.stack([sfm_vox[:, 0], sfm_vox[:, 1], float(D) - sfm_vox[:, 2]], axis=1))
    d_sfm = dev.from_numpy(sfm_mesh)
    d_in, d_vox = dev.DeviceBuffer(nvox), dev.DeviceBuffer(nvox)

    def contain(d_q, n, f64, d_verts=dv, order=0, table=0, **kw):
        def run():
            L.set_tuning("inside_order", order)
            L.set_tuning("inside_table", table)
            try:
                return pb3d.points_in_mesh_resident(d_q, n, d_verts, nv, df, nf, f64, False, False, out=d_in, **kw)
            finally:
                L.set_tuning("inside_order", 0)
                L.set_tuning("inside_table", 0)
        return run

    def once(fn):
        def run():
            out = fn()
            for b in (out if isinstance(out, tuple) else (out,)):
                if isinstance(b, dev.DeviceBuffer) and b is not d_in and b is not d_vox:
                    b.free()
        return timeit(run, 1, warm=0)

    def stats(t):
        return {"ms": round(float(np.median(t)), 4), "min_max_ms": [round(min(t), 4), round(max(t), 4)]}

    def in_turn(fns):
        """every variant once as a warm-up, then reps rounds of all of them in turn"""
        for fn in fns.values():
            once(fn)
        t = {k: [] for k in fns}
        for _ in range(reps):
            for k, fn in fns.items():
                t[k].append(once(fn))
        return t

    def split(fn):
        """(index ms, query ms) of the call's own events: the best of reps after one warm-up"""
        L.set_tuning("inside_timing", 1)
        try:
            got = []
            for _ in range(reps + 1):
                fn()
                got.append(pb3d.points_in_mesh_last(timed=True))
        finally:
            L.set_tuning("inside_timing", 0)
        return got[-1][:3], min(g[3][0] for g in got[1:]), min(g[3][1] for g in got[1:])

    base = {"grid_shape": list(shape), "nverts": int(nv), "nfaces": int(nf), "reps": reps}
    rows = []

    # ---- 1: the grid's sample points; equality first
    _, st = contain(d_lattice, nvox, False, return_stats=True)()
    got = d_in.download(shape)
    assert np.array_equal(got != 0, occ), "points_in_mesh at the grid's sample points differs from the grid's occupancy"
    contain(d_lattice, nvox, False, order=1)()
    assert np.array_equal(d_in.download(shape), got), "the query order changed a byte"
    pb3d.voxelize_mesh_resident(dv, nv, df, nf, shape, frame="meshify", out=d_vox)
    contain(d_ijk, nvox, False, d_verts=d_vl)()
    assert np.array_equal(d_in.download(shape), d_vox.download(shape)), "lattice frame: points_in_mesh differs from voxelize_mesh"
    for order in (0, 1):
        contain(d_lattice, nvox, False, order=order, table=1)()
        assert np.array_equal(d_in.download(shape), got), "the set-up table changed a byte"
    fns = {"input_order": contain(d_lattice, nvox, False), "cell_order": contain(d_lattice, nvox, False, order=1),
           "input_order_table": contain(d_lattice, nvox, False, table=1), "cell_order_table": contain(d_lattice, nvox, False, order=1, table=1),
           "lattice_frame": contain(d_ijk, nvox, False, d_verts=d_vl), "lattice_frame_cell_order": contain(d_ijk, nvox, False, d_verts=d_vl, order=1),
           "lattice_frame_table": contain(d_ijk, nvox, False, d_verts=d_vl, table=1),
           "voxelize": lambda: pb3d.voxelize_mesh_resident(dv, nv, df, nf, shape, frame="meshify", out=d_vox)}
    t = in_turn(fns)
    for key, op, name, d_q, d_verts, order, table in (
            ("input_order", "INSIDE/lattice", "every sample point of the grid, mesh frame, input order", d_lattice, dv, 0, 0),
            ("cell_order", "INSIDE/lattice", "every sample point of the grid, mesh frame, cell order (inside_order = 1)", d_lattice, dv, 1, 0),
            ("input_order_table", "INSIDE/lattice", "every sample point of the grid, mesh frame, input order, set-up table (inside_table = 1)",
             d_lattice, dv, 0, 1),
            ("cell_order_table", "INSIDE/lattice", "every sample point of the grid, mesh frame, cell order, set-up table", d_lattice, dv, 1, 1),
            ("lattice_frame", "INSIDE/lattice_a2", "every sample point of the grid, lattice frame (rays along a2), input order", d_ijk, d_vl, 0, 0),
            ("lattice_frame_cell_order", "INSIDE/lattice_a2", "every sample point of the grid, lattice frame, cell order", d_ijk, d_vl, 1, 0),
            ("lattice_frame_table", "INSIDE/lattice_a2", "every sample point of the grid, lattice frame, input order, set-up table", d_ijk, d_vl, 0, 1)):
        (cells, entries, halvings), ms_index, ms_query = split(contain(d_q, nvox, False, d_verts=d_verts, order=order, table=table))
        rows.append(dict(base, op=op, name="points_in_mesh: " + name, queries=nvox, **stats(t[key]), Mquery_s=round(nvox / float(np.median(t[key])) / 1e3, 1),
                         index_ms=round(ms_index, 4), query_ms=round(ms_query, 4), index_share=round(ms_index / (ms_index + ms_query), 4),
                         cells=list(cells), entries=entries, entries_per_face=round(entries / nf, 3), halvings=halvings,
                         ratio_to_voxelize=round(float(np.median(t[key])) / float(np.median(t["voxelize"])), 1),
                         equals_occupancy=True, **(st if key == "input_order" else {})))
    rows.append(dict(base, op="INSIDE/lattice", name="yardstick: voxelize_mesh of the same mesh into the same grid", **stats(t["voxelize"])))

    # ---- 2 and 3: the grid's own points and the SfM sample; containment, distance, signed distance
    for tag, d_q, n, f64, host in (("points", d_pts, len(pts), False, pts), ("sfm20k", d_sfm, len(sfm_mesh), True, sfm_mesh)):
        _, st = contain(d_q, n, f64, return_stats=True)()
        fns = {"input_order": contain(d_q, n, f64), "cell_order": contain(d_q, n, f64, order=1), "table": contain(d_q, n, f64, table=1),
               "dist": lambda d_q=d_q, n=n, f64=f64: point_to_mesh_distances_resident(d_q, n, dv, nv, df, nf, f64, False, False),
               "signed": lambda d_q=d_q, n=n, f64=f64: pb3d.signed_point_to_mesh_distances_resident(d_q, n, dv, nv, df, nf, f64, False, False)}
        t = in_turn(fns)
        (cells, entries, halvings), ms_index, ms_query = split(contain(d_q, n, f64))
        med = {k: float(np.median(v)) for k, v in t.items()}
        what = "the grid's own points (MESHD's queries)" if tag == "points" else "the 20 k SfM sample in the mesh's frame"
        rows.append(dict(base, op="INSIDE/" + tag, name=f"points_in_mesh: {what}, input order", queries=int(n), **stats(t["input_order"]),
                         Mquery_s=round(n / med["input_order"] / 1e3, 1), index_ms=round(ms_index, 4), query_ms=round(ms_query, 4),
                         index_share=round(ms_index / (ms_index + ms_query), 4), ratio_to_unsigned_distance=round(med["input_order"] / med["dist"], 4),
                         fraction_outside=round(1.0 - st["inside"] / n, 4), **st))
        rows.append(dict(base, op="INSIDE/" + tag, name=f"points_in_mesh: {what}, cell order (inside_order = 1)", queries=int(n),
                         **stats(t["cell_order"]), ratio_to_input_order=round(med["cell_order"] / med["input_order"], 3)))
        rows.append(dict(base, op="INSIDE/" + tag, name=f"points_in_mesh: {what}, input order, set-up table (inside_table = 1)", queries=int(n),
                         **stats(t["table"]), ratio_to_input_order=round(med["table"] / med["input_order"], 3)))
        rows.append(dict(base, op="INSIDE/" + tag, name=f"yardstick: point_to_mesh_distances_resident, {what}", queries=int(n), **stats(t["dist"])))
        rows.append(dict(base, op="INSIDE/" + tag, name=f"signed_point_to_mesh_distances_resident, {what}", queries=int(n), **stats(t["signed"]),
                         ratio_to_unsigned_distance=round(med["signed"] / med["dist"], 4)))
    # ---- where the cell order starts to pay: shuffled samples of the grid's points (a cloud's order says nothing about its cells)
    rng = np.random.default_rng(0)
    for n in (20000, 100000, 300000, 1000000, 3000000, len(pts)):
        d_s = dev.from_numpy(pts[rng.permutation(len(pts))[:n]])
        t = in_turn({"input_order": contain(d_s, n, False), "cell_order": contain(d_s, n, False, order=1)})
        med = {k: float(np.median(v)) for k, v in t.items()}
        rows.append(dict(base, op="INSIDE/order", name="points_in_mesh: a shuffled sample of the grid's points, input order against cell order",
                         queries=int(n), input_order_ms=round(med["input_order"], 4), cell_order_ms=round(med["cell_order"], 4),
                         cell_over_input=round(med["cell_order"] / med["input_order"], 3),
                         min_max_ms={k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}))
        d_s.free()
    for r in rows:
        print(json.dumps(r), flush=True)
        res.append(r)
    for b in (dv, df, d_lattice, d_ijk, d_vl, d_pts, d_sfm, d_in, d_vox):
        b.free()


def raycast(reps, res):
    """RAYCAST, cast_rays / rays_occluded (csrc/raycast.hip) against the stride-1 mesh of the stored Taj grid (float32 vertices, int32
    faces, resident, meshify's frame), every call whole: index build and host waits included, by device events, a row's call and its
    yardstick timed in turn, rep by rep, in the same run (median and min / max of reps after one warm-up of each).  Every row carries the
    call's own index / query split (knob raycast_timing) and face tests and cells per ray (knob raycast_stats); the rows also go to
    profiles/raycast_opbench.jsonl.
    RAYCAST/camera: the H x W rays of the stored final front camera (camera_rays, mapped into the mesh's frame), first hit, beside
      render_mesh of the same view (depth and face); the share of pixels whose face agrees is reported, no bit equality is claimed.
    RAYCAST/occlusion: the segments from the grid's own points (MESHD's queries) to that camera's centre, any hit on [1e-6, 1], beside
      point_to_mesh_distances on the same queries.
    RAYCAST/random: 1 M rays with uniform origins in the box of the vertices and normal directions, first hit and any hit."""
    import pb3d.eval_helpers_intra as ev
    import pb3d.render as rd
    from pb3d.eval_helpers import point_to_mesh_distances_resident
    L = pb3d._lib
    g = os.path.join(ROOT, "tests", "golden")
    taj = np.ascontiguousarray(np.load(os.path.join(g, "stored_Taj_voxel_grid.npz"))["voxel_grid"])
    shape = taj.shape[:3]
    D = float(shape[2])
    cam = ev.load_camera_json(os.path.join(g, "stored_Taj_camera_params_final.json"), "front")
    H, W = ev.resize_mask_to_voxel_grid(ev.load_mask(os.path.join(g, "data_Taj_front_mask.png")), taj).shape[:2]
    d_g = dev.from_numpy(taj)
    (dv, df, dn, dc), (nv, nf) = dev.meshify(d_g, taj.shape, stride=1, download=False)
    for b in (d_g, dn, dc):
        b.free()
    verts = dv.download((nv, 3), np.float32)
    to_mesh = lambda p: np.ascontiguousarray(np.stack([p[:, 0], p[:, 1], D - p[:, 2]], axis=1))       # noqa: E731  (points frame -> meshify's)
    view = (cam["cam_pos"], cam["target"], cam["f"], cam["cx"], cam["cy"])

    def stats(t):
        return {"ms": round(float(np.median(t)), 4), "min_max_ms": [round(min(t), 4), round(max(t), 4)]}

    def once(fn):
        def run():
            out = fn()
            for b in (out if isinstance(out, tuple) else (out,)):
                if isinstance(b, dev.DeviceBuffer):
                    b.free()
        return timeit(run, 1, warm=0)

    def in_turn(fns):
        for fn in fns.values():
            once(fn)
        t = {k: [] for k in fns}
        for _ in range(reps):
            for k, fn in fns.items():
                t[k].append(once(fn))
        return t

    def own(fn, n):
        """the call's own events (best of reps after a warm-up) and its counts"""
        L.set_tuning("raycast_timing", 1)
        L.set_tuning("raycast_stats", 1)
        try:
            ms = []
            for _ in range(reps + 1):
                once(fn)
                ms.append(pb3d.cast_rays_last(timed=True))
            st = pb3d.cast_rays_last()
        finally:
            L.set_tuning("raycast_timing", 0)
            L.set_tuning("raycast_stats", 0)
        i_ms, q_ms = min(m[0] for m in ms[1:]), min(m[1] for m in ms[1:])
        return dict(index_ms=round(i_ms, 4), query_ms=round(q_ms, 4), index_share=round(i_ms / (i_ms + q_ms), 4),
                    face_tests_per_ray=round(st["face_tests"] / n, 2), cells_per_ray=round(st["cells"] / n, 2),
                    entries_per_face=round(st["entries"] / nf, 3), **st)

    base = {"grid_shape": list(shape), "nverts": int(nv), "nfaces": int(nf), "reps": reps}
    rows = []

    # ---- (a) the camera's rays beside render_mesh
    o, d = pb3d.camera_rays(*view, H, W)
    n = H * W
    d_o, d_d = dev.from_numpy(to_mesh(o)), dev.from_numpy(np.ascontiguousarray(d * np.array([1.0, 1.0, -1.0])))
    first = lambda: pb3d.cast_rays_resident(d_o, d_d, n, dv, nv, df, nf, 1e-6, np.inf)                 # noqa: E731
    render = lambda: rd.render_mesh_resident(dv, nv, df, nf, *view, H, W, frame="meshify", depth=shape[2])   # noqa: E731
    a, b = first(), render()
    face_r, face_c = b[1].download((H, W), np.int32), a[1].download((n,), np.int32).reshape(H, W)
    t_r, t_c = b[0].download((H, W), np.float64), a[0].download((n,), np.float64).reshape(H, W)
    for x in a + b:
        x.free()
    both = (face_r >= 0) & (face_c >= 0)
    t = in_turn({"cast": first, "render": render})
    med = {k: float(np.median(v)) for k, v in t.items()}
    rows.append(dict(base, op="RAYCAST/camera", name="cast_rays: the rays of the stored final front camera, first hit", rays=n, image=[H, W],
                     **stats(t["cast"]), Mray_s=round(n / med["cast"] / 1e3, 2), ratio_to_render_mesh=round(med["cast"] / med["render"], 3),
                     hit_pixels=int((face_c >= 0).sum()), render_hit_pixels=int((face_r >= 0).sum()),
                     same_face_share=round(float((face_r == face_c).mean()), 6),
                     max_depth_difference=float(np.abs(t_r[both] - t_c[both]).max()) if both.any() else 0.0, **own(first, n)))
    rows.append(dict(base, op="RAYCAST/camera", name="yardstick: render_mesh of the same view (depth and face)", image=[H, W], **stats(t["render"])))
    d_o.free()
    d_d.free()

    # ---- (b) occlusion of the grid's own points towards the camera's centre beside the nearest-point search
    occ = np.any(taj > 0, axis=-1)
    ijk = np.argwhere(occ).astype(np.float64)
    pts = np.ascontiguousarray(np.stack([ijk[:, 2], ijk[:, 1], D - ijk[:, 0]], axis=1))                 # voxel (i, j, k) in meshify's frame
    n = len(pts)
    eye = to_mesh(np.asarray(cam["cam_pos"], np.float64)[None, :])[0]
    d_o, d_d = dev.from_numpy(pts), dev.from_numpy(np.ascontiguousarray(eye[None, :] - pts))
    hidden = lambda: pb3d.rays_occluded_resident(d_o, d_d, n, dv, nv, df, nf, 1e-6, 1.0)               # noqa: E731
    dist = lambda: point_to_mesh_distances_resident(d_o, n, dv, nv, df, nf, True, False, False)        # noqa: E731
    t = in_turn({"occluded": hidden, "dist": dist})
    med = {k: float(np.median(v)) for k, v in t.items()}
    rows.append(dict(base, op="RAYCAST/occlusion", name="rays_occluded: the grid's own points towards the camera's centre, any hit on [1e-6, 1]",
                     rays=n, **stats(t["occluded"]), Mray_s=round(n / med["occluded"] / 1e3, 2),
                     ratio_to_point_to_mesh_distances=round(med["occluded"] / med["dist"], 3), **own(hidden, n)))
    rows[-1]["visible_share"] = round(1.0 - rows[-1]["hits"] / n, 4)
    rows.append(dict(base, op="RAYCAST/occlusion", name="yardstick: point_to_mesh_distances_resident on the same queries", queries=n,
                     **stats(t["dist"])))
    d_o.free()
    d_d.free()

    # ---- (c) scattered rays: uniform origins in the box, normal directions
    rng = np.random.default_rng(0)
    n = 1000000
    lo, hi = verts.min(axis=0).astype(np.float64), verts.max(axis=0).astype(np.float64)
    d_o, d_d = dev.from_numpy(rng.uniform(lo, hi, (n, 3))), dev.from_numpy(rng.normal(size=(n, 3)))
    first = lambda: pb3d.cast_rays_resident(d_o, d_d, n, dv, nv, df, nf)                                # noqa: E731
    anyh = lambda: pb3d.rays_occluded_resident(d_o, d_d, n, dv, nv, df, nf)                             # noqa: E731
    t = in_turn({"first": first, "any": anyh})
    med = {k: float(np.median(v)) for k, v in t.items()}
    rows.append(dict(base, op="RAYCAST/random", name="cast_rays: 1 M rays, uniform origins in the box, normal directions, first hit", rays=n,
                     **stats(t["first"]), Mray_s=round(n / med["first"] / 1e3, 2), **own(first, n)))
    rows.append(dict(base, op="RAYCAST/random", name="rays_occluded: the same rays, any hit", rays=n, **stats(t["any"]),
                     Mray_s=round(n / med["any"] / 1e3, 2), ratio_to_first_hit=round(med["any"] / med["first"], 3), **own(anyh, n)))
    with open(os.path.join(ROOT, "profiles", "raycast_opbench.jsonl"), "w") as fh:
        for r in rows:
            print(json.dumps(r), flush=True)
            fh.write(json.dumps(r) + "\n")
            res.append(r)
    for b in (dv, df, d_o, d_d):
        b.free()


def density(reps, res, cpu_ref=True):
    """DENS, pointcloud_to_voxel_grid (csrc/density.hip) on every point of the stored Taj grid (pb3d_points_extract_dev, float32) at
    grid_size 128 and 512, sigma 1: the resident form (bounds with their one host wait, clear, scatter, three filter passes; device
    events), the NumPy API (upload, the same, download of the volume; host wall clock, best of reps) and, with cpu_ref, the reference's
    composition -- normalisation, np.add.at, scipy.ndimage.gaussian_filter, zero faces -- on this host and the same input (context
    only: one CPU measurement, and the reference itself samples 20-50 k points first)."""
    from pb3d.eval_helpers import density_grid_resident
    from pb3d.preprocess_helpers import normalize_preserve_aspect
    lib, L = pb3d._lib.load(), pb3d._lib
    taj = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    nvox = int(np.prod(taj.shape[:3]))
    d_g = dev.from_numpy(taj)
    d_tp, d_tc = dev.DeviceBuffer(nvox * 12), dev.DeviceBuffer(nvox * 3)
    n = C.c_int64(0)
    L.check(lib.pb3d_points_extract_dev(L.ctx(), C.c_void_p(d_g.ptr), *taj.shape[:3], 3, None, 0, nvox, C.c_void_p(d_tp.ptr),
                                        C.c_void_p(d_tc.ptr), C.byref(n)))
    npts = n.value
    pts = d_tp.download((npts, 3), np.float32)
    for G in (128, 512):
        d_out = dev.DeviceBuffer(G ** 3 * 4)
        ms = timeit(lambda: density_grid_resident(d_tp, npts, G, 1.0, f64=False, out=d_out), reps)
        got = d_out.download((G, G, G), np.float32)
        d_out.free()
        pb3d.pointcloud_to_voxel_grid(pts, G, 1.0)
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            pb3d.pointcloud_to_voxel_grid(pts, G, 1.0)
            wall.append(time.perf_counter() - t0)
        r = {"op": "DENS", "name": "pointcloud_to_voxel_grid, every point of the stored Taj grid", "grid_shape": list(taj.shape[:3]),
             "points": int(npts), "grid_size": G, "sigma": 1.0, "resident_ms": round(ms, 4), "numpy_api_ms": round(1e3 * min(wall), 3)}
        if cpu_ref:
            from scipy.ndimage import gaussian_filter
            t0 = time.perf_counter()
            idx = (normalize_preserve_aspect(pts) * (G - 1)).astype(int)
            vol = np.zeros((G, G, G), np.float32)
            np.add.at(vol, (idx[:, 0], idx[:, 1], idx[:, 2]), 1)
            vol = gaussian_filter(vol, sigma=1.0)
            vol[[0, -1], :, :] = 0
            vol[:, [0, -1], :] = 0
            vol[:, :, [0, -1]] = 0
            r["reference_cpu_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            r["equal_bits"] = bool(np.array_equal(vol.view(np.uint32), got.view(np.uint32)))
        print(json.dumps(r), flush=True)
        res.append(r)
    for b in (d_g, d_tp, d_tc):
        b.free()


def isosurface(reps, res):
    """ISO, the isosurface of a resident density volume (pb3d_iso_*, csrc/mesh.hip) at level 0.1, divisor grid_size: (a) the default
    case of get_marching_cubes_mesh, the 128^3 volume of the 20 k SfM sample; (b) the 512^3 volume of every point of the stored Taj
    grid.  resident_ms: count with its one host wait + fill into new device buffers, by device events (mean of reps after two warm
    calls).  passes_ms: under knob iso_timing the calls' own events -- bits pass, count and its two scans, vertex pass, faces (median
    of reps; the fill then waits once more, so these runs are not the ones resident_ms times).  Two yardsticks that are not the code
    under test, in the same run: device.meshify(download=False) on a uint8 (G, G, G, 1) grid holding the same sign mask (the same
    topology passes on 1 B per voxel, plus normals and colours), and the plain sweep A2 (_occupancy: 3 B read + 1 B written per
    element) over G^3 elements, the floor of a pass that reads 4 B per voxel once."""
    from pb3d.eval_helpers import density_grid_resident
    lib, L = pb3d._lib.load(), pb3d._lib
    sfm = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "inter_sfm20k.npz"))["sfm"])
    taj = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    nvox = int(np.prod(taj.shape[:3]))
    d_g = dev.from_numpy(taj)
    d_tp, d_tc = dev.DeviceBuffer(nvox * 12), dev.DeviceBuffer(nvox * 3)
    n = C.c_int64(0)
    L.check(lib.pb3d_points_extract_dev(L.ctx(), C.c_void_p(d_g.ptr), *taj.shape[:3], 3, None, 0, nvox, C.c_void_p(d_tp.ptr),
                                        C.c_void_p(d_tc.ptr), C.byref(n)))
    d_g.free(); d_tc.free()
    d_sfm = dev.from_numpy(sfm)
    for name, d_p, npts, f64, G in (("20 k SfM sample", d_sfm, len(sfm), True, 128), ("every point of the stored Taj grid", d_tp, n.value, False, 512)):
        d_vol = density_grid_resident(d_p, npts, G, 1.0, f64=f64)
        shape = (G, G, G)
        keep = []

        def run():
            keep.append(dev.isosurface(d_vol, shape, 0.1, G, download=False))

        def drop():
            for bufs, _ in keep:
                for b in bufs:
                    b.free()
            del keep[:]
        ms = timeit(run, reps)
        nv, nf = keep[-1][1]
        drop()
        L.set_tuning("iso_timing", 1)
        passes = []
        try:
            for _ in range(max(3, reps)):
                run()
                pm = (C.c_double * 4)()
                L.check(lib.pb3d_iso_last(L.ctx(), pm))
                passes.append(list(pm))
                drop()
        finally:
            L.set_tuning("iso_timing", 0)
        bits_ms, count_ms, verts_ms, faces_ms = (float(x) for x in np.median(np.array(passes), axis=0))
        # yardstick 1: meshify on the same sign mask
        mask = (d_vol.download(shape, np.float32).astype(np.float64) > 0.1).astype(np.uint8)[..., None] * np.uint8(255)
        d_m = dev.from_numpy(mask)
        mkeep = []

        def mrun():
            mkeep.append(dev.meshify(d_m, mask.shape, stride=1, download=False))
        mesh_ms = timeit(mrun, reps)
        mnv, mnf = mkeep[-1][1]
        for bufs, _ in mkeep:
            for b in bufs:
                b.free()
        d_m.free()
        # yardstick 2: the plain sweep over G^3 elements of 4 B
        d_c, d_o = dev.DeviceBuffer(G ** 3 * 3), dev.DeviceBuffer(G ** 3)
        d_c.zero()
        sweep_ms = timeit(lambda: dev.occupancy(d_c, G ** 3, d_o), 20)
        d_c.free(); d_o.free()
        r = {"op": "ISO", "name": f"isosurface of the density volume, {name}", "points": int(npts), "grid_size": G, "sigma": 1.0, "level": 0.1,
             "nverts": int(nv), "nfaces": int(nf), "resident_ms": round(ms, 4),
             "passes_ms": {"bits": round(bits_ms, 4), "count_and_scans": round(count_ms, 4), "verts": round(verts_ms, 4), "faces": round(faces_ms, 4)},
             "bits_GB_s": round(4 * G ** 3 / bits_ms / 1e6, 1),
             "yardstick_meshify_same_mask_resident_ms": round(mesh_ms, 4), "meshify_same_counts": bool((mnv, mnf) == (nv, nf)),
             "yardstick_sweep_4B_per_voxel_ms": round(sweep_ms, 4), "sweep_GB_s": round(4 * G ** 3 / sweep_ms / 1e6, 1),
             "ratio_iso_to_meshify": round(ms / mesh_ms, 3), "ratio_bits_to_sweep": round(bits_ms / sweep_ms, 3)}
        print(json.dumps(r), flush=True)
        res.append(r)
        d_vol.free()
    d_sfm.free(); d_tp.free()


def mesh_components(reps, res):
    """MESHCOMP, mesh_components, select_faces and keep_mesh_components (csrc/meshcomp.hip, csrc/simplify.hip) on the meshes of the
    SIMPLIFY and ISO rows: the stride-1 mesh of the stored Taj grid and the 512^3 isosurface of the density volume of its points at level
    0.1.  Resident, by device events (best mean of reps, host waits inside): the labelling under both connectivities, without and with
    the measures; mesh_topology; keep_mesh_components(k=1) by faces; select_faces on keep's own mask.  Two yardsticks that are not the
    code under test, on the same mesh in the same run: mesh_vertex_adjacency_resident (it sorts 6 m pairs by two keys where the
    labelling sorts 3 m records) and compact_mesh_resident with duplicate_faces="keep" (the select tail's passes on every face)."""
    from pb3d import meshcomp as mcp, simplify as sm, smooth as smo
    from pb3d.eval_helpers import density_grid_resident
    lib, L = pb3d._lib.load(), pb3d._lib
    taj = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    nvox = int(np.prod(taj.shape[:3]))
    d_g = dev.from_numpy(taj)

    def best(fn):
        return min(timeit(fn, reps, warm=1) for _ in range(2))

    def free(bufs):
        for b in bufs:
            if hasattr(b, "free"):
                b.free()

    def taj_mesh():
        (d_v, d_f, d_n, d_c), (nv, nf) = dev.meshify(d_g, taj.shape, download=False)
        free((d_n, d_c))
        return d_v, d_f, nv, nf

    def iso_mesh():
        d_tp, d_tc = dev.DeviceBuffer(nvox * 12), dev.DeviceBuffer(nvox * 3)
        n = C.c_int64(0)
        L.check(lib.pb3d_points_extract_dev(L.ctx(), C.c_void_p(d_g.ptr), *taj.shape[:3], 3, None, 0, nvox, C.c_void_p(d_tp.ptr),
                                            C.c_void_p(d_tc.ptr), C.byref(n)))
        d_vol = density_grid_resident(d_tp, n.value, 512, 1.0, f64=False)
        (d_v, d_f), (nv, nf) = dev.isosurface(d_vol, (512, 512, 512), 0.1, 512, download=False)
        free((d_tp, d_tc, d_vol))
        return d_v, d_f, nv, nf

    for name, make in (("stored Taj, stride-1 mesh", taj_mesh), ("512^3 isosurface of the Taj density volume, level 0.1", iso_mesh)):
        d_v, d_f, nv, nf = make()
        r = {"op": "MESHCOMP", "name": f"mesh_components: {name}", "nverts": int(nv), "nfaces": int(nf), "records": 3 * int(nf), "reps": reps}
        for conn in ("edge", "vertex"):
            for measured in (False, True):
                def call():
                    *bufs, t = mcp.mesh_components_resident(d_f, nf, nv, d_v if measured else None, conn)
                    free(bufs)
                    return t
                r[f"{conn}{'_measured' if measured else ''}_ms"] = round(best(call), 4)
            r[f"{conn}_components"] = call()["components"]
        t = mcp.mesh_topology_resident(d_f, nf, nv)
        r.update({"topology_ms": round(best(lambda: mcp.mesh_topology_resident(d_f, nf, nv)), 4),
                  "topology": {k: t[k] for k in mcp.TOTALS + ("euler", "closed", "edge_manifold", "watertight")}})

        def keep():
            out, d_lab, chosen = mcp.keep_mesh_components_resident(d_v, nv, d_f, nf, k=1)
            free(out[:6] + (d_lab,))
            return out[6]
        r["keep_k1_ms"] = round(best(keep), 4)
        r["keep_k1_counts"] = list(keep())
        d_keep = dev.from_numpy(np.ones(nf, np.uint8))
        r["select_all_ms"] = round(best(lambda: free(mcp.select_faces_resident(d_v, nv, d_f, nf, d_keep)[:6])), 4)
        # the yardsticks
        r["yardstick_adjacency_ms"] = round(best(lambda: free(smo.mesh_vertex_adjacency_resident(d_f, nv, nf)[:4])), 4)
        r["yardstick_compact_keep_ms"] = round(best(lambda: free(sm.compact_mesh_resident(d_v, nv, d_f, nf, duplicate_faces="keep")[:6])), 4)
        r.update({"edge_over_adjacency": round(r["edge_ms"] / r["yardstick_adjacency_ms"], 3),
                  "vertex_over_adjacency": round(r["vertex_ms"] / r["yardstick_adjacency_ms"], 3),
                  "edge_measured_over_adjacency": round(r["edge_measured_ms"] / r["yardstick_adjacency_ms"], 3),
                  "select_over_compact_keep": round(r["select_all_ms"] / r["yardstick_compact_keep_ms"], 3),
                  "keep_k1_over_edge_plus_compact": round(r["keep_k1_ms"] / (r["edge_ms"] + r["yardstick_compact_keep_ms"]), 3)})
        print(json.dumps(r), flush=True)
        res.append(r)
        free((d_v, d_f, d_keep))
    d_g.free()


def mesh_repair(reps, res, orient=True, weld=True):
    """ORIENT and WELD, mesh_orientation / orient_mesh (csrc/orient.hip) and weld_vertices (csrc/weld.hip) on the two meshes of the
    MESHCOMP rows.  Resident, by device events (best mean of reps, host waits inside).  ORIENT: mesh_orientation without vertices, with
    them and with the sign rule; orient_mesh on a copy with a seeded random half of the faces wound the other way.  Its yardstick, not
    the code under test, on the same faces in the same run: mesh_components_resident(connectivity="edge") without measures -- the same
    two sorts, half the unions and a forest half as long.  WELD: weld_vertices of the mesh's soup (three vertices of its own per
    face), float32 and float64.  Its yardsticks: mesh_vertex_adjacency_resident on the welded mesh (two sorts of 6 m pairs) and a
    device-to-device copy of the soup's vertex bytes."""
    from pb3d import meshcomp as mcp, orient as ori, smooth as smo, weld as wl
    from pb3d.eval_helpers import density_grid_resident
    lib, L = pb3d._lib.load(), pb3d._lib
    taj = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    nvox = int(np.prod(taj.shape[:3]))
    d_g = dev.from_numpy(taj)

    def best(fn):
        return min(timeit(fn, reps, warm=1) for _ in range(2))

    def free(bufs):
        for b in bufs:
            if hasattr(b, "free"):
                b.free()

    def taj_mesh():
        (d_v, d_f, d_n, d_c), (nv, nf) = dev.meshify(d_g, taj.shape, download=False)
        free((d_n, d_c))
        return d_v, d_f, nv, nf

    def iso_mesh():
        d_tp, d_tc = dev.DeviceBuffer(nvox * 12), dev.DeviceBuffer(nvox * 3)
        n = C.c_int64(0)
        L.check(lib.pb3d_points_extract_dev(L.ctx(), C.c_void_p(d_g.ptr), *taj.shape[:3], 3, None, 0, nvox, C.c_void_p(d_tp.ptr),
                                            C.c_void_p(d_tc.ptr), C.byref(n)))
        d_vol = density_grid_resident(d_tp, n.value, 512, 1.0, f64=False)
        (d_v, d_f), (nv, nf) = dev.isosurface(d_vol, (512, 512, 512), 0.1, 512, download=False)
        free((d_tp, d_tc, d_vol))
        return d_v, d_f, nv, nf

    for name, make in (("stored Taj, stride-1 mesh", taj_mesh), ("512^3 isosurface of the Taj density volume, level 0.1", iso_mesh)):
        d_v, d_f, nv, nf = make()
        F = d_f.download((nf, 3), np.int32)
        if orient:
            r = {"op": "ORIENT", "name": f"mesh_orientation: {name}", "nverts": int(nv), "nfaces": int(nf), "records": 3 * int(nf), "reps": reps}
            swapped = F.copy()
            k = np.random.default_rng(1).random(nf) < 0.5
            swapped[k] = swapped[k][:, [0, 2, 1]]
            d_s = dev.from_numpy(swapped)

            def run(d_faces, d_verts, sign, out_faces=False):
                *bufs, t = ori.mesh_orientation_resident(d_faces, nf, nv, d_verts, sign, out_faces=out_faces)
                free(bufs)
                return t
            r["orientation_ms"] = round(best(lambda: run(d_f, None, None)), 4)
            r["orientation_volumes_ms"] = round(best(lambda: run(d_f, d_v, None)), 4)
            r["orientation_sign_rule_ms"] = round(best(lambda: run(d_f, d_v, "negative")), 4)
            r["orient_mesh_half_swapped_ms"] = round(best(lambda: run(d_s, d_v, "negative", True)), 4)
            r["totals"] = run(d_f, d_v, "negative")
            r["totals_half_swapped"] = run(d_s, d_v, "negative", True)

            def components():
                *bufs, t = mcp.mesh_components_resident(d_f, nf, nv, None, "edge")
                free(bufs)
            r["yardstick_components_edge_ms"] = round(best(components), 4)
            for key in ("orientation_ms", "orientation_volumes_ms", "orientation_sign_rule_ms", "orient_mesh_half_swapped_ms"):
                r[key.replace("_ms", "_over_components_edge")] = round(r[key] / r["yardstick_components_edge_ms"], 3)
            print(json.dumps(r), flush=True)
            res.append(r)
            d_s.free()
        if weld:
            V = d_v.download((nv, 3), np.float32)
            soup = V[F].reshape(-1, 3)
            SF = np.arange(3 * nf, dtype=np.int32).reshape(nf, 3)
            d_sf = dev.from_numpy(SF)
            r = {"op": "WELD", "name": f"weld_vertices of the soup: {name}", "soup_vertices": 3 * int(nf), "nfaces": int(nf), "reps": reps}
            for f64 in (False, True):
                host = soup.astype(np.float64) if f64 else soup
                d_sv = dev.from_numpy(host)
                d_copy = dev.DeviceBuffer(host.nbytes)
                tag = "float64" if f64 else "float32"

                def run():
                    *bufs, m = wl.weld_vertices_resident(d_sv, 3 * nf, d_sf, nf, verts_f64=f64)
                    free(bufs)
                    return m
                r[f"weld_{tag}_ms"] = round(best(run), 4)
                r[f"classes_{tag}"] = run()
                r[f"yardstick_copy_{tag}_ms"] = round(best(lambda: L.check(lib.pb3d_d2d(L.ctx(), C.c_void_p(d_copy.ptr), C.c_void_p(d_sv.ptr), host.nbytes))), 4)
                r[f"weld_{tag}_over_copy"] = round(r[f"weld_{tag}_ms"] / r[f"yardstick_copy_{tag}_ms"], 1)
                free((d_sv, d_copy))
            r["yardstick_adjacency_ms"] = round(best(lambda: free(smo.mesh_vertex_adjacency_resident(d_f, nv, nf)[:4])), 4)
            for tag in ("float32", "float64"):
                r[f"weld_{tag}_over_adjacency"] = round(r[f"weld_{tag}_ms"] / r["yardstick_adjacency_ms"], 3)
            r["classes_equal_vertices_named"] = bool(r["classes_float32"] == mcp.mesh_topology_resident(d_f, nf, nv)["vertices"])
            print(json.dumps(r), flush=True)
            res.append(r)
            d_sf.free()
        free((d_v, d_f))
    d_g.free()


def overlays(reps, res):
    """overlays, notebook 2's projection-IoU overlays (csrc/overlay.hip) on the stored Akbar grid and, when the fixture is present,
    Itimad's deformed 512 x 381 x 512 grid, under the final front camera and the ten colours of PART_COLORS: the resident sweep
    (pb3d_grid_hit_bits_resident) and one compose launch per mode (device events), projection_overlays through the NumPy API and with a
    resident DeviceGrid, and beside them the existing projection_iou_by_part on the same grid and camera (host wall clock, median and
    min / max of reps after one warm-up call: upload, presence, sweep, compose and downloads included)."""
    from pb3d import camera_estimation as ce
    from pb3d import eval_helpers_intra as ev
    lib, L = pb3d._lib.load(), pb3d._lib
    g = os.path.join(ROOT, "tests", "golden")
    PC = pb3d.PART_COLORS
    cols = list(PC.values())
    tab = np.ascontiguousarray(np.array(cols, np.uint8))
    bg = np.array(PC["background"], np.uint8)

    def wall(key, fn):
        fn()
        t = []
        for _ in range(max(3, reps)):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        r[key] = round(1e3 * float(np.median(t)), 3)
        r["wall_min_max_ms"][key] = [round(1e3 * min(t), 3), round(1e3 * max(t), 3)]

    for mon, path in (("Akbar", "stored_Akbar_voxel_grid.npz"), ("Itimad deformed", "stored_Itimad_deformed_voxel_grid.npz")):
        if not os.path.exists(os.path.join(g, path)):
            continue
        grid = ev.load_voxel_grid(os.path.join(g, path))
        name = mon.split()[0]
        cam = ev.load_camera_json(os.path.join(g, f"stored_{name}_camera_params_final.json"), "front")
        image = np.ascontiguousarray(ev.resize_mask_to_voxel_grid(ev.load_mask(os.path.join(g, f"data_{name}_front_mask.png")), grid)[:, :, :3])
        H, W = image.shape[:2]
        d_g = dev.from_numpy(grid); d_img = dev.from_numpy(image)
        d_bits = dev.DeviceBuffer(H * W * 4); d_vis = dev.DeviceBuffer(len(cols) * H * W * 3); d_cnt = dev.DeviceBuffer(len(cols) * 16)
        sweep_ms = timeit(lambda: ce.hit_bits_resident(d_g, grid.shape, cols, cam, H, W, out=d_bits), reps)
        compose = {}
        for mode, m in ce.OVERLAY_MODES.items():
            fn = lambda: L.check(lib.pb3d_overlay_compose_resident(L.ctx(), C.c_void_p(d_bits.ptr), 1, C.c_void_p(d_img.ptr), H, W, L.p_u8(tab), len(cols),
                                                              L.p_u8(bg), None, m, C.c_void_p(d_vis.ptr), C.c_void_p(d_cnt.ptr)))
            compose[mode] = round(timeit(fn, reps), 4)
        resident = dev.DeviceGrid(d_g, grid.shape)
        r = {"op": "overlays", "name": f"projection overlays, {mon} {'x'.join(map(str, grid.shape[:3]))}, final front camera", "image": [H, W],
             "parts": len(cols), "sweep_resident_ms": round(sweep_ms, 4), "compose_resident_ms": compose, "wall_min_max_ms": {}}
        for mode in ce.OVERLAY_MODES:
            wall(f"{mode}_numpy_api_ms", lambda: ce.projection_overlays(grid, PC, image, cam, mode))
            wall(f"{mode}_device_grid_ms", lambda: ce.projection_overlays(resident, PC, image, cam, mode))
        wall("projection_iou_by_part_ms", lambda: ce.projection_iou_by_part(grid, PC, image, cam))
        for mode in ("part_on_whole", "whole_on_whole"):          # the two modes that return what projection_iou_by_part returns, plus images
            r[f"per_part_over_{mode}"] = round(r["projection_iou_by_part_ms"] / r[f"{mode}_numpy_api_ms"], 2)
        print(json.dumps(r), flush=True)
        res.append(r)
        for b in (d_g, d_img, d_bits, d_vis, d_cnt):
            b.free()


if __name__ == "__main__":
    main()
