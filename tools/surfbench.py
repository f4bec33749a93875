"""Timing of the mesh regularity metrics (csrc/surface.hip, pb3d_knn_dev of csrc/nn.hip) on the meshes of the stored Taj grid at
strides 1 and 2: k-NN (k = 20) on the vertices themselves, vertex normals, the per-vertex metrics given both, and the whole call,
resident (device events) and through the NumPy API (wall clock, uploads and the 24 B per vertex of download included).
python tools/surfbench.py [--reps 5] [--out profiles/surface_opbench.jsonl]; one JSON line per mesh.  Under
`rocprofv3 --kernel-trace --stats -- python tools/surfbench.py --reps 1` the same run gives the per-kernel table.
The reference's wall time for scale is measured on a CPU by tools/gen_golden_surface.py (a few thousand vertices per mesh)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "part-based-3d-reconstruction_amd"))
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

import pb3d  # noqa: E402
from pb3d import device as dev  # noqa: E402
from pb3d import eval_helpers as eh  # noqa: E402

K = 20


def timeit(fn, reps, warm=1):
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib, ctx = pb3d._lib.load(), pb3d._lib.ctx()
    g = np.load(os.path.join(ROOT, "tests", "golden", "stored_Taj_voxel_grid.npz"))["voxel_grid"]
    d_g = dev.from_numpy(g)
    rows = []
    for s in (1, 2):
        (dv, df, dn, dc), (nv, nf) = dev.meshify(d_g, g.shape, stride=s, download=False)
        d_n = eh.vertex_normals_resident(dv, nv, df, nf)
        _, d_idx = eh.knn_resident(dv, nv, dv, nv, K, False, False, dist=False)
        d_out = dev.DeviceBuffer(nv * 24)

        def run_knn():
            eh.knn_resident(dv, nv, dv, nv, K, False, False, dist=False)[1].free()

        def run_metrics():
            pb3d._lib.check(lib.pb3d_surface_metrics_dev(ctx, C.c_void_p(dv.ptr), C.c_void_p(d_n.ptr), 0, nv, C.c_void_p(d_idx.ptr), K,
                                                         d_out.at(0), d_out.at(nv * 8), d_out.at(nv * 16)))

        r = {"op": "SURF", "name": "compute_surface_metrics, mesh of the stored Taj grid", "stride": s, "nverts": int(nv), "nfaces": int(nf),
             "k": K, "knn_ms": round(timeit(run_knn, a.reps), 3),
             "vertex_normals_ms": round(timeit(lambda: eh.vertex_normals_resident(dv, nv, df, nf, out=d_n), a.reps), 3),
             "metrics_ms": round(timeit(run_metrics, a.reps), 3),
             "resident_whole_ms": round(timeit(lambda: eh.surface_metrics_resident(dv, nv, df, nf, K).free(), a.reps), 3)}
        v, f = dv.download((nv, 3), np.float32), df.download((nf, 3), np.int32)
        for b in (dv, df, dn, dc, d_n, d_idx, d_out):
            b.free()
        res = pb3d.compute_surface_metrics(v, f, K)
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = pb3d.compute_surface_metrics(v, f, K)
            wall.append(time.perf_counter() - t0)
        r["numpy_api_ms"] = round(1e3 * min(wall), 3)
        r["result"] = {key: float(val) for key, val in res.items()}
        print(json.dumps(r, ensure_ascii=False), flush=True)
        rows.append(r)
    d_g.free()
    if a.out:
        with open(a.out, "w", encoding="utf-8") as fh:
            for r in rows:
                fh.write(json.dumps(r, ensure_ascii=False) + "\n")


if __name__ == "__main__":
    main()
