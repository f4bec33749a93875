// The cell grid and the ring walk of the exact searches: csrc/nn.hip (points in the cells) and csrc/meshdist.hip (triangles in the
// cells).  One text for both: what a cell holds -- the payload -- is a template parameter of ring_walk, and the search's Best decides
// what a run of a cell's entries means.
#pragma once
#include <cmath>

#include "pb3d_internal.h"

namespace {

constexpr double kPerCell = 2.0;             // points per cell the grid aims at
constexpr i64 kMaxCells = 1ll << 25;         // cap on the cell count (index memory: 12 bytes per cell)
constexpr double kMargin = 1e-12;            // relative margin of every pruning comparison (rounding errors are ~1e-15)

// ---- the cell grid ------------------------------------------------------------------------------------------------------------------
using Grid = pb3d_nn_grid;      // pb3d_internal.h (csrc/icp.hip keeps one between calls)

// cell of a coordinate: floor((v - lo) * inv) clamped to [0, n - 1] (NaN -> 0); points and queries use the same function
__device__ __forceinline__ int cell_of(const Grid& g, int a, double v) {
    const double t = fmin(fmax(floor((v - g.lo[a]) * g.inv[a]), 0.0), (double)(g.n[a] - 1));
    return (int)t;
}
__device__ __forceinline__ i64 cell_index(const Grid& g, int cx, int cy, int cz) { return ((i64)cx * g.n[1] + cy) * g.n[2] + cz; }

// Cell size for about kPerCell points per cell: h^d = (product of the d extents) / (n / kPerCell), computed in logs.  An axis whose
// extent is below h (zero extent included) gets one cell and leaves the product; the cell count is capped at kMaxCells.
inline Grid make_grid(const double b[6], i64 n) {
    Grid g;
    bool flat[3];
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = b[a];
        g.hi[a] = b[3 + a];
        flat[a] = !(b[3 + a] - b[a] > 0.0) || !std::isfinite(b[3 + a] - b[a]);
    }
    const double target = std::fmax(1.0, (double)n / kPerCell);
    double h = 0.0;
    for (int it = 0; it < 3; ++it) {
        int d = 0;
        double lsum = 0.0;
        for (int a = 0; a < 3; ++a)
            if (!flat[a]) { ++d; lsum += std::log(b[3 + a] - b[a]); }
        if (d == 0) break;
        h = std::exp((lsum - std::log(target)) / d);
        bool changed = false;
        for (int a = 0; a < 3; ++a)
            if (!flat[a] && b[3 + a] - b[a] < h) { flat[a] = true; changed = true; }
        if (!changed) break;
    }
    for (;;) {
        i64 total = 1;
        for (int a = 0; a < 3; ++a) {
            double na = flat[a] ? 1.0 : std::ceil((b[3 + a] - b[a]) / h);
            na = std::fmin(std::fmax(na, 1.0), (double)kMaxCells);
            g.n[a] = (int)na;
            total *= g.n[a];
            if (total > kMaxCells) total = kMaxCells + 1;
        }
        if (total <= kMaxCells) { g.ncells = total; break; }
        h *= 1.26;      // 2^(1/3): halves the cell count per step
    }
    for (int a = 0; a < 3; ++a) {
        const double ext = b[3 + a] - b[a];
        g.inv[a] = g.n[a] > 1 ? (double)g.n[a] / ext : 0.0;
        g.h[a] = g.n[a] > 1 ? ext / (double)g.n[a] : 0.0;
    }
    return g;
}

// The same box in fewer cells: every axis keeps at most floor(extent / (min_edge (1 + 1e-6))) of its cells, so a cell's edge exceeds
// min_edge and a search of radius min_edge ends with the ring next to the query's cell (27 cells).  Never more cells than g has.
inline void coarsen_grid(Grid& g, double min_edge) {
    g.ncells = 1;
    for (int a = 0; a < 3; ++a) {
        const double ext = g.hi[a] - g.lo[a];
        if (g.n[a] > 1) {
            const double na = std::floor(ext / (min_edge * (1.0 + 1e-6)));
            if (!(na >= (double)g.n[a])) g.n[a] = na >= 1.0 ? (int)na : 1;      // (a NaN quotient: one cell)
        }
        g.inv[a] = g.n[a] > 1 ? (double)g.n[a] / ext : 0.0;
        g.h[a] = g.n[a] > 1 ? ext / (double)g.n[a] : 0.0;
        g.ncells *= g.n[a];
    }
}

// Lower bound (margin applied) of |v - s| over s in the slab of cells [c0, c1] of axis a: the first and last cells reach the box's
// exact faces, the others end at lo + c h.  tol: the query's margin on this axis.
__device__ __forceinline__ double slab_gap(const Grid& g, int a, int c0, int c1, double v, double tol) {
    const double s0 = c0 == 0 ? g.lo[a] : g.lo[a] + (double)c0 * g.h[a];
    const double s1 = c1 == g.n[a] - 1 ? g.hi[a] : g.lo[a] + (double)(c1 + 1) * g.h[a];
    const double d = fmax(s0 - v, v - s1) - tol;
    return d > 0.0 ? d : 0.0;
}

// true when a lower bound lb (squared) proves that nothing there beats best (squared, as computed)
__device__ __forceinline__ bool beyond(double lb, double best) { return lb * (1.0 - kMargin) > best; }

// ---- the ring walk: one query against the index, for every search ----------------------------------------------------------------
// Best is the search's "best so far" and supplies two things: bound(), the pruning bound (the k-th best squared distance, as
// computed), and visit(pts, s, e, qv), which takes the run [s, e) of the cell-sorted arrays.  A column's runs (at most two) are decided
// first and then visited by ONE loop: a visit at each of the three places a run is chosen would inline KBest's insertion three
// times and take k_knn_query<8> and <20> to 256 registers.  The second z-end cell of a column is therefore tested against a bound
// that the first has not tightened yet; pruning only ever skips cells, so no result depends on it.
// Payload: the cell-sorted arrays themselves (csrc/nn.hip: Sorted; csrc/meshdist.hip: Faces), handed through to visit.
template <class Payload, class Best>
__device__ __forceinline__ void ring_walk(const Grid& g, const i64* __restrict__ start, const Payload& pts, const double (&qv)[3],
                                          Best& best) {
    int c[3];
    double tol[3], out2[3];     // per axis: margin, squared distance of the query to the box's extent on that axis
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c[a] = cell_of(g, a, qv[a]);
        tol[a] = 1e-12 * (fabs(g.lo[a]) + fabs(g.hi[a]) + fabs(qv[a]));
        const double o = fmax(fmax(g.lo[a] - qv[a], qv[a] - g.hi[a]) - tol[a], 0.0);
        out2[a] = o * o;
    }
    const int rmax = max(max(g.n[0], g.n[1]), g.n[2]);
    for (int r = 0; r <= rmax; ++r) {
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.n[0] - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.n[1] - 1);
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.n[2] - 1);
        for (int i = x0; i <= x1; ++i) {
            const double gx = slab_gap(g, 0, i, i, qv[0], tol[0]);
            const double gx2 = gx * gx;
            if (beyond(gx2, best.bound())) continue;
            const bool xe = i == c[0] - r || i == c[0] + r;
            for (int j = y0; j <= y1; ++j) {
                const double gy = slab_gap(g, 1, j, j, qv[1], tol[1]);
                const double gxy = gx2 + gy * gy;
                if (beyond(gxy, best.bound())) continue;
                const i64 row = cell_index(g, i, j, 0);
                i64 s0 = 0, e0 = 0, s1 = 0, e1 = 0;
                const auto z_run = [&](int za, int zb, i64* s, i64* e) {     // the cells [za, zb] of this column, unless pruned
                    const double gz = slab_gap(g, 2, za, zb, qv[2], tol[2]);
                    if (!beyond(gxy + gz * gz, best.bound())) { *s = start[row + za]; *e = start[row + zb + 1]; }
                };
                if (xe || j == c[1] - r || j == c[1] + r) {         // the whole z-run of the ring's face
                    z_run(z0, z1, &s0, &e0);
                } else {                                            // inside the ring's (x, y) box: its two z-end cells only
                    if (c[2] - r >= 0) z_run(c[2] - r, c[2] - r, &s0, &e0);
                    if (r > 0 && c[2] + r < g.n[2]) z_run(c[2] + r, c[2] + r, &s1, &e1);
                }
#pragma nounroll
                for (int t = 0; t < 2; ++t) best.visit(pts, t ? s1 : s0, t ? e1 : e0, qv);
            }
        }
        // lower bound over the cells not yet visited: per face of the visited box with cells beyond it, the gap to that face plus the
        // query's distance to the grid box along the other two axes
        const int lo_[3] = {x0, y0, z0}, hi_[3] = {x1, y1, z1};
        double lb = INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double rest = out2[(a + 1) % 3] + out2[(a + 2) % 3];
            if (hi_[a] < g.n[a] - 1) {
                const double gap = fmax(g.lo[a] + (double)(hi_[a] + 1) * g.h[a] - qv[a] - tol[a], 0.0);
                lb = fmin(lb, gap * gap + rest);
            }
            if (lo_[a] > 0) {
                const double gap = fmax(qv[a] - (g.lo[a] + (double)lo_[a] * g.h[a]) - tol[a], 0.0);
                lb = fmin(lb, gap * gap + rest);
            }
        }
        if (lb == INFINITY || beyond(lb, best.bound())) break;
    }
}

}  // namespace
