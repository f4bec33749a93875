// The 3 x 3 symmetric eigen solve that csrc/surface.hip (the roughness of compute_surface_metrics) and csrc/normals.hip (point-cloud
// normals) share: one text, so the pair order, the threshold and the sweep limit that include/pb3d.h states are the same for both.
#pragma once
#include <cmath>

#include "pb3d_internal.h"

// Cyclic Jacobi on a symmetric 3 x 3 matrix: a -> diagonal, v (identity on entry) -> the rotations' product, columns = eigenvectors.
// Every index is a constant once the loops are unrolled.
__device__ __forceinline__ void jacobi3(double a[3][3], double v[3][3]) {
    for (int sweep = 0; sweep < 8; ++sweep) {
        bool any = false;
#pragma unroll
        for (int pi = 0; pi < 3; ++pi) {
            const int p = pi == 2 ? 1 : 0, q = pi == 0 ? 1 : 2, r = 3 - p - q;
            const double apq = a[p][q];
            if (apq == 0.0) continue;
            if (fabs(apq) > 0x1p-70 * sqrt(fabs(a[p][p] * a[q][q]))) {
                any = true;
                const double tau = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
                const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
                a[p][p] -= t * apq;
                a[q][q] += t * apq;
                const double arp = a[r][p], arq = a[r][q];
                a[r][p] = a[p][r] = c * arp - s * arq;
                a[r][q] = a[q][r] = s * arp + c * arq;
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    const double vp = v[x][p], vq = v[x][q];
                    v[x][p] = c * vp - s * vq;
                    v[x][q] = s * vp + c * vq;
                }
            }
            a[p][q] = a[q][p] = 0.0;
        }
        if (!any) break;
    }
}
