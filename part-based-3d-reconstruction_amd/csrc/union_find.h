// The lock-free min-root union-find of csrc/cluster.hip (core points) and csrc/meshcomp.hip (faces or vertices): one copy.
#pragma once
#include "pb3d_internal.h"

__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- the forest: parent[v] == v at a root, parent[v] < v otherwise ------------------------------------------------------------------
// The union of csrc/ccl.hip on plain indices: both root searches advance together with path halving (every store is an ancestor), the
// larger root is hung under the smaller with atomicMin, and a root that was re-parented meanwhile (old != a) sends the union on from
// its new parent.  Every link points to a smaller position inside the same component, so whatever the interleaving the one root a
// component ends with is its smallest position.
__device__ __forceinline__ void uf_union(int* parent, int a, int b) {
    while (true) {
        int pa = ld(&parent[a]), pb = ld(&parent[b]);
        while (pa != a || pb != b) {
            const int ga = pa != a ? ld(&parent[pa]) : pa;
            const int gb = pb != b ? ld(&parent[pb]) : pb;
            if (pa != a) { if (ga != pa) st(&parent[a], ga); a = pa; pa = ga; }
            if (pb != b) { if (gb != pb) st(&parent[b], gb); b = pb; pb = gb; }
        }
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}
