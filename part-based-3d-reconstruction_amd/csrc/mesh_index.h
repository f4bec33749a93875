// How the mesh kernels (csrc/surface.hip, meshdist.hip, smooth.hip) read a face list of int32 or int64 indices, and how their hosts
// turn the mesh's two run-time widths into template arguments.
#pragma once
#include "pb3d_internal.h"

template <bool I64>
__device__ __forceinline__ i64 load_index(const void* p, i64 e) {
    return I64 ? ((const i64*)p)[e] : (i64)((const int*)p)[e];
}
// a checked index in [-nv, nv) as NumPy reads it
__device__ __forceinline__ i64 wrap(i64 v, i64 nv) { return v < 0 ? v + nv : v; }

// fn(VF64, I64) with the mesh's vertex and index widths as compile-time constants
template <class Fn>
void with_mesh_types(int verts_f64, int faces_i64, Fn fn) {
    if (verts_f64 && faces_i64) fn(std::true_type{}, std::true_type{});
    else if (verts_f64) fn(std::true_type{}, std::false_type{});
    else if (faces_i64) fn(std::false_type{}, std::true_type{});
    else fn(std::false_type{}, std::false_type{});
}
