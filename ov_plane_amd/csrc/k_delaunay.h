// Launch prototype of the device Delaunay triangulation (k_delaunay.hip) and the layout of its result header.
#pragma once
#include <hip/hip_runtime.h>

// hdr: OVP_DL_HDR ints in front of the triangle list
//   [0] triangles written   [1] overflow flag (then [0] = 0 and no triangle is written)   [2] vertices (points whose flag bit 0 is set)
//   [3] most table slots in use at once, ghosts included   [4] largest cavity (triangles)
#define OVP_DL_HDR 16

extern "C" {
// n <= OVP_DET_MAX_POINTS points xy [2n] (f32, device); flag == nullptr: every point is a vertex, else the points whose flag
// bit 0 is set, compacted in point order; tris [3 * tri_cap] (device).  One workgroup.
hipError_t ovp_launch_delaunay(int n, const float* xy, const int* flag, int* hdr, int* tris, int tri_cap, hipStream_t stream);
}
