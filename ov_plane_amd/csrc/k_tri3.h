// The 3 x 3 pieces of a linear triangulation system that its kernels share (device only): k_det_triangulate (k_plane_detect.hip)
// and k_active_tracks (k_active_tracks.hip).  A is symmetric and stored as its upper triangle (00 01 02 11 12 22).  Both functions
// are inlined into their callers, so a kernel that used to carry this text compiles to the code it had.
#pragma once
#include <hip/hip_runtime.h>

// one Jacobi rotation of the symmetric 3x3 (p, q the rotated pair, r the third index)
#define OVP_TRI3_JACOBI(app, aqq, apq, arp, arq)                                  \
  if (apq != 0.0) {                                                               \
    const double th = (aqq - app) / (2.0 * apq);                                  \
    const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0)); \
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;                          \
    app -= t * apq;                                                               \
    aqq += t * apq;                                                               \
    apq = 0.0;                                                                    \
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;                  \
    arp = rp;                                                                     \
    arq = rq;                                                                     \
  }

// A x = b by elimination with row pivoting
__device__ __forceinline__ void ovp_tri3_solve(const double A[6], const double b[3], double q[3]) {
  double M[3][4] = {{A[0], A[1], A[2], b[0]}, {A[1], A[3], A[4], b[1]}, {A[2], A[4], A[5], b[2]}};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int r = c + 1; r < 3; ++r)
      if (fabs(M[r][c]) > fabs(M[c][c])) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double t = M[c][k];
          M[c][k] = M[r][k];
          M[r][k] = t;
        }
      }
#pragma unroll
    for (int r = c + 1; r < 3; ++r) {
      const double f = M[r][c] / M[c][c];
#pragma unroll
      for (int k = c; k < 4; ++k) M[r][k] -= f * M[c][k];
    }
  }
  q[2] = M[2][3] / M[2][2];
  q[1] = (M[1][3] - M[1][2] * q[2]) / M[1][1];
  q[0] = (M[0][3] - M[0][1] * q[1] - M[0][2] * q[2]) / M[0][0];
}

// largest over smallest singular value: the singular values of the symmetric A are the magnitudes of its eigenvalues (cyclic Jacobi)
__device__ __forceinline__ double ovp_tri3_cond(const double A[6]) {
  double a00 = A[0], a01 = A[1], a02 = A[2], a11 = A[3], a12 = A[4], a22 = A[5];
  for (int sweep = 0; sweep < 8; ++sweep) {
    OVP_TRI3_JACOBI(a00, a11, a01, a02, a12)
    OVP_TRI3_JACOBI(a00, a22, a02, a01, a12)
    OVP_TRI3_JACOBI(a11, a22, a12, a01, a02)
  }
  const double e0 = fabs(a00), e1 = fabs(a11), e2 = fabs(a22);
  return fmax(e0, fmax(e1, e2)) / fmin(e0, fmin(e1, e2));
}
