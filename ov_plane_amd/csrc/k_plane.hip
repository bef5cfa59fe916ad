// The on-plane feature kernel of the plane loop (update/UpdaterMSCKF.cpp:411-649; the loop's other kernels: k_plane2.hip, k_chol2.hip).
//
// Per on-plane MSCKF feature: get_feature_jacobian_full with the point-on-plane rows (update/UpdaterHelper.cpp:448-512) and
// UpdaterPlane::nullspace_project_inplace (update/UpdaterPlane.cpp:483-517).
// Facts used (verified numerically):
//   * the m identical constraint rows of a feature (:503-511) are one row scaled by sqrt(m) as far as any Gram
//     product is concerned;
//   * H_cp lies in range(H_x) (gauge freedom), so the truncation after compression loses no information on
//     (x, cp): the retained system has exactly the Gram pair of the untruncated one;
//   * there is no per-feature gate for plane features - only the plane-level one.
// So the kernel only emits sparse rows, projector rows G = Q1^T [H_x | H_cp | r] and the constraint-row moments; K2's kernels and
// k_plane_assemble2 reduce them.
#include "ovp_feat_model.h"
#include "k_tile_body.h"
#include <utility>

namespace ovp {

typedef double double4_t __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// K1p: one wave per on-plane feature. lanes 0..2m-1 bearing rows; the merged constraint row is wave-uniform (an extra term of the sums).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_plane_feat(const FeatParams p, const PlaneParams pp) {
  const int fl = blockIdx.x;                 // local feature index within this plane
  const int f = pp.feat_list[fl];            // index into the feature batch
  const int lane = threadIdx.x;
  const int m = p.n_meas[f];
  const int n = 2 * m;
  const int a = lane >> 1, r = lane & 1;
  const bool valid = lane < n;
  const int* cidx = p.clone_idx + (size_t)f * p.max_meas;
  const int ci = cidx[valid ? a : 0];
  const int ida = p.clone_id[ci];
  __shared__ __attribute__((aligned(16))) double Gst[3 * OVP_LDG_CAP];

  double jrow[6], crow[14], hf[3], res;
  build_bearing_row(p, f, a, r, valid, ci, jrow, crow, hf, res);

  // constraint row (update/UpdaterHelper.cpp:450-497), merged: m identical rows == one row scaled by sqrt(m).  Its entries
  // depend on the feature and the plane only, not on an observation: every lane computes them (wave-uniform) and the row
  // takes part in the sums below as an extra term instead of occupying lane 2m - a track of 32 observations (64 bearing rows)
  // keeps its constraint (round 4; until then 2m + 1 rows had to fit the wavefront: OVP_E_CAPACITY above 31 observations,
  // update/UpdaterMSCKF.cpp:413-649 has no such limit)
  double hcp[3], hfc[3], resc;
  {
    const double* cp = pp.cp + 3 * pp.plane;
    const double* cpf = pp.in_state ? (pp.cp_fej + 3 * pp.plane) : cp;  // UpdaterMSCKF.cpp:467-475
    const double pf0 = p.p_FinG[3 * f], pf1 = p.p_FinG[3 * f + 1], pf2 = p.p_FinG[3 * f + 2];
    const double sm = sqrt((double)m) * pp.white_c;
    double d = sqrt(cp[0] * cp[0] + cp[1] * cp[1] + cp[2] * cp[2]);
    double id = 1.0 / d;
    double n0 = cp[0] * id, n1 = cp[1] * id, n2 = cp[2] * id;
    resc = sm * (0.0 - (n0 * pf0 + n1 * pf1 + n2 * pf2 - d));
    if (p.do_fej) {
      d = sqrt(cpf[0] * cpf[0] + cpf[1] * cpf[1] + cpf[2] * cpf[2]);
      id = 1.0 / d;
      n0 = cpf[0] * id;
      n1 = cpf[1] * id;
      n2 = cpf[2] * id;
    }
    const double ndp = n0 * pf0 + n1 * pf1 + n2 * pf2;  // p_FinG_fej == p_FinG for MSCKF features
    const double s = sm * id;
    hcp[0] = s * (pf0 - ndp * n0 - d * n0);
    hcp[1] = s * (pf1 - ndp * n1 - d * n1);
    hcp[2] = s * (pf2 - ndp * n2 - d * n2);
    hfc[0] = sm * n0;
    hfc[1] = sm * n1;
    hfc[2] = sm * n2;
  }

  // Q1 by CholeskyQR2 on H_f (2m+1 rows)
  double q[3] = {hf[0], hf[1], hf[2]};
  double qc[3] = {hfc[0], hfc[1], hfc[2]};  // the constraint row's part of Q1 (wave-uniform)
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    double v[8];
    v[0] = q[0] * q[0];
    v[1] = q[0] * q[1];
    v[2] = q[0] * q[2];
    v[3] = q[1] * q[1];
    v[4] = q[1] * q[2];
    v[5] = q[2] * q[2];
    v[6] = 0.0;
    v[7] = 0.0;
    const double rsum = wave_transpose_reduce<8>(v);
    const double g00 = readlane_f64(rsum, reduce_owner_lane<8>(0)) + qc[0] * qc[0], g01 = readlane_f64(rsum, reduce_owner_lane<8>(1)) + qc[0] * qc[1];
    const double g02 = readlane_f64(rsum, reduce_owner_lane<8>(2)) + qc[0] * qc[2], g11 = readlane_f64(rsum, reduce_owner_lane<8>(3)) + qc[1] * qc[1];
    const double g12 = readlane_f64(rsum, reduce_owner_lane<8>(4)) + qc[1] * qc[2], g22 = readlane_f64(rsum, reduce_owner_lane<8>(5)) + qc[2] * qc[2];
    // R^T R = G with the reciprocals of the diagonal (v_rsq_f64 + two Newton steps each): a sqrt and five divisions per pass were
    // 3.2 K cycles of dependent div / sqrt sequences.  Q1 is orthonormal to rounding after the second pass either way.
    const double i00 = rsqrt_nr2(g00), r01 = g01 * i00, r02 = g02 * i00;
    const double i11 = rsqrt_nr2(g11 - r01 * r01), r12 = (g12 - r01 * r02) * i11;
    const double i22 = rsqrt_nr2(g22 - r02 * r02 - r12 * r12);
    const double a0 = q[0] * i00;
    const double a1 = (q[1] - a0 * r01) * i11;
    const double a2 = (q[2] - a0 * r02 - a1 * r12) * i22;
    q[0] = a0;
    q[1] = a1;
    q[2] = a2;
    const double c0 = qc[0] * i00;
    const double c1 = (qc[1] - c0 * r01) * i11;
    const double c2 = (qc[2] - c0 * r02 - c1 * r12) * i22;
    qc[0] = c0;
    qc[1] = c1;
    qc[2] = c2;
  }

  const int ldg = p.ldg;
  for (int idx = lane; idx < 3 * ldg; idx += 64) Gst[idx] = 0.0;
  __syncthreads();
  double gsq = 0.0;  // |g|^2
  {
    double v[64];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int k = 0; k < 14; ++k) v[t * 14 + k] = q[t] * crow[k];
#pragma unroll
    for (int t = 0; t < 3; ++t) v[42 + t] = q[t] * res;
    v[45] = res * res;
#pragma unroll
    for (int k = 46; k < 64; ++k) v[k] = 0.0;
    double rsum = wave_transpose_reduce<64>(v);
    // the constraint row's terms of Q1^T r (lanes 42..44) and of r^T r (lane 45); its calibration / clone entries are zero
    rsum += lane == 42 ? qc[0] * resc : (lane == 43 ? qc[1] * resc : (lane == 44 ? qc[2] * resc : (lane == 45 ? resc * resc : 0.0)));
    {
      // where this lane's sum goes: lanes 0..41 = (projector row t, calibration entry k), 42..44 = the residual column.  The column
      // is picked by a select chain over the table - a kernel-argument array indexed by a lane-dependent k is a waterfall loop
      const int t = lane < 42 ? lane / 14 : lane - 42, k = lane - 14 * t;
      int col = -1;
#pragma unroll
      for (int kk = 0; kk < 14; ++kk) col = (k == kk && ((p.calmask >> kk) & 1)) ? p.calcol[kk] : col;
      if (lane >= 42) col = lane < 45 ? p.n : -1;
      if (col >= 0) Gst[t * ldg + col] = rsum;
    }
    const double g0 = readlane_f64(rsum, 42), g1 = readlane_f64(rsum, 43), g2 = readlane_f64(rsum, 44);
    gsq = g0 * g0 + g1 * g1 + g2 * g2;
    const double rr = readlane_f64(rsum, 45);
    // constraint-row moments (already scaled by m): hh (6), h*res (3), projected residual energy
    const double h0 = hcp[0], h1 = hcp[1], h2 = hcp[2];
    const double rc = resc;
    if (lane == 0) {
      double* o = pp.cst + (size_t)fl * 10;
      o[0] = h0 * h0;
      o[1] = h0 * h1;
      o[2] = h0 * h2;
      o[3] = h1 * h1;
      o[4] = h1 * h2;
      o[5] = h2 * h2;
      o[6] = h0 * rc;
      o[7] = h1 * rc;
      o[8] = h2 * rc;
      o[9] = rr - gsq;
    }
    // plane columns of G: only the constraint lane has a non-zero H_cp row
    const double qc0 = qc[0], qc1 = qc[1], qc2 = qc[2];
    if (lane < 9) {
      const int t = lane / 3, k = lane - 3 * t;
      const double qt = t == 0 ? qc0 : (t == 1 ? qc1 : qc2);
      const double hk = k == 0 ? h0 : (k == 1 ? h1 : h2);
      const int col = pp.in_state ? (pp.plane_sid + k) : (p.n + 1 + k);
      Gst[t * ldg + col] = qt * hk;
    }
  }
  // clone columns
  {
    double cv[18];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int l = 0; l < 6; ++l) {
        const double v = q[t] * jrow[l];
        cv[6 * t + l] = v + shfl_xor_f64(v, 1);
      }
    if (valid && r == 0) {  // (one masked block: eighteen of them were eighteen EXEC round trips)
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int l = 0; l < 6; ++l) Gst[t * ldg + ida + l] = cv[6 * t + l];
    }
  }
  __syncthreads();
  {
    double* gout = p.G + (size_t)3 * fl * ldg;
    for (int idx = lane; idx < 3 * ldg; idx += 64) gout[idx] = Gst[idx];
  }
  // sparse bearing rows, grouped by clone slot, local feature index
  // clone slots this feature was seen from: every valid lane already holds its observation's slot (a rolled loop over cidx[]
  // was m dependent loads, ~6 us of a 12 us kernel)
  const unsigned long long seen = wave_or_u64(valid ? (1ull << ci) : 0ull);
  if (valid) {
    double* ro = p.rec + (((size_t)ci * pp.n_local + fl) * 2 + r) * OVP_REC;
#pragma unroll
    for (int l = 0; l < 6; ++l) ro[l] = jrow[l];
#pragma unroll
    for (int k = 0; k < 14; ++k) ro[6 + k] = crow[k];
    ro[20] = res;
  }
  for (int cc = 0; cc < p.n_clones; ++cc) {
    if (!((seen >> cc) & 1ull)) {
      double* ro = p.rec + (((size_t)cc * pp.n_local + fl) * 2) * OVP_REC;
      if (lane < 2 * OVP_REC) ro[lane] = 0.0;
    }
  }
}

}  // namespace ovp

extern "C" hipError_t ovp_launch_plane_feat(const ovp::FeatParams* p, const ovp::PlaneParams* pp, int n_local, hipStream_t stream) {
  if (n_local <= 0) return hipSuccess;
  hipLaunchKernelGGL(ovp::k_plane_feat, dim3(n_local), dim3(64), 0, stream, *p, *pp);
  return hipGetLastError();
}
