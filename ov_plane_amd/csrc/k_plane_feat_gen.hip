// General on-plane features in the plane loop (ovp_msckf_plane_update_general): observations of any camera, tracks of up to
// OVP_GEN_MAX_MEAS_DEV views - the on-plane features the wave-per-feature kernel (k_plane_feat, k_plane.hip) cannot carry.
// update/UpdaterHelper.cpp:335-440 (bearing rows over every camera), :448-512 (point-on-plane rows), update/UpdaterPlane.cpp:483-517
// (nullspace projection), update/UpdaterMSCKF.cpp:411-649 (the loop that stacks them).
//
// k_plane_feat_gen: one workgroup of 256 threads per feature.
//   rows      thread i < 2m builds bearing row i with ovp_feat_model.h (the camera of the observation picks the calibration block);
//             thread 2m builds the point-on-plane row with build_plane_row - the reference's m equal rows merged into one scaled
//             by sqrt(m) (NOTES 3b) - with the plane's three columns (state columns of an in-state plane, n + 1 .. n + 3 otherwise).
//   projector U = orthonormal basis of range(H_f) over the 2m + 1 rows (modified Gram-Schmidt, twice, in wave 0); Pi = I - U U^T, as
//             k_feat_gen does: any orthonormal basis N of the complement gives the same (N^T H)^T (N^T H) = H^T Pi H.
//   rows out  Hp = Pi [H_x | r | H_cp] over the n + 4 columns of the plane's extended pair, staged in global memory (129 rows x up
//             to 292 columns do not fit LDS beside the rows), with a mark per column the feature touches.
// k_plane_gen_pair: one workgroup per 16 x 16 tile of the extended pair, one thread per entry, the features added in list order:
// no atomics, the same bits from run to run.  The sum goes out as one more split of the G^T G partials k_plane_assemble2 sums
// (negated: that kernel subtracts the partials from the structured Gram), the projected residual energy as one more
// constraint-moment record - so the Schur complement of an out-of-state plane, the normalised Gram and the gate statistic see batch
// features and general features as one system, and k_plane_assemble2 itself is unchanged.
// k_plane_gen_commit: behind k_chol2 - the accepted plane's correction applied to the camera tables of ovp_cameras_upload
// (k_chol2 commits the clone tables, camera 0's table of ovp_state_upload and the planes).
#include "ovplane_hip.h"
#include "ovp_dev.h"
#include "ovp_feat_model.h"
#include "ovp_kernels.h"
#include "k_plane_gen.h"

namespace ovp {

static constexpr int PG_THREADS = 256;
static constexpr int PG_NZ = 20;  // non-zero state columns of a bearing row: clone (6) + camera (14)

struct PlaneGenLds {
  double J[PG_ROWS][PG_NZ];  // row i: clone block (6) | extrinsics (6) | intrinsics (8), whitened; the plane row's is zero
  double hf[PG_ROWS][3];
  double r[PG_ROWS];
  double U[PG_ROWS][3];
  double hc[3];                            // H_c_plane of the merged point-on-plane row
  int col[OVP_GEN_MAX_MEAS_DEV][PG_NZ];    // state column of every non-zero of observation a, -1 = not estimated
};

__global__ __launch_bounds__(PG_THREADS) void k_plane_feat_gen(const PlaneGenParams g) {
  __shared__ PlaneGenLds s;
  const int fl = blockIdx.x, tid = threadIdx.x;
  const int f = g.list[fl];
  const int m = g.n_meas[f], nb = 2 * m, nr = nb + 1;
  const int n = g.n, ncols = n + 4;
  if (m < 2 || m > OVP_GEN_MAX_MEAS_DEV) return;  // (the host lists no such feature)
  double* blk = g.hp + (size_t)fl * g.hp_stride;
  int* mark = g.mark + (size_t)fl * g.mark_stride;
  for (int e = tid; e < ncols; e += PG_THREADS) mark[e] = 0;
  for (int e = tid; e < nr * ncols; e += PG_THREADS) blk[e] = 0.0;
  const size_t ob = (size_t)f * g.max_meas;
  if (tid < nb) {  // ---- bearing rows (UpdaterHelper.cpp:335-440) ----
    const int a = tid >> 1, rr = tid & 1;
    const int ci = g.clone_idx[ob + a], cam = g.cam_idx[ob + a];
    FeatParams p = g.fp;
    p.cal = g.cam_cal + 20 * cam;
    p.fisheye = g.cam_fisheye[cam];
    p.uv = g.uv;
    p.max_meas = g.max_meas;
    p.p_FinG = g.p_FinG;
    double jrow[6], crow[14], h[3], res;
    build_bearing_row<false>(p, f, a, rr, true, ci, jrow, crow, h, res);
#pragma unroll
    for (int k = 0; k < 6; ++k) s.J[tid][k] = jrow[k];
#pragma unroll
    for (int k = 0; k < 14; ++k) s.J[tid][6 + k] = crow[k];
    s.hf[tid][0] = h[0];
    s.hf[tid][1] = h[1];
    s.hf[tid][2] = h[2];
    s.r[tid] = res;
    if (rr == 0) {
      const int cid = g.fp.clone_id[ci];
#pragma unroll
      for (int k = 0; k < 6; ++k) s.col[a][k] = cid + k;
#pragma unroll
      for (int k = 0; k < 14; ++k) s.col[a][6 + k] = ((g.fp.calmask >> k) & 1) ? g.cc.col[cam][k] : -1;
    }
  } else if (tid == nb) {  // ---- point-on-plane row (UpdaterHelper.cpp:448-512), m equal rows as one ----
    const double* cp = g.cp + 3 * g.plane;
    const double* cf = g.in_state ? g.cp_fej + 3 * g.plane : cp;  // UpdaterMSCKF.cpp:467-475
    const double* pf = g.p_FinG + 3 * f;                          // fej == value for MSCKF features (:499-500)
    double h[3], hc[3], res;
    build_plane_row(pf, pf, cp, cf, g.fp.do_fej, g.white_c, h, hc, res);
    const double sm = sqrt((double)m);
#pragma unroll
    for (int k = 0; k < PG_NZ; ++k) s.J[nb][k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      s.hf[nb][k] = sm * h[k];
      s.hc[k] = sm * hc[k];
    }
    s.r[nb] = sm * res;
  }
  __syncthreads();
  // ---- U: orthonormal basis of range(H_f), wave 0, lane l holds rows l, l + 64 and l + 128 ----
  if (tid < 64) {
    double u[3][3];
#pragma unroll
    for (int h = 0; h < 3; ++h)
#pragma unroll
      for (int c = 0; c < 3; ++c) u[h][c] = (tid + 64 * h < nr) ? s.hf[tid + 64 * h][c] : 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int pass = 0; pass < 2; ++pass)
#pragma unroll
        for (int d = 0; d < c; ++d) {
          const double dot = wave_sum(u[0][d] * u[0][c] + u[1][d] * u[1][c] + u[2][d] * u[2][c]);
#pragma unroll
          for (int h = 0; h < 3; ++h) u[h][c] -= dot * u[h][d];
        }
      const double nrm = sqrt(wave_sum(u[0][c] * u[0][c] + u[1][c] * u[1][c] + u[2][c] * u[2][c]));
      const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;  // (a direction H_f does not span is not projected out)
#pragma unroll
      for (int h = 0; h < 3; ++h) u[h][c] *= inv;
    }
#pragma unroll
    for (int h = 0; h < 3; ++h)
      if (tid + 64 * h < nr)
#pragma unroll
        for (int c = 0; c < 3; ++c) s.U[tid + 64 * h][c] = u[h][c];
  }
  // ---- [H_x | r | H_cp] into the staged block (zeroed above, in front of the barrier) ----
  if (tid < nb) {
    const int a = tid >> 1;
    for (int k = 0; k < PG_NZ; ++k) {
      const int ck = s.col[a][k];
      if (ck < 0 || ck >= n) continue;
      blk[(size_t)ck * nr + tid] = s.J[tid][k];
      mark[ck] = 1;
    }
    blk[(size_t)n * nr + tid] = s.r[tid];
  } else if (tid == nb) {
    const int pc = g.in_state ? g.plane_sid : n + 1;
    if (pc >= 0 && pc + 3 <= ncols)
      for (int k = 0; k < 3; ++k) {
        blk[(size_t)(pc + k) * nr + nb] = s.hc[k];
        mark[pc + k] = 1;
      }
    blk[(size_t)n * nr + nb] = s.r[nb];
    mark[n] = 1;
  }
  __syncthreads();
  // ---- Hp = Pi H, column by column ----
  for (int cc = tid; cc < ncols; cc += PG_THREADS) {
    if (!mark[cc]) continue;
    double* colp = blk + (size_t)cc * nr;
    double t[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < nr; ++i) {
      const double h = colp[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) t[c] += s.U[i][c] * h;
    }
    for (int i = 0; i < nr; ++i) colp[i] -= s.U[i][0] * t[0] + s.U[i][1] * t[1] + s.U[i][2] * t[2];
  }
}

// entry (I, J) of the plane's extended pair: sum over the plane's general features, in list order, of Hp_f[:, I] . Hp_f[:, J]
__global__ __launch_bounds__(256) void k_plane_gen_pair(const PlaneGenParams g) {
  const int tile = blockIdx.x, e = threadIdx.x;
  int ti = (int)((sqrt(8.0 * tile + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > tile) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
  const int tj = tile - ti * (ti + 1) / 2;
  const int I = 16 * ti + (e >> 4), J = 16 * tj + (e & 15);
  const int n = g.n, ncols = n + 4;
  double acc = 0.0;
  if (I < ncols && J < ncols)
    for (int fl = 0; fl < g.n_local; ++fl) {
      const int* mark = g.mark + (size_t)fl * g.mark_stride;
      if (!mark[I] || !mark[J]) continue;
      const int nr = 2 * g.n_meas[g.list[fl]] + 1;
      const double* cu = g.hp + (size_t)fl * g.hp_stride + (size_t)I * nr;
      const double* cv = g.hp + (size_t)fl * g.hp_stride + (size_t)J * nr;
      for (int i = 0; i < nr; ++i) acc += cu[i] * cv[i];
    }
  g.part_split[(size_t)tile * 256 + e] = -acc;
  if (I == n && J == n) {  // constraint-moment record: the plane moments travel in the split, the energy here
    for (int k = 0; k < 9; ++k) g.cst_rec[k] = 0.0;
    g.cst_rec[9] = acc;
  }
}

// ext JPLQuat::update on a rotation matrix: R <- R(dq) R, dq = quatnorm([dth / 2, 1])
__device__ __forceinline__ void pg_rot_update(double* R, const double* dth) {
  double qx = 0.5 * dth[0], qy = 0.5 * dth[1], qz = 0.5 * dth[2], qw = 1.0;
  const double nn = 1.0 / sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
  qx *= nn;
  qy *= nn;
  qz *= nn;
  qw *= nn;
  const double a = 2.0 * qw * qw - 1.0;
  const double D[9] = {a + 2.0 * qx * qx,  2.0 * qw * qz + 2.0 * qx * qy,  -2.0 * qw * qy + 2.0 * qx * qz,
                       -2.0 * qw * qz + 2.0 * qy * qx, a + 2.0 * qy * qy, 2.0 * qw * qx + 2.0 * qy * qz,
                       2.0 * qw * qy + 2.0 * qz * qx,  -2.0 * qw * qx + 2.0 * qz * qy, a + 2.0 * qz * qz};
  double O[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) O[3 * i + j] = D[3 * i] * R[j] + D[3 * i + 1] * R[3 + j] + D[3 * i + 2] * R[6 + j];
  for (int i = 0; i < 9; ++i) R[i] = O[i];
}

// Type::update of every camera of ovp_cameras_upload after an accepted plane (state/StateHelper.cpp:188-194): lane = camera
__global__ __launch_bounds__(64) void k_plane_gen_commit(const double* __restrict__ res, const double* __restrict__ dx,
                                                         double* __restrict__ cam_cal, int n_cams, const PlaneGenCols cc,
                                                         unsigned calmask) {
  if (!(res[1] > 0.5)) return;
  const int c = threadIdx.x;
  if (c >= n_cams || c >= OVP_GEN_MAX_CAMS) return;
  double tc[20];
  for (int k = 0; k < 20; ++k) tc[k] = cam_cal[20 * c + k];
  if ((calmask & 0x3Fu) && cc.col[c][0] >= 0) {
    const double dth[3] = {dx[cc.col[c][0]], dx[cc.col[c][1]], dx[cc.col[c][2]]};
    pg_rot_update(tc, dth);
    for (int k = 0; k < 3; ++k) tc[9 + k] += dx[cc.col[c][3 + k]];
  }
  if ((calmask & (0xFFu << 6)) && cc.col[c][6] >= 0)
    for (int k = 0; k < 8; ++k) tc[12 + k] += dx[cc.col[c][6 + k]];
  for (int k = 0; k < 20; ++k) cam_cal[20 * c + k] = tc[k];
}

}  // namespace ovp

extern "C" hipError_t ovp_launch_plane_feat_gen(const ovp::PlaneGenParams* g, hipStream_t stream) {
  if (g->n_local <= 0) return hipSuccess;
  hipLaunchKernelGGL(ovp::k_plane_feat_gen, dim3(g->n_local), dim3(ovp::PG_THREADS), 0, stream, *g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int nt = (g->n + 4 + 15) / 16;
  hipLaunchKernelGGL(ovp::k_plane_gen_pair, dim3(nt * (nt + 1) / 2), dim3(256), 0, stream, *g);
  return hipGetLastError();
}

extern "C" hipError_t ovp_launch_plane_gen_commit(const double* res, const double* dx, double* cam_cal, int n_cams,
                                                  const ovp::PlaneGenCols* cc, unsigned calmask, hipStream_t stream) {
  hipLaunchKernelGGL(ovp::k_plane_gen_commit, dim3(1), dim3(64), 0, stream, res, dx, cam_cal, n_cams, *cc, calmask);
  return hipGetLastError();
}
