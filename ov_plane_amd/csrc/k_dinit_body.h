// Body of the delayed-initialisation row kernels (k_dinit.hip), included once per instance INSIDE the kernel function:
//   DI_GEN 0  k_dinit_rows(DinitParams dp)         every observation is camera 0's (DinitParams::cal), one calibration block
//   DI_GEN 1  k_dinit_rows_gen(DinitGenParams gp)  observation a by camera gp.cam_idx[cand][a], its tables from ovp_cameras_upload;
//             local columns [clone blocks of the distinct clones in first-seen order | estimated calibration columns of every
//             camera of the candidate, in camera order]; the commit applies the previous correction to camera 0's DinitParams::cal
//             AND to every camera of the general tables
//   DI_PL 1   k_dinit_rows_pl(DinitParams dp, DinitPlaneParams pp) / k_dinit_rows_gen_pl(DinitGenParams gp, DinitPlaneParams pp):
//             the same two for ovp_slam_delayed_init_planes.  pp.slot > 0: the candidate lies on plane pp.slot - 1 of the device plane
//             table: m point-on-plane rows behind the 2m bearing rows (ovp_feat_model.h build_plane_row, the row of k_slam_body.h),
//             the plane's three columns behind the calibration columns, the split of H_f over 3m rows.  The commit also adds the
//             previous correction to the closest point of EVERY plane of the table.  pp.skip != nullptr: this is attempt B of a plane
//             candidate (no plane rows, linearised at p_FinG_noplane, no commit - attempt A did it): nothing to do when A was accepted.
// (in the kernel function itself rather than in a device function template, so that the mono instance stays the kernel it was)
  extern __shared__ double sm[];
  const int t = threadIdx.x;
  const FeatParams& p = dp.fp;
#if DI_PL
  if (pp.skip && pp.skip[1] > 0.5) return;  // (attempt A stands; k_init_update_sk forwards its result block)
#endif
#ifdef OVP_DI_STAMPS
  long long st[12];
  int sti = 0;
#define DI_STAMP() do { if (t == 0) st[sti++] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define DI_STAMP() do { } while (0)
#endif
  DI_STAMP();
  // Everything this kernel reads from global memory is requested HERE, in one batch: a round trip behind a kernel boundary is
  // 2-3 us (the data was just written by other CUs), and the first version paid five of them one after the other (previous
  // result -> clone ids -> tables -> clone slots -> tables again -> P).  The barriers below are LDS-only (no vmcnt(0)): the
  // prefetched operand of the M product stays in flight until it is needed.
  const int l = dp.cand;
  const int m = dp.m_obs;
  const int C = p.n_clones;
  const int ncal = __popc(p.calmask & 0x3FFFu);
#if DI_PL
  const int pl = dp.cand >= 0 ? pp.slot : 0;  // 1-based slot of the candidate's plane, 0 = no plane rows
#if DI_GEN
  const int cols = gp.cols, rows = (pl ? 3 : 2) * m, W = (cols + 4) | 1;  // (gp.cols counts the plane's three columns)
#else
  const int cols = 6 * m + ncal + (pl ? 3 : 0), rows = (pl ? 3 : 2) * m, W = (cols + 4) | 1;
#endif
#elif DI_GEN
  const int cols = gp.cols, rows = 2 * m, W = (cols + 4) | 1;  // (clone blocks of the distinct clones, every camera's calibration)
#else
  const int cols = 6 * m + ncal, rows = 2 * m, W = (cols + 4) | 1;  // [H_f (3) | H_x (cols) | res], odd pitch (LDS banks)
#endif
  const int n_prev = dp.n - 3;  // dimension in front of the previous candidate
  __shared__ double tabR[9 * OVP_MAX_CLONES], tabP[3 * OVP_MAX_CLONES], tabRf[9 * OVP_MAX_CLONES], tabPf[3 * OVP_MAX_CLONES], tabC[20];
  __shared__ double dxs[OVP_LDG_CAP], pf_s[4], okf;
  __shared__ float uv_s[2 * OVP_MAX_MEAS_DEV];
  __shared__ int cid_s[OVP_MAX_CLONES], ci_s[OVP_MAX_MEAS_DEV];
  __shared__ double beta_s, Ri[9];
#if DI_GEN
  __shared__ double tabG[20 * OVP_GEN_MAX_CAMS];  // every camera's tables (ovp_cameras_upload), camera 0 included
  __shared__ int cam_s[OVP_MAX_MEAS_DEV];
#endif
#if DI_PL
  __shared__ double pl_s[OVP_DINIT_PLTAB];  // the candidate's plane: cp | cp_fej | id
  double ldq = 0.0;
  if (pl && t >= 96 && t < 96 + OVP_DINIT_PLTAB) ldq = pp.tab[(size_t)(pl - 1) * OVP_DINIT_PLTAB + (t - 96)];
#endif
  // (a) previous result + tables + this candidate's inputs
  double ld0 = 0.0, ld1 = 0.0, ld2 = 0.0, ld3 = 0.0, ld4 = 0.0;
  float lf0 = 0.f;
  int li0 = 0, li1 = 0;
  if (dp.prev_res && t < dp.n && t < OVP_LDG_CAP) ld0 = dp.prev_res[4 + t];
  if (t < 12 * C) {
    ld1 = t < 9 * C ? dp.clone_R[t] : dp.clone_p[t - 9 * C];
    ld2 = t < 9 * C ? p.clone_R_fej[t] : p.clone_p_fej[t - 9 * C];
  }
  if (t < 20) ld3 = dp.cal[t];
#if DI_GEN
  double ldg = 0.0;
  int lic = 0;
  if (t < 20 * gp.n_cams) ldg = gp.cam_cal[t];
  if (l >= 0 && t < m) lic = gp.cam_idx[(size_t)l * p.max_meas + t];
#endif
  if (t < C) li0 = p.clone_id[t];
  if (t == 0 && dp.prev_res) ld4 = dp.prev_res[1];
  if (l >= 0) {
    if (t < m) li1 = p.clone_idx[(size_t)l * p.max_meas + t];
    if (t < 2 * m) lf0 = p.uv[(size_t)l * p.max_meas * 2 + t];
    if (t >= 64 && t < 67) ld4 = p.p_FinG[3 * l + (t - 64)];
  }
  DI_STAMP();
  DI_STAMP();
  // (c) into LDS
  if (t < OVP_LDG_CAP) dxs[t] = ld0;
  if (t < 9 * C) tabR[t] = ld1, tabRf[t] = ld2;
  else if (t < 12 * C) tabP[t - 9 * C] = ld1, tabPf[t - 9 * C] = ld2;
  if (t < 20) tabC[t] = ld3;
#if DI_GEN
  if (t < 20 * OVP_GEN_MAX_CAMS) tabG[t] = ldg;
  if (l >= 0 && t < m) cam_s[t] = lic;
#endif
  if (t < C) cid_s[t] = li0;
  if (t == 0) okf = ld4;
#if DI_PL
  if (t >= 96 && t < 96 + OVP_DINIT_PLTAB) pl_s[t - 96] = ldq;
#endif
  if (l >= 0) {
    if (t < m) ci_s[t] = li1;
    if (t < 2 * m) uv_s[t] = lf0;
    if (t >= 64 && t < 67) pf_s[t - 64] = ld4;
  }
  di_lds_barrier();
  DI_STAMP();
  // ---- commit of the previous candidate (StateHelper.cpp:188-194 Type::update; the host repeats it on its own copy): the tables
  // in LDS are what the rows below are built at, the global copies what later kernels read ----
  if (dp.prev_res) {
    const bool ok = okf > 0.5;
    if (ok) {
      if (t < C) {
        const int id = cid_s[t];
        dinit_rot_update(tabR + 9 * t, dxs + id);
        for (int k = 0; k < 3; ++k) tabP[3 * t + k] += dxs[id + 3 + k];
        for (int k = 0; k < 9; ++k) dp.clone_R[9 * t + k] = tabR[9 * t + k];
        for (int k = 0; k < 3; ++k) dp.clone_p[3 * t + k] = tabP[3 * t + k];
      } else if (t == 64) {
        if (p.calmask & 0x3Fu) {
          dinit_rot_update(tabC, dxs + p.calcol[0]);
          for (int k = 0; k < 3; ++k) tabC[9 + k] += dxs[p.calcol[3] + k];
        }
        if (p.calmask & (0xFFu << 6))
          for (int k = 0; k < 8; ++k) tabC[12 + k] += dxs[p.calcol[6] + k];
        for (int k = 0; k < 20; ++k) dp.cal[k] = tabC[k];
      }
#if DI_GEN
      else if (t >= 128 && t < 128 + gp.n_cams) {  // every camera of ovp_cameras_upload at its own calibration columns
        const int c = t - 128;
        double* tc = tabG + 20 * c;
        if (p.calmask & 0x3Fu) {
          dinit_rot_update(tc, dxs + gp.cam_calib_id[c]);
          for (int k = 0; k < 3; ++k) tc[9 + k] += dxs[gp.cam_calib_id[c] + 3 + k];
        }
        if (p.calmask & (0xFFu << 6))
          for (int k = 0; k < 8; ++k) tc[12 + k] += dxs[gp.cam_intr_id[c] + k];
        for (int k = 0; k < 20; ++k) gp.cam_cal[20 * c + k] = tc[k];
      }
#endif
#if DI_PL
      else if (t == 65) {  // the candidate's own plane in LDS: the same sum as the table's entry below
        if (pl)
          for (int k = 0; k < 3; ++k) pl_s[k] += dxs[(int)pl_s[6] + k];
      } else if (t >= 256) {  // Vec::update of every plane's closest point (additive), one thread per plane
        for (int q = t - 256; q < pp.n_planes; q += DI_T - 256) {
          double* e = pp.tab + (size_t)q * OVP_DINIT_PLTAB;
          const int id = (int)e[6];
          for (int k = 0; k < 3; ++k) e[k] += dxs[id + k];
        }
      }
#endif
    } else {
      // rejected: its three columns stay as an inert block (nobody reads it; the host removes it after the loop)
      double* P = dp.P;
      for (int e = t; e < 3 * dp.n; e += DI_T) {
        const int k = e / dp.n, r = e - k * dp.n;
        const double v = (r == n_prev + k) ? 1.0 : 0.0;
        P[(size_t)r * p.ldp + n_prev + k] = v;
        P[(size_t)(n_prev + k) * p.ldp + r] = v;
      }
    }
  }
  if (l < 0) return;  // commit only (behind the last candidate)
  double* A = sm;                 // [rows][W] row-major
  double* v = A + (size_t)rows * W;  // [rows] Householder vector
  int* ids_s = (int*)(v + rows + 8);
  DI_STAMP();
  for (int e = t; e < rows * W; e += DI_T) A[e] = 0.0;
#if DI_GEN
  for (int e = t; e < cols; e += DI_T) ids_s[e] = gp.idg[e];
#else
  for (int e = t; e < cols; e += DI_T) ids_s[e] = dp.idv[e];
#endif
  di_lds_barrier();
  DI_STAMP();
#if DI_PL
  if (t < 2 * m) {
#else
  if (t < rows) {
#endif
    const int a = t >> 1, r = t & 1;
    // the measurement model on the LDS copies: tables as the commit above left them, this candidate's inputs as feature 0
    FeatParams q = p;
    q.clone_R = tabR;
    q.clone_p = tabP;
    q.clone_R_fej = tabRf;
    q.clone_p_fej = tabPf;
#if DI_GEN
    const int cam = cam_s[a];
    q.cal = tabG + 20 * cam;
    q.fisheye = gp.cam_fisheye[cam];
    const int oc = 3 + gp.ocol[a], cc = 3 + gp.ccol[cam];  // the observation's clone block, its camera's calibration block
#else
    q.cal = tabC;
    const int oc = 3 + 6 * a, cc = 3 + 6 * m;
#endif
    q.uv = uv_s;
    q.p_FinG = pf_s;
    double jrow[6], crow[14], hf[3], res;
    build_bearing_row(q, 0, a, r, true, ci_s[a], jrow, crow, hf, res);  // (first estimate of the new landmark = its value, :240-246)
    double* h = A + (size_t)t * W;
    h[0] = hf[0], h[1] = hf[1], h[2] = hf[2];
#pragma unroll
    for (int k = 0; k < 6; ++k) h[oc + k] = jrow[k];
#pragma unroll
    for (int k = 0; k < 14; ++k)
      if ((p.calmask >> k) & 1) h[cc + __popc(p.calmask & ((1u << k) - 1u))] = crow[k];
    h[3 + cols] = res;
  }
#if DI_PL
  if (pl && t >= 128 && t < 128 + m) {
    // point-on-plane row of observation t - 128 (all m equal, UpdaterHelper.cpp:503-511); the new landmark's first estimate is its
    // value, the plane has its own
    double hf[3], hc[3], res;
    build_plane_row(pf_s, pf_s, pl_s, pl_s + 3, p.do_fej, pp.white_c, hf, hc, res);
    double* h = A + (size_t)(2 * m + (t - 128)) * W;
#pragma unroll
    for (int k = 0; k < 3; ++k) h[k] = hf[k], h[3 + cols - 3 + k] = hc[k];
    h[3 + cols] = res;
  }
#endif
  di_lds_barrier();
  DI_STAMP();
  // ---- H_f = Q [R3; 0]: three reflectors applied to [H_f | H_x | res] ----
  for (int j = 0; j < 3; ++j) {
    if (t < 64) {  // wave 0: |x|^2 of column j below the diagonal by a wave reduction
      double part = 0.0;
      for (int i = j + t; i < rows; i += 64) part = fma(A[(size_t)i * W + j], A[(size_t)i * W + j], part);
      part += xor_lane_f64<1>(part);   // (DPP + row swaps: plain VALU; wave_sum's ds_bpermute round trips were 1.5 us per reflector)
      part += xor_lane_f64<2>(part);
      part += xor_lane_f64<4>(part);
      part += xor_lane_f64<8>(part);
      const double nn = rows_sum_f64(part);
      if (t == 0) {
        const double x0 = A[(size_t)j * W + j];
        const double alpha = x0 >= 0.0 ? -sqrt(nn) : sqrt(nn);
        const double v0 = x0 - alpha;
        const double vv = nn - x0 * x0 + v0 * v0;
        beta_s = vv > 0.0 ? 2.0 / vv : 0.0;
        v[j] = v0;
      }
    }
    for (int i = j + 1 + t; i < rows; i += DI_T) v[i] = A[(size_t)i * W + j];
    di_lds_barrier();
    // eight lanes per column, each an eighth of the rows; the partial dot products meet inside the group of eight (DPP); columns
    // beyond 128 take a second pass
    for (int cb = j; cb < W; cb += DI_T / 8) {
      const int c = cb + (t >> 3), part = t & 7;
      double s = 0.0;
      if (c < W)
        for (int i = j + part; i < rows; i += 8) s = fma(v[i], A[(size_t)i * W + c], s);
      s += xor_lane_f64<1>(s);
      s += xor_lane_f64<2>(s);
      s += xor_lane_f64<4>(s);
      s *= beta_s;
      if (c < W)
        for (int i = j + part; i < rows; i += 8) A[(size_t)i * W + c] = fma(-s, v[i], A[(size_t)i * W + c]);
    }
    di_lds_barrier();
  }
  DI_STAMP();
  if (t == 0) {
    // R3 upper triangular (rows 0..2 of the H_f columns); H_L^-1 = R3^-1
    const double r00 = A[0], r01 = A[1], r02 = A[2], r11 = A[W + 1], r12 = A[W + 2], r22 = A[2 * W + 2];
    const double i00 = 1.0 / r00, i11 = 1.0 / r11, i22 = 1.0 / r22;
    Ri[0] = i00, Ri[1] = -r01 * i00 * i11, Ri[2] = (r01 * r12 - r02 * r11) * i00 * i11 * i22;
    Ri[3] = 0.0, Ri[4] = i11, Ri[5] = -r12 * i11 * i22;
    Ri[6] = 0.0, Ri[7] = 0.0, Ri[8] = i22;
    // H_Linv * res_init: what the host adds to the new landmark's value (StateHelper.cpp:577)
    const double q0 = A[3 + cols], q1 = A[W + 3 + cols], q2 = A[2 * W + 3 + cols];
    dp.res[4 + dp.n_max + 0] = Ri[0] * q0 + Ri[1] * q1 + Ri[2] * q2;
    dp.res[4 + dp.n_max + 1] = Ri[4] * q1 + Ri[5] * q2;
    dp.res[4 + dp.n_max + 2] = Ri[8] * q2;
    for (int i = 0; i < 9; ++i) dp.Hinv[i] = Ri[i];           // row-major [3][3]
    for (int i = 0; i < 9; ++i) dp.Rk[i] = (i % 4 == 0) ? 1.0 : 0.0;  // R_init = I (:304 R = identity)
  }
  // ---- the stacked transposed system H_all^T [cols][rows] (init rows 0..2, update rows behind) and the update residual ----
  for (int e = t; e < cols * rows; e += DI_T) {
    const int a = e / rows, i = e - a * rows;
    dp.Ht[e] = A[(size_t)i * W + 3 + a];
  }
  for (int i = 3 + t; i < rows; i += DI_T) dp.resid[i - 3] = A[(size_t)i * W + 3 + cols];
