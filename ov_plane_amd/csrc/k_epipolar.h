// The epipolar check of TrackPlane::perform_matching (track_plane/TrackPlane.cpp:1331-1350): what ovp_klt_epipolar (k_klt.hip) hands
// to the kernels of k_epipolar.hip.  tests/epi_ref.py defines the stage.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int EPI_MAX_ITERS = 1024;        // hypotheses of one call
constexpr int EPI_MAX_SUBSET_TRIES = 8;    // sets tried per hypothesis (our own constant)
constexpr int EPI_MAX_DRAWS = 256;         // draws per hypothesis, whatever they were spent on (our own constant)
constexpr int EPI_MIN_POINTS = 10;         // :1319

struct EpiInfoDev {  // the device's half of ovp_epipolar_info, in its layout
  double F[9];
  int32_t best_count, winner_h, winner_model, niters, n_with_model, too_few, no_model, stop;
};

struct EpiLaunch {
  int n, max_iters, mode;
  unsigned seed;
  double intr[8];
  float thr2;                        // (float)(threshold^2): the error is compared as a float
  const float *pts0, *pts1;          // [2n] each, as uploaded
  const unsigned char* status;       // [n]
  const int* table;                  // [n + 1]
  // intermediate results, kept for ovp_klt_debug
  int* samples;                      // [max_iters][7], -1 without a set
  int* n_models;                     // [max_iters]
  double* models;                    // [max_iters][3][9]
  int* counts;                       // [max_iters][3]
  // published
  float *uvn0, *uvn1;                // [2n] each
  unsigned char* mask;               // [n]
  EpiInfoDev* info;
  hipEvent_t* ev;                    // NULL, or five events around the four kernels
};

// the four launches on `stream`; 0 or an OVP_E_* code
int ovp_epi_enqueue(const EpiLaunch& a, hipStream_t stream);
// k_epi_undistort alone (both point sets, the kernel as it is): uvn0 / uvn1 of pts0 / pts1, nothing else written
int ovp_epi_enqueue_undistort(const EpiLaunch& a, hipStream_t stream);
// table[c] = RANSACUpdateNumIters(confidence, (n - c) / n, 7, max_iters), c = 0..n, with the host's libm
void ovp_epi_table(int n, double confidence, int max_iters, int32_t* table);
