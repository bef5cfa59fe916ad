// The hand-over of a frame's tracks to the feature database in one device pass (ovp_klt_match_frame, k_klt.hip): what the entry
// hands to k_klt_keep_append (k_klt_frame.hip), the database's table as its kernels see it, the one statement of "append an
// observation to a slot" that k_featdb_append and k_klt_keep_append share, and the two host calls through which the tracker's entry
// reaches the database's shadow (k_featdb.hip) - the shadow stays the database's own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct ovp_ctx;

struct FdbTable {
  double* ts;        // [S*M]
  float2 *uv, *uvn;  // [S*M]
  int *count, *del;  // [S]
  long long* id;     // [S]
  int M;
};

// ext FeatureDatabase::update_feature for one observation: placed at count[slot].  A slot a feature has just taken holds what its
// former owner left: the count starts at 0 and the flag is cleared.
__device__ __forceinline__ void fdb_append_one(const FdbTable& t, int s, bool fresh, long long id, double stamp, float2 uv, float2 uvn) {
  const int k = fresh ? 0 : t.count[s];
  if (k >= t.M) return;  // (the host has refused such a frame: never met)
  if (fresh) t.id[s] = id, t.del[s] = 0;
  t.ts[(size_t)s * t.M + k] = stamp;
  t.uv[(size_t)s * t.M + k] = uv;
  t.uvn[(size_t)s * t.M + k] = uvn;
  t.count[s] = k + 1;
}

struct KltFrameArgs {
  int n, cols, rows;                // points; the tracker's image size (the mask's rows are packed: its pitch is cols)
  int to_db;
  const float2* pts;                // [n] where KLT left every point
  const unsigned char* mask_epi;    // [n] status & mask_rsc, or the status alone
  const float2* uvn;                // [n] undistort_cv of pts, or NULL
  const unsigned char* mask;        // [rows][cols] the image mask, or NULL
  // the database's half (to_db): per candidate its slot (a known id) or the fresh flag; the k-th fresh survivor takes free_slots[k]
  const int* slot;
  const unsigned char* fresh;
  const long long* ids;
  const int* free_slots;
  double stamp;
  FdbTable t;
  // published
  unsigned char* keep;              // [n]
  int* kept_index;                  // [n] the first n_kept: the survivors, ascending
  float2 *kept_uv, *kept_uvn;       // [n] the first n_kept (kept_uvn only with uvn)
  int* n_kept;
};

// one launch of k_klt_keep_append on `stream` (n in 1..4096); 0 or a code
int ovp_klt_frame_enqueue(const KltFrameArgs& a, hipStream_t stream);

// ---- the database's side of ovp_klt_match_frame (k_featdb.hip) ----
// Every candidate of a frame against the shadow, nothing touched: slot[i] of a known id (-1 for a fresh one), fresh[i], and
// free_slots[k], k < *n_fresh, in the order ovp_featdb_append would hand slots out.  OVP_E_STATE without a database, OVP_E_ARG for a
// NaN time stamp, OVP_E_CAPACITY for a known id whose slot is full or more fresh candidates than free slots.
int ovp_featdb_frame_plan(ovp_ctx* c, double stamp, int n, const int64_t* ids, int32_t* slot, unsigned char* fresh, int32_t* free_slots,
                          int* n_fresh, FdbTable* table);
// The shadow follows what the device appended: the candidates planned above whose keep [n] is set, in order (the replay is
// ov_plane::frame_plan, host/ov_plane_frame_plan.h).
void ovp_featdb_frame_commit(ovp_ctx* c, double stamp, int n, const int64_t* ids, const unsigned char* keep);
