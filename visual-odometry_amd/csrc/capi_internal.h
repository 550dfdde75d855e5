// capi_internal.h -- what the two host translation units behind the extern "C" boundary share: capi.hip (context, events,
// graphs, PICP, matcher, frames, RANSAC, epipolar) and capi_map.hip (the map).  Included by those two only.
#pragma once

#include "../../include/vo_hip.h"
#include "vo_internal.h"
#include "map_checks.h"      // aligned8, invert_k
#include "ws_poison.h"       // the test hook of DevBuf::ensure

#define VO_HIDDEN __attribute__((visibility("hidden")))

#define VO_HIP_CHECK(expr)                                                              \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) {                                                             \
      (void)hipGetLastError(); /* reported here: must not resurface in the next call's launch check */ \
      return vo_fail(_e == hipErrorOutOfMemory ? VO_ERR_OUT_OF_MEMORY : VO_ERR_HIP,     \
                     "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    }                                                                                   \
  } while (0)

#define VO_REQUIRE(cond, msg) \
  do { if (!(cond)) return vo_fail(VO_ERR_INVALID_ARG, "%s: %s", __func__, msg); } while (0)

// entry points that copy host memory or wait for the stream cannot be part of a graph capture (vo_ctx_begin_capture): refused
// BEFORE any HIP call, because a refused HIP call would invalidate the capture in progress
#define VO_NOT_CAPTURING(ctx) \
  do { if ((ctx)->capturing) return vo_fail(VO_ERR_NOT_READY, "%s: not allowed inside a graph capture (only *_dev entry points are)", __func__); } while (0)

struct VO_HIDDEN DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  bool keeps_state = false;   // the buffer carries data from one ensure() to a later one on purpose ("The workspace contract")
  DevBuf() = default;
  explicit DevBuf(bool state) : keeps_state(state) {}
  static bool capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
  }
  // grow-only; contents are NOT preserved.  A call reads nothing from a workspace that the same call has not written first:
  // under the test hook VO_WS_POISON=<byte> (ws_poison.h) every ensure() outside a graph capture fills all `cap` bytes with the
  // byte, on the call's stream -- a buffer that keeps state only when it grows.  Unset: the HIP calls below and no other.
  hipError_t ensure(size_t bytes, hipStream_t st) {
    const int poison = ws_poison_byte();
    if (bytes <= cap) {
      if (poison < 0 || keeps_state || !p || capturing(st)) return hipSuccess;
      return hipMemsetAsync(p, poison, cap, st);
    }
    // growing frees, allocates and synchronises: none of it may happen inside a graph capture
    if (capturing(st)) return hipErrorStreamCaptureUnsupported;
    if (p) {
      hipError_t e = hipStreamSynchronize(st);
      if (e != hipSuccess) return e;
      (void)hipFree(p);
      p = nullptr; cap = 0;
    }
    size_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) { p = nullptr; return e; }
    cap = want;
    return poison < 0 ? hipSuccess : hipMemsetAsync(p, poison, cap, st);
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct vo_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int n_cu = 0;
  char name[128] = "";
  DevBuf scratch;     // compaction counts
  DevBuf best;        // matcher keys
  DevBuf table;       // join table
  // staging for host-pointer entry points
  DevBuf in[6] = {DevBuf(true), DevBuf(true), DevBuf(true), DevBuf(true), DevBuf(true), DevBuf(true)};   // keeps_state: a host form's uploads, from the copy in to the launches that read them
  DevBuf out[3] = {DevBuf(true), DevBuf(true), DevBuf(true)};   // keeps_state: a host form's results, from the launches that write them to the copy back
  DevBuf counts;      // small device ints
  DevBuf batch_pack;  // packed correspondences of the batched solver
  DevBuf batch_bad;   // its per-problem bad-index counters
  DevBuf batch_states{true};   // launch-per-round form of the batched solver: per-problem state.  keeps_state: the parameter block behind the states, as last uploaded (batch_params_dev)
  DevBuf batch_partials;       //   ... and its partial rows
  DevBuf batch_help;  // shared form (fewer problems than CUs): tagged words handed between workgroups
  vo::PicpParams batch_params_host{};    //   its parameter block as last uploaded, and where
  const vo::PicpParams* batch_params_dev = nullptr;
  DevBuf prune_ws;    // sorted copies / tables of the matcher's sorted searches
  DevBuf epi_ws;      // maxima, A^T A and vote counts of vo_estimate_transform
  DevBuf ransac_ws;   // points, hypotheses, counts, mask and inlier pairs of vo_estimate_transform_ransac
  DevBuf pose_ws;     // the same for vo_estimate_pose_ransac
  DevBuf pose_batch_ws;   // ... and for vo_estimate_pose_ransac_batch_dev (all problems' blocks)
  DevBuf refine_ws;   // state and workgroup rows of vo_refine_transform_dev
  DevBuf track_ws;    // vo_frames_batch_track_dev: the moved cloud, the tracked pairs and the winners the caller did not ask for
  DevBuf pose_graph_ws;   // voe_pose_graph*: the state in double, the edges' records, the incidence lists and the PCG vectors
  // Steering of the automatic matcher by what the previous batched call found: after a call that ran the
  // exact-duplicate pass, "did any frame take it?" travels to pinned host memory behind the call (no wait); a later call
  // that finds the answer "none" there leaves the pass out for the next HINT_SKIP calls, then probes again.  Data whose
  // descriptors are recomputed per frame (no bitwise copies, ever) then pays the sampling pass once in seventeen calls.
  // A call that ran WITHOUT the pass asks the same question of the keys the search left (a sample query at distance 0 from
  // its match): the answer "yes" ends the skipping at once, so data that regains its copies loses one or two calls, not sixteen.
  // vo_match_set_mode() forgets what was learnt.
  int* hint_host = nullptr;        // pinned
  int* hint_dev = nullptr;
  hipEvent_t hint_ev = nullptr;
  bool hint_pending = false;
  int hint_skip_left = 0;
  bool hint_of_skipped_call = false;   // what the pending answer was asked of
  int hint_none_streak = 0;            // consecutive answers "no frame took the pass": two in a row start the skipping (a context
                                       // that alternates between data with and without copies is then never steered wrong)
  int match_mode = 0; // 0 auto, 1 full scan, 2 bucket-pruned scan, 3 cell-hash search, 4 / 5 exact-duplicate pass first, then 2 / 3
  int batch_form = 0; // batched solver: 0 auto, 1 one launch per round, 2 one workgroup per problem
  int batch_last_form = 0, batch_last_wgs = 0;   // what the last batched call ran as (vo_picp_batch_info)
  int batch_last_help_rows = 0, batch_last_problems = 0, batch_last_help_mode = 0;   // ... and where its helper record lies (vo_picp_batch_help_info)
  bool capturing = false;
  unsigned long long id = 0;   // unique per context ever created: an address can be reused, an id cannot
};

// ---- defined in capi.hip ------------------------------------------------------------------------------------------------------
VO_HIDDEN int set_device(vo_ctx* ctx);
VO_HIDDEN int upload(vo_ctx* c, DevBuf& b, const void* src, size_t bytes);
VO_HIDDEN int ensure_counts(vo_ctx* c);
VO_HIDDEN bool ctx_alive(const vo_ctx* c);
VO_HIDDEN bool ctx_alive(const vo_ctx* c, unsigned long long id);   // ... and still THAT context, not a new one at the recycled address
extern "C" VO_HIDDEN int ransac_check_params(const vo_ransac_params* p);   // (extern "C": defined among the entry points, like the two below)
// vo_picp_set_camera and vo_picp_set_kernel_threshold without the pose upload (the pose comes from device memory); the
// parameters go to the device again only when they differ from the handle's
extern "C" VO_HIDDEN void picp_set_camera_threshold(vo_picp* s, int rows, int cols, int z_near, int z_far, const float K[9], float thr);
extern "C" VO_HIDDEN const vo::PicpState* picp_state_dev(const vo_picp* s);   // the handle's state on the device (vo_picp itself stays capi.hip's)
