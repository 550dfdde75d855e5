// vo/localise.hpp -- reading the device map by appearance (vo_map_lookup*, vo_map_localise*): an extension of the facade,
// not a reference interface (the reference never reads its map back).  DeviceMap owns a vo_map: update() is
// PointCloudVector<3>::update, lookup() answers "which entries of the map does this frame see?", localise() "where is this
// camera in the map?" -- lookup -> P3P RANSAC -> PICP rounds, from the frame alone; refine() re-estimates the map's points from
// all the frames that see them, the poses fixed (vo_map_refine), refinePoses() the poses from the map (vo_map_refine_poses),
// adjust() alternates the two (vo_map_adjust), bundle() adjusts both jointly (vox_map_bundle).  A frame that cannot be localised is a
// status in the statistics, not an exception; vo::Error is thrown where the C call refuses.
#pragma once

#include <cmath>

#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "camera.hpp"
#include "context.hpp"
#include "ransac.hpp"
#include "utils.hpp"

namespace vo {

//! defaults of apps/localise: 64 hypotheses, 2 px, seed 0
inline vo_ransac_params localise_ransac_params(float threshold_px = 2.f, int n_hypotheses = 64, uint64_t seed = 0) {
  return ransac_params(threshold_px, n_hypotheses, seed);
}

struct LocaliseOptions {
  vo_ransac_params ransac = localise_ransac_params();   //!< n_hypotheses == 0: no RANSAC, the prior T0 is the start
  float kernel_threshold = 10000.f;
  int n_iters = 50;
  int min_inliers = 6;
};

inline const char* localise_status_name(int status) {
  static const char* names[] = {"OK", "FEW_MATCHES", "NO_CONSENSUS", "FEW_INLIERS", "NOT_FINITE"};
  return status >= 0 && status < 5 ? names[status] : "?";
}

//! vo_map_refine: structure-only adjustment of the map's points (the poses are fixed)
struct RefineOptions {
  int n_rounds = 10;
  int min_obs = 3;
  float huber_px = 0;   //!< 0: squared error
  float damping = 0;
};

inline const char* refine_status_name(int status) {
  static const char* names[] = {"OK", "UNSEEN", "FEW_OBS", "BEHIND", "NOT_FINITE", "COST_ROSE"};
  return status >= 0 && status < 6 ? names[status] : "?";
}

//! vo_map_refine_poses: motion-only adjustment of the frames' poses on the same cost (the points are fixed)
struct PoseRefineOptions {
  int n_rounds = 10;
  int min_obs = 3;
  float huber_px = 0;   //!< 0: squared error
  float damping = 0;
};

inline const char* pose_refine_status_name(int status) {
  static const char* names[] = {"OK", "FIXED", "FEW_OBS", "BEHIND", "NOT_FINITE", "COST_ROSE"};
  return status >= 0 && status < 6 ? names[status] : "?";
}

//! vo_map_adjust: the alternation of the two halves.  A descent, not a fast one.
struct AdjustOptions {
  int n_sweeps = 6;
  int pose_rounds = 2, point_rounds = 2;
  int min_obs_pose = 3, min_obs_point = 3;
  float huber_px = 0;
  float damping = 0;
};

//! vox_map_bundle: the joint adjustment -- Levenberg-Marquardt rounds, the reduced camera system solved by matrix-free PCG
//!
struct BundleOptions {
  int n_rounds = 3;
  int n_cg = 64;
  float cg_tol = 1e-8f;
  float lambda0 = 1e-4f;
  int min_obs_pose = 3, min_obs_point = 3;
  float huber_px = 0;
};

//! voe_map_cull: which landmarks leave the map.  A threshold of 0 switches its test off.
struct CullOptions {
  int min_obs = 3;
  int min_frames = 2;
  float max_rms_px = 2.f;
  float max_err_px = 0;
  float min_parallax_deg = 0;
  bool drop_unseen = false;
  bool dry_run = false;
};
inline const char* cull_verdict_name(int verdict) {
  static const char* names[] = {"KEPT", "UNSEEN", "FEW_OBS", "FEW_FRAMES", "NOT_FINITE", "BEHIND", "HIGH_ERROR", "LOW_PARALLAX"};
  return verdict >= 0 && verdict < 8 ? names[verdict] : "?";
}

//! voe_map_grow: which tracks of unmapped rows become landmarks.  A threshold of 0 switches its test off;
//! max_added 0 means one per row of the window.
struct GrowOptions {
  int n_rounds = 5;
  int min_obs = 3;
  int min_frames = 3;
  float huber_px = 0;
  float damping = 0;
  float max_rms_px = 2.f;
  float max_err_px = 0;
  float min_parallax_deg = 2.f;
  int max_added = 0;
  bool dry_run = false;
};
inline const char* grow_verdict_name(int verdict) {
  static const char* names[] = {"ADDED", "FEW_OBS", "FEW_FRAMES", "DEGENERATE", "NOT_FINITE", "BEHIND", "HIGH_ERROR", "LOW_PARALLAX", "NO_ROOM"};
  return verdict >= 0 && verdict < 9 ? names[verdict] : "?";
}

//! voe_map_covis: which entries every frame sees and how many every two frames share
struct Covisibility {
  size_t n_frames = 0, n_words = 0;
  std::vector<uint32_t> bits;        //!< [n_frames][n_words]: bit e & 31 of word e >> 5 of row f is set when frame f sees entry e
  std::vector<int32_t> counts;       //!< [n_frames][n_frames], or empty when not asked for
  voe_map_covis_stats stats{};
  bool sees(size_t f, size_t e) const { return (bits[f * n_words + (e >> 5)] >> (e & 31)) & 1u; }
  int32_t shared(size_t f, size_t g) const { return counts[f * n_frames + g]; }
};
//! voe_map_window: the local window of a frame
struct WindowOptions {
  int k_free = 8;                    //!< frames to free, the query among them
  int k_fixed = 8;                   //!< frames to hold
  int min_shared = 15;               //!< entries a frame must share to be a candidate
};
struct MapWindow {
  std::vector<int32_t> role;         //!< VOE_MAP_WINDOW_OUTSIDE / _FREE / _FIXED per frame
  std::vector<int> n_rows;           //!< the frame's live rows inside the window, 0 outside: what bundle / adjust / cull take
  std::vector<uint8_t> fixed;        //!< 0 for the free frames, 1 otherwise: the mask bundle / adjust take
  std::vector<int32_t> order;        //!< the free frames in rank order (the query first), the fixed frames in rank order, then -1
  std::vector<uint32_t> landmarks;   //!< [n_words] the OR of the free frames' rows
  voe_map_window_stats stats{};
};
inline const char* window_status_name(int status) {
  static const char* names[] = {"OK", "NO_FIXED", "QUERY_UNSEEN"};
  return status >= 0 && status < 3 ? names[status] : "?";
}

//! voe_map_align: how two maps of one scene relate.  threshold in the units of the map aligned TO.
struct AlignOptions {
  float threshold = 0.05f;
  int n_hypotheses = 64;
  uint64_t seed = 1;
  bool with_scale = true;
  int n_refits = 1;
  int min_inliers = 3;
};
inline const char* align_status_name(int status) {
  static const char* names[] = {"OK", "FEW_MATCHES", "NO_HYPOTHESIS", "FEW_INLIERS"};
  return status >= 0 && status < 4 ? names[status] : "?";
}
//! a similarity [c R | t] as the library hands it out: column-major 4x4, last row 0 0 0 1
struct Similarity3f {
  float m[16];
  float operator()(int r, int c) const { return m[r + 4 * c]; }
  const float* data() const { return m; }
  static Similarity3f Identity() { Similarity3f S{}; S.m[0] = S.m[5] = S.m[10] = S.m[15] = 1.f; return S; }
};
//! The pose of a frame of src's in the map moved by S: T (p_cam = T p_src) and S = [c R | t] (p_dst = S p_src) give the rigid
//! T' = [R_T R^T | c t_T - R_T R^T t], on the host in double.  T' p_dst = c T p_src: camera points only scale by c, so every
//! projection is unchanged.
inline Isometry3f similarity_pose(const Isometry3f& T, const Similarity3f& S) {
  double M[3][3], det;
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) M[r][c] = S(r, c);
  det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
        M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
  const double c = std::cbrt(det);
  Isometry3f out = Isometry3f::Identity();
  double Rn[3][3];
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) {                              // R_T R^T, R = M / c
      Rn[r][k] = ((double)T(r, 0) * M[k][0] + (double)T(r, 1) * M[k][1] + (double)T(r, 2) * M[k][2]) / c;
      out(r, k) = (float)Rn[r][k];
    }
  for (int r = 0; r < 3; ++r)
    out(r, 3) = (float)(c * (double)T(r, 3) - (Rn[r][0] * (double)S(0, 3) + Rn[r][1] * (double)S(1, 3) + Rn[r][2] * (double)S(2, 3)));
  return out;
}

//! voe_map_loops: the loop edges a drifted map shows (include/vo_map_loops.h)
struct LoopsOptions {
  int gap = 50;                      //!< a loop (i, j) has i < j - gap
  int ref_window = 5;                //!< the band of i: the entries whose reference frame lies in [i - ref_window, i]
  int min_shared = 12;               //!< entries of the band frame j must see
  int separation = 3;                //!< candidates this close suppress each other
  int max_loops = 8;                 //!< slots
  LocaliseOptions measure;           //!< the P3P RANSAC and the PICP rounds of every slot
  float w_loop[3] = {1.f, 1.f, 1.f}; //!< (w_t, w_r, w_s) of every OK edge
};
struct MapLoops {
  std::vector<int32_t> edges;        //!< [max_loops][2] (i, j); (-1, -1) for an empty slot
  std::vector<Similarity3f> Z;       //!< [max_loops] Z_ij ~ S_j S_i^-1; the identity unless the slot is OK
  std::vector<float> weights;        //!< [max_loops][3]; 0 0 0 unless the slot is OK: voe_pose_graph skips such an edge
  std::vector<voe_map_loop_record> loops;   //!< [max_loops]
  std::vector<int32_t> hist;         //!< [n_frames][n_frames], or empty when not asked for
  std::vector<int32_t> ref_frame;    //!< [map size], or empty when not asked for
  voe_map_loops_stats stats{};
};
inline const char* loop_status_name(int status) {
  static const char* names[] = {"OK", "FEW_MATCHES", "NO_CONSENSUS", "FEW_INLIERS", "NOT_FINITE", "EMPTY"};
  return status >= 0 && status < 6 ? names[status] : "?";
}

//! voe_map_nearest: frames associated with the map by the nearest appearance within a radius (include/vo_hip.h, NEAREST; DESIGN.md
//! section 4.23)
struct NearestOptions {
  float radius = 0.1f;               //!< an entry matches when its squared distance is below radius^2
  float ratio = 0.f;                 //!< 0: off; otherwise a row whose best is not below ratio^2 times its second best is AMBIGUOUS
  bool unique = false;               //!< an entry keeps its closest row of a frame, the others are DISPLACED
};
struct MapNearest {
  std::vector<std::vector<int32_t>> entry;     //!< per frame, per row: the entry, -1 unless MATCHED
  std::vector<std::vector<int32_t>> status;    //!< VOE_MAP_NEAREST_*
  std::vector<std::vector<float>> dist2;       //!< the best squared distance, +inf where there is none
  std::vector<Vector10fVector> canonical;      //!< the rows as every map call is to see them: matched rows carry their entry's bytes
  voe_map_nearest_stats stats{};
};
inline const char* nearest_status_name(int status) {
  static const char* names[] = {"MATCHED", "NO_ENTRY", "AMBIGUOUS", "DISPLACED", "NAN_ROW", "NOT_LIVE"};
  return status >= 0 && status < 6 ? names[status] : "?";
}

//! voe_map_guided: frames associated with the map by the nearest appearance among the entries that project, under a pose prior,
//! within a pixel window of the row (include/vo_hip.h, GUIDED)
struct GuidedOptions {
  float radius_px = 8.f;             //!< an entry is a candidate when it projects within radius_px of the row's pixel
  float radius = 0.1f;               //!< ... and its squared appearance distance is below radius^2
  float ratio = 0.f;                 //!< 0: off; otherwise a row whose best is not below ratio^2 times its second-best candidate is AMBIGUOUS
  bool unique = false;               //!< an entry keeps its closest row of a frame, the others are DISPLACED
};
struct MapGuided {
  std::vector<std::vector<int32_t>> entry;     //!< per frame, per row: the entry, -1 unless MATCHED
  std::vector<std::vector<int32_t>> status;    //!< VOE_MAP_GUIDED_*
  std::vector<std::vector<float>> dist2;       //!< the best squared appearance distance, +inf where there is none
  std::vector<std::vector<float>> pix2;        //!< the squared pixel distance of that candidate, +inf where there is none
  std::vector<Vector10fVector> canonical;      //!< the rows as every map call is to see them: matched rows carry their entry's bytes
  voe_map_guided_stats stats{};
};
inline const char* guided_status_name(int status) {
  static const char* names[] = {"MATCHED", "NO_ENTRY", "AMBIGUOUS", "DISPLACED", "NAN_ROW", "NOT_LIVE"};
  return status >= 0 && status < 6 ? names[status] : "?";
}

//! voe_map_fuse: duplicate landmarks of the map -- mutual nearest in appearance within a radius in space -- fused (include/vo_hip.h,
//! FUSE)
struct FuseOptions {
  float radius_xyz = 0.04f;          //!< two entries can be one landmark when their points lie within radius_xyz
  float radius = 0.1f;               //!< ... and their squared appearance distance is below radius^2
  bool midpoint = true;              //!< the survivor's point becomes the midpoint of the two (false: it keeps its own)
  bool veto_shared_frame = false;    //!< with frames: a pair that some frame sees together is two landmarks and stays
  bool dry_run = false;              //!< everything is reported, the map and the rows stay as they are
};
struct MapFuse {
  std::vector<int32_t> partner;      //!< per old entry: its partner, -1 for none
  std::vector<float> dist2, gap2;    //!< the partner's squared appearance distance and squared distance in space, +inf for none
  std::vector<int32_t> verdict;      //!< VOE_MAP_FUSE_*
  std::vector<int32_t> remap;        //!< the new index of the entry, for an ABSORBED entry that of its survivor
  std::vector<Vector10fVector> rows; //!< with frames: the rows as the fused map finds them (rows on an absorbed entry carry the survivor's bytes)
  voe_map_fuse_stats stats{};
};
inline const char* fuse_verdict_name(int verdict) {
  static const char* names[] = {"NOT_FINITE", "ALONE", "NOT_MUTUAL", "CONFLICT", "SURVIVOR", "ABSORBED"};
  return verdict >= 0 && verdict < 6 ? names[verdict] : "?";
}

//! voe_map_keyframes: which frames to keep at all -- redundant frames dropped one at a time, the most redundant first
//! (include/vo_hip.h, KEYFRAMES)
struct KeyframesOptions {
  int min_observers = 3;             //!< other kept frames that must see an entry for it to count as redundant in a frame
  int share_permille = 900;          //!< a frame is a candidate when that many of 1000 of its entries are redundant
  int min_seen = 1;                  //!< a frame that sees fewer entries is EMPTY and stays
  int max_gap = 0;                   //!< > 0: no run of more than max_gap missing frames in the chain
  int max_dropped = VOE_MAP_KEYFRAMES_MAX_STEPS;      //!< 0: the analysis alone
};
struct MapKeyframes {
  std::vector<int32_t> verdict;      //!< VOE_MAP_KEYFRAMES_* per frame
  std::vector<int> n_rows;           //!< the frame's live rows, 0 for DROPPED and GONE: what refine / bundle / adjust / cull / grow / loops take
  std::vector<uint8_t> keep;         //!< 0 for DROPPED and GONE, 1 otherwise: the flags of the next call are keep ? flag : GONE
  std::vector<int32_t> step;         //!< the step at which the frame was dropped, or -1
  std::vector<int32_t> order;        //!< the dropped frames in drop order, then -1
  std::vector<int32_t> seen, red;    //!< entries seen / of them redundant: at its own step for a dropped frame, at the end otherwise
  voe_map_keyframes_stats stats{};
};
inline const char* keyframes_verdict_name(int verdict) {
  static const char* names[] = {"LEFT", "PROTECTED", "GONE", "DROPPED", "EMPTY", "NEEDED", "GAP"};
  return verdict >= 0 && verdict < 7 ? names[verdict] : "?";
}

//! voe_map_prune: single observations taken out of their frames, with a guard per landmark and per frame (include/vo_hip.h,
//! PRUNE)
struct PruneOptions {
  float max_err_px = 0.f;            //!< > 0: an eligible observation with |e| above it is HIGH_ERROR
  float rel_factor = 0.f;            //!< > 0: ... with |e| above rel_factor times its landmark's (lower) median is RELATIVE
  float rel_floor_px = 0.f;          //!< RELATIVE only above this
  int rel_min_obs = 3;               //!< RELATIVE only on landmarks with that many eligible observations (at least 3)
  bool unique = true;                //!< of the rows of one frame on one entry only the best stays
  int max_share_landmark = 1000;     //!< more soft observations than that many of 1000: the landmark is at fault, its rows stay
  int max_share_frame = 1000;        //!< the same for a frame, after the landmarks
};
struct MapPrune {
  std::vector<int32_t> entry;        //!< per frame and row (the longest frame's length each): the entry of a row that stays, or -1
  std::vector<int32_t> status;       //!< VOE_MAP_PRUNE_* per frame and row
  std::vector<double> sq;            //!< |e|^2 of an observation, +inf elsewhere
  std::vector<Vector10fVector> appearances;      //!< the frames' rows, a pruned row's first component a NaN: what the other map calls take
  std::vector<voe_map_prune_landmark> landmarks; //!< one record per entry of the map
  std::vector<voe_map_prune_frame> frames;       //!< one record per frame
  size_t n_max = 0;                  //!< the row length of entry, status and sq
  voe_map_prune_stats stats{};
};
inline const char* prune_status_name(int status) {
  static const char* names[] = {"KEPT", "NOT_LIVE", "MISS", "NOT_FINITE", "BEHIND", "DUPLICATE", "HIGH_ERROR", "RELATIVE", "LANDMARK_AT_FAULT", "FRAME_AT_FAULT"};
  return status >= 0 && status < 10 ? names[status] : "?";
}

//! The rigid pose that goes with a similarity S = [c R | t] of the pose graph (vo/pose_graph.hpp): [R | t / c], on the host in
//! double.  A map point moved by S_new^-1 S_old of its reference frame (DeviceMap::applyCorrection) projects there, under
//! rigid_pose(S_new), where it projected before.
inline Isometry3f rigid_pose(const Similarity3f& S) {
  double M[3][3];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) M[r][c] = S(r, c);
  const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                     M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
  const double c = std::cbrt(det);
  Isometry3f out = Isometry3f::Identity();
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) out(r, k) = (float)(M[r][k] / c);
    out(r, 3) = (float)((double)S(r, 3) / c);
  }
  return out;
}

class DeviceMap {
 public:
  explicit DeviceMap(int capacity = 0, Context& ctx = default_context()) : ctx_(ctx.handle()) {
    check(vo_map_create(ctx_, capacity, &h_), "vo_map_create");
  }
  ~DeviceMap() { if (h_) vo_map_destroy(h_); }
  DeviceMap(const DeviceMap&) = delete;
  DeviceMap& operator=(const DeviceMap&) = delete;
  vo_map* handle() const { return h_; }

  //! map.update(T * cloud) (PointCloud.h:52-66)
  void update(const Vector3fVector& points, const Vector10fVector& appearances, const Isometry3f* T = nullptr) {
    if (points.size() != appearances.size()) throw Error(VO_ERR_INVALID_ARG, "DeviceMap::update: points and appearances differ in size");
    check(vo_map_update(h_, points.empty() ? nullptr : points[0].data(), appearances.empty() ? nullptr : appearances[0].data(),
                        (int)points.size(), T ? T->data() : nullptr), "vo_map_update");
  }
  int size() const { int n = 0; check(vo_map_size(h_, &n), "vo_map_size"); return n; }
  void clear() { check(vo_map_clear(h_), "vo_map_clear"); }

  //! the hits in query order as (query index, entry index); *points: the hit entries' points; *entries: the entry of every
  //! query, -1 for none
  IntPairVector lookup(const Vector10fVector& appearances, Vector3fVector* points = nullptr, std::vector<int32_t>* entries = nullptr) const {
    const int n = (int)appearances.size();
    IntPairVector pairs(appearances.size());
    if (points) points->resize(appearances.size());
    if (entries) entries->assign(appearances.size(), -1);
    int k = 0;
    check(vo_map_lookup(h_, n ? appearances[0].data() : nullptr, n, n ? pair_data(pairs) : nullptr, &k,
                        points && n ? (*points)[0].data() : nullptr, entries && n ? entries->data() : nullptr), "vo_map_lookup");
    pairs.resize((size_t)k);
    if (points) points->resize((size_t)k);
    return pairs;
  }

  //! pose of the camera in the map (p_cam = T * p_map) from one frame; stats->status says whether it is one (VO_MAP_LOCALISE_*):
  //! otherwise the result is *T0, or the identity
  Isometry3f localise(const Camera& cam, const Vector2fVector& pixels, const Vector10fVector& appearances,
                      const LocaliseOptions& opt = LocaliseOptions(), vo_map_localise_stats* stats = nullptr,
                      const Isometry3f* T0 = nullptr) const {
    if (pixels.size() != appearances.size()) throw Error(VO_ERR_INVALID_ARG, "DeviceMap::localise: pixels and appearances differ in size");
    Isometry3f T = Isometry3f::Identity();
    vo_map_localise_stats s{};
    check(vo_map_localise(h_, cam.rows(), cam.cols(), cam.zNear(), cam.zFar(), cam.cameraMatrix().data(), detail::ptr(pixels),
                          appearances.empty() ? nullptr : appearances[0].data(), (int)pixels.size(), &opt.ransac, opt.kernel_threshold,
                          opt.n_iters, opt.min_inliers, T0 ? T0->data() : nullptr, T.data(), &s), "vo_map_localise");
    if (stats) *stats = s;
    return T;
  }

  //! every frame of `pixels` / `appearances` in ONE call (vo_map_localise_batch_dev): padded to the largest frame, uploaded,
  //! localised, read back.  stats (if given) receives one entry per frame.
  IsometryVector localise_batch(const Camera& cam, const std::vector<Vector2fVector>& pixels, const std::vector<Vector10fVector>& appearances,
                                const LocaliseOptions& opt = LocaliseOptions(), std::vector<vo_map_localise_stats>* stats = nullptr,
                                const IsometryVector* T0 = nullptr) const {
    const size_t F = pixels.size();
    if (appearances.size() != F || (T0 && T0->size() != F)) throw Error(VO_ERR_INVALID_ARG, "DeviceMap::localise_batch: per-frame arrays differ in size");
    IsometryVector out(F, Isometry3f::Identity());
    if (stats) stats->assign(F, vo_map_localise_stats{});
    if (F == 0) return out;
    size_t cap = 1;
    for (size_t f = 0; f < F; ++f) {
      if (pixels[f].size() != appearances[f].size()) throw Error(VO_ERR_INVALID_ARG, "DeviceMap::localise_batch: pixels and appearances differ in size");
      if (pixels[f].size() > cap) cap = pixels[f].size();
    }
    std::vector<float> uv(F * cap * 2, 0.f), app(F * cap * 10, 0.f);
    std::vector<int> n(F);
    for (size_t f = 0; f < F; ++f) {
      n[f] = (int)pixels[f].size();
      for (size_t i = 0; i < pixels[f].size(); ++i) {
        for (int k = 0; k < 2; ++k) uv[(f * cap + i) * 2 + k] = pixels[f][i][k];
        for (int k = 0; k < 10; ++k) app[(f * cap + i) * 10 + k] = appearances[f][i][k];
      }
    }
    struct Buf {
      vo_ctx* c; void* p = nullptr;
      Buf(vo_ctx* ctx, size_t bytes, const void* src) : c(ctx) {
        check(vo_dev_alloc(c, bytes, &p), "vo_dev_alloc");
        if (src) { const int rc = vo_memcpy_h2d(c, p, src, bytes); if (rc != VO_OK) { vo_dev_free(c, p); check(rc, "vo_memcpy_h2d"); } }
      }
      ~Buf() { if (p) vo_dev_free(c, p); }
      Buf(const Buf&) = delete;
      Buf& operator=(const Buf&) = delete;
    };
    Buf d_uv(ctx_, uv.size() * sizeof(float), uv.data()), d_app(ctx_, app.size() * sizeof(float), app.data());
    Buf d_n(ctx_, F * sizeof(int), n.data()), d_T(ctx_, F * 64, nullptr), d_st(ctx_, F * sizeof(vo_map_localise_stats), nullptr);
    Buf d_T0(ctx_, F * 64, T0 ? (const void*)(*T0)[0].data() : nullptr);
    check(vo_map_localise_batch_dev(h_, (int)F, cam.rows(), cam.cols(), cam.zNear(), cam.zFar(), cam.cameraMatrix().data(),
                                    static_cast<const float*>(d_uv.p), cap, static_cast<const float*>(d_app.p), cap, (int)cap,
                                    static_cast<const int*>(d_n.p), &opt.ransac, opt.kernel_threshold, opt.n_iters, opt.min_inliers,
                                    T0 ? static_cast<const float*>(d_T0.p) : nullptr, static_cast<float*>(d_T.p),
                                    static_cast<vo_map_localise_stats*>(d_st.p)), "vo_map_localise_batch_dev");
    check(vo_memcpy_d2h(ctx_, out[0].data(), d_T.p, F * 64), "vo_memcpy_d2h");
    if (stats) check(vo_memcpy_d2h(ctx_, stats->data(), d_st.p, F * sizeof(vo_map_localise_stats)), "vo_memcpy_d2h");
    return out;
  }

  //! every point of the map re-estimated, in place, from all the rows of the frames that see it, the poses (p_cam = T p_map,
  //! one per frame) fixed (vo_map_refine: the frames are padded to the largest one and uploaded).  *status receives one
  //! VO_MAP_REFINE_* per entry; only OK entries are replaced.
  void refine(const Camera& cam, const std::vector<Vector2fVector>& pixels, const std::vector<Vector10fVector>& appearances,
              const IsometryVector& poses, const RefineOptions& opt = RefineOptions(), vo_map_refine_stats* stats = nullptr,
              std::vector<int32_t>* status = nullptr) {
    const Window w = pack("DeviceMap::refine", pixels, appearances, poses);
    if (status) status->assign((size_t)size(), -1);
    const vo_map_refine_params prm{opt.n_rounds, opt.min_obs, opt.huber_px, opt.damping};
    vo_map_refine_stats s{};
    check(vo_map_refine(h_, (int)w.F, cam.cameraMatrix().data(), w.uv.data(), w.app.data(), w.n.data(), (int)w.cap, w.T.data(), &prm,
                        status && !status->empty() ? status->data() : nullptr, &s), "vo_map_refine");
    if (stats) *stats = s;
  }

  //! every frame's pose (p_cam = T p_map) re-estimated, in place, from all its rows that hit an entry, the map fixed
  //! (vo_map_refine_poses: the other half of the same cost).  fixed: one flag per frame, or null for none.  *status receives
  //! one VO_MAP_POSE_* per frame; only OK poses are replaced.  *information: per frame the damped 6x6 H of the last solved
  //! round, column-major (36 doubles; NaN for a frame that never solved).
  void refinePoses(const Camera& cam, const std::vector<Vector2fVector>& pixels, const std::vector<Vector10fVector>& appearances,
                   IsometryVector& poses, const std::vector<uint8_t>* fixed = nullptr, const PoseRefineOptions& opt = PoseRefineOptions(),
                   vo_map_pose_refine_stats* stats = nullptr, std::vector<int32_t>* status = nullptr,
                   std::vector<double>* information = nullptr) {
    Window w = pack("DeviceMap::refinePoses", pixels, appearances, poses, fixed);
    if (status) status->assign(w.F, -1);
    if (information) information->assign(w.F * 36, std::numeric_limits<double>::quiet_NaN());
    const vo_map_pose_refine_params prm{opt.n_rounds, opt.min_obs, opt.huber_px, opt.damping};
    vo_map_pose_refine_stats s{};
    check(vo_map_refine_poses(h_, (int)w.F, cam.cameraMatrix().data(), w.uv.data(), w.app.data(), w.n.data(), (int)w.cap, w.T.data(),
                              fixed ? fixed->data() : nullptr, &prm, status ? status->data() : nullptr,
                              information ? information->data() : nullptr, &s), "vo_map_refine_poses");
    for (size_t f = 0; f < w.F; ++f)
      for (int k = 0; k < 16; ++k) poses[f].data()[k] = w.T[16 * f + k];
    if (stats) *stats = s;
  }

  //! block-coordinate bundle adjustment (vo_map_adjust): opt.n_sweeps times refinePoses in place on `poses`, then refine in
  //! place on the map.  Hold the gauge with `fixed`: with no frame held the solution drifts in its seven free parameters.
  //! *sweeps receives one pair of statistics per sweep; the statuses are those of the last sweep.
  void adjust(const Camera& cam, const std::vector<Vector2fVector>& pixels, const std::vector<Vector10fVector>& appearances,
              IsometryVector& poses, const std::vector<uint8_t>* fixed, const AdjustOptions& opt = AdjustOptions(),
              std::vector<vo_map_adjust_stats>* sweeps = nullptr, std::vector<int32_t>* pose_status = nullptr,
              std::vector<int32_t>* point_status = nullptr) {
    Window w = pack("DeviceMap::adjust", pixels, appearances, poses, fixed);
    if (pose_status) pose_status->assign(w.F, -1);
    if (point_status) point_status->assign((size_t)size(), -1);
    const vo_map_adjust_params prm{opt.n_sweeps, opt.pose_rounds, opt.point_rounds, opt.min_obs_pose, opt.min_obs_point, opt.huber_px, opt.damping};
    std::vector<vo_map_adjust_stats> s((size_t)(opt.n_sweeps > 0 ? opt.n_sweeps : 1));
    check(vo_map_adjust(h_, (int)w.F, cam.cameraMatrix().data(), w.uv.data(), w.app.data(), w.n.data(), (int)w.cap, w.T.data(),
                        fixed ? fixed->data() : nullptr, &prm, pose_status ? pose_status->data() : nullptr,
                        point_status && !point_status->empty() ? point_status->data() : nullptr, s.data()), "vo_map_adjust");
    for (size_t f = 0; f < w.F; ++f)
      for (int k = 0; k < 16; ++k) poses[f].data()[k] = w.T[16 * f + k];
    if (sweeps) *sweeps = s;
  }

  //! joint bundle adjustment (vox_map_bundle): the free frames' poses in place on `poses`, the free landmarks' points in place on
  //! the map, only when the call's status (the returned statistics) is VOX_MAP_BUNDLE_OK.  Hold the gauge with `fixed`.
  //! *rounds receives one record per round; the statuses say which frames and landmarks were free.
  vox_map_bundle_stats bundle(const Camera& cam, const std::vector<Vector2fVector>& pixels, const std::vector<Vector10fVector>& appearances,
                              IsometryVector& poses, const std::vector<uint8_t>* fixed, const BundleOptions& opt = BundleOptions(),
                              std::vector<vox_map_bundle_round>* rounds = nullptr, std::vector<int32_t>* pose_status = nullptr,
                              std::vector<int32_t>* point_status = nullptr) {
    Window w = pack("DeviceMap::bundle", pixels, appearances, poses, fixed);
    if (pose_status) pose_status->assign(w.F, -1);
    if (point_status) point_status->assign((size_t)size(), -1);
    const vox_map_bundle_params prm{opt.n_rounds, opt.n_cg, opt.cg_tol, opt.lambda0, opt.min_obs_pose, opt.min_obs_point, opt.huber_px};
    std::vector<vox_map_bundle_round> r((size_t)(opt.n_rounds > 0 ? opt.n_rounds : 1));
    vox_map_bundle_stats st{};
    check(vox_map_bundle(h_, (int)w.F, cam.cameraMatrix().data(), w.uv.data(), w.app.data(), w.n.data(), (int)w.cap, w.T.data(),
                         fixed ? fixed->data() : nullptr, &prm, pose_status ? pose_status->data() : nullptr,
                         point_status && !point_status->empty() ? point_status->data() : nullptr, r.data(), &st), "vox_map_bundle");
    for (size_t f = 0; f < w.F; ++f)
      for (int k = 0; k < 16; ++k) poses[f].data()[k] = w.T[16 * f + k];
    r.resize((size_t)(opt.n_rounds > 0 ? opt.n_rounds : 0));
    if (rounds) *rounds = r;
    return st;
  }

  //! landmarks taken out of the map (voe_map_cull): every entry judged from all the rows of the frames that see it, the poses
  //! (p_cam = T p_map, one per frame) given; the survivors keep their order.  *verdict receives one VOE_MAP_CULL_* per OLD entry,
  //! *remap its new index or -1, *entries its statistics.  With opt.dry_run the map stays as it is.
  voe_map_cull_stats cull(const Camera& cam, const std::vector<Vector2fVector>& pixels, const std::vector<Vector10fVector>& appearances,
                          const IsometryVector& poses, const CullOptions& opt = CullOptions(), std::vector<int32_t>* verdict = nullptr,
                          std::vector<int32_t>* remap = nullptr, std::vector<voe_map_cull_entry>* entries = nullptr) {
    const Window w = pack("DeviceMap::cull", pixels, appearances, poses);
    const size_t M = (size_t)size();
    if (verdict) verdict->assign(M, -1);
    if (remap) remap->assign(M, -1);
    if (entries) entries->assign(M, voe_map_cull_entry{});
    const voe_map_cull_params prm{opt.min_obs, opt.min_frames, opt.max_rms_px, opt.max_err_px, opt.min_parallax_deg, opt.drop_unseen ? 1 : 0,
                                  opt.dry_run ? 1 : 0};
    voe_map_cull_stats st{};
    check(voe_map_cull(h_, (int)w.F, cam.cameraMatrix().data(), w.uv.data(), w.app.data(), w.n.data(), (int)w.cap, w.T.data(), &prm,
                       verdict && M ? verdict->data() : nullptr, remap && M ? remap->data() : nullptr,
                       entries && M ? entries->data() : nullptr, &st), "voe_map_cull");
    return st;
  }

  //! landmarks added from the frames (voe_map_grow): the rows that find no entry are grouped into tracks by equal appearance, every
  //! track is triangulated from all its rows at the poses (p_cam = T p_map, one per frame) given, refined, judged by the cull's
  //! tests and, when it passes, appended.  *rows receives, frame by frame (the longest frame's length each), the entry every row
  //! is found at afterwards (-1: no row or a NaN; -2 - t: its track t was not added), *tracks one record per track.  With
  //! opt.dry_run the map stays as it is.
  voe_map_grow_stats grow(const Camera& cam, const std::vector<Vector2fVector>& pixels, const std::vector<Vector10fVector>& appearances,
                          const IsometryVector& poses, const GrowOptions& opt = GrowOptions(), std::vector<int32_t>* rows = nullptr,
                          std::vector<voe_map_grow_track>* tracks = nullptr) {
    const Window w = pack("DeviceMap::grow", pixels, appearances, poses);
    const size_t R = w.F * w.cap;
    if (rows) rows->assign(R, -1);
    if (tracks) tracks->assign(R, voe_map_grow_track{});
    const voe_map_grow_params prm{opt.n_rounds, opt.min_obs, opt.min_frames, opt.huber_px, opt.damping, opt.max_rms_px, opt.max_err_px,
                                  opt.min_parallax_deg, opt.max_added, opt.dry_run ? 1 : 0};
    voe_map_grow_stats st{};
    check(voe_map_grow(h_, (int)w.F, cam.cameraMatrix().data(), w.uv.data(), w.app.data(), w.n.data(), (int)w.cap, w.T.data(), &prm,
                       rows && R ? rows->data() : nullptr, tracks && R ? tracks->data() : nullptr, tracks && R ? (int)R : 0, &st), "voe_map_grow");
    if (tracks) tracks->resize((size_t)st.n_tracks < R ? (size_t)st.n_tracks : R);
    return st;
  }

  //! the similarity S with p_this ~ S p_src from the landmarks the two maps share (voe_map_align): 3-point RANSAC, then
  //! opt.n_refits Umeyama refits over the inliers.  S is the identity unless stats->status is VOE_MAP_ALIGN_OK.  *pairs: the
  //! matches as (src entry, entry of this map); *inliers: one byte per match.
  Similarity3f align(const DeviceMap& src, const AlignOptions& opt = AlignOptions(), voe_map_align_stats* stats = nullptr,
                     IntPairVector* pairs = nullptr, std::vector<uint8_t>* inliers = nullptr) const {
    const size_t n = (size_t)src.size();
    IntPairVector pr(n ? n : 1);
    std::vector<uint8_t> mask(n ? n : 1, 0);
    const voe_map_align_params prm{opt.seed, opt.n_hypotheses, opt.with_scale ? 1 : 0, opt.n_refits, opt.min_inliers, opt.threshold, 0};
    voe_map_align_stats st{};
    Similarity3f S = Similarity3f::Identity();
    int k = 0;
    check(voe_map_align(h_, src.h_, &prm, S.m, pair_data(pr), &k, mask.data(), nullptr, &st), "voe_map_align");
    pr.resize((size_t)k); mask.resize((size_t)k);
    if (stats) *stats = st;
    if (pairs) *pairs = pr;
    if (inliers) *inliers = mask;
    return S;
  }

  //! src's entries, moved by S (or as they are), into this map (voe_map_merge): VOE_MAP_MERGE_TAKE_SRC as update does, or
  //! VOE_MAP_MERGE_KEEP_DST appending only what this map does not hold.  *remap: the entry of this map per src entry, or -1.
  voe_map_merge_stats merge(const DeviceMap& src, const Similarity3f* S = nullptr, int policy = VOE_MAP_MERGE_TAKE_SRC,
                            std::vector<int32_t>* remap = nullptr) {
    const size_t n = (size_t)src.size();
    if (remap) remap->assign(n, -1);
    voe_map_merge_stats st{};
    check(voe_map_merge(h_, src.h_, S ? S->m : nullptr, policy, remap && n ? remap->data() : nullptr, &st), "voe_map_merge");
    return st;
  }

  //! the covisibility of frames (voe_map_covis): the entries every frame's rows find, as bit rows, and -- with want_counts --
  //! the number of entries every two frames share.  Two rows of one frame that hit one entry see it once.
  Covisibility covisibility(const std::vector<Vector10fVector>& appearances, bool want_counts = true) const {
    Covisibility c;
    const size_t F = c.n_frames = appearances.size();
    size_t cap = 0;
    for (const auto& a : appearances) cap = a.size() > cap ? a.size() : cap;
    std::vector<float> app(F * cap * 10 + 10, 0.f);
    std::vector<int> n(F + 1, 0);
    for (size_t f = 0; f < F; ++f) {
      n[f] = (int)appearances[f].size();
      for (size_t i = 0; i < appearances[f].size(); ++i)
        for (int k = 0; k < 10; ++k) app[(f * cap + i) * 10 + k] = appearances[f][i][k];
    }
    int bound = 0;
    check(voe_map_size_bound(h_, &bound), "voe_map_size_bound");
    c.n_words = (size_t)(bound > 0 ? (bound + 31) / 32 : 1);
    c.bits.assign((F ? F : 1) * c.n_words, 0u);
    if (want_counts) c.counts.assign((F ? F : 1) * (F ? F : 1), 0);
    check(voe_map_covis(h_, (int)F, app.data(), n.data(), (int)cap, (int)c.n_words, c.bits.data(), want_counts ? c.counts.data() : nullptr,
                        &c.stats), "voe_map_covis");
    return c;
  }

  //! the nearest entry within a radius for every row of every frame, and the rows canonicalised (voe_map_nearest): hand
  //! `canonical` to any other call of this class in place of the appearances and it sees the association decided here
  MapNearest nearest(const std::vector<Vector10fVector>& appearances, const NearestOptions& o = NearestOptions()) const {
    MapNearest r;
    const size_t F = appearances.size();
    size_t cap = 0;
    for (const auto& a : appearances) cap = a.size() > cap ? a.size() : cap;
    std::vector<float> app(F * cap * 10 + 10, 0.f), d2(F * cap + 1, 0.f);
    std::vector<int> n(F + 1, 0);
    std::vector<int32_t> ent(F * cap + 1, -1), st(F * cap + 1, VOE_MAP_NEAREST_NOT_LIVE);
    for (size_t f = 0; f < F; ++f) {
      n[f] = (int)appearances[f].size();
      for (size_t i = 0; i < appearances[f].size(); ++i)
        for (int k = 0; k < 10; ++k) app[(f * cap + i) * 10 + k] = appearances[f][i][k];
    }
    const voe_map_nearest_params p{o.radius, o.ratio, o.unique ? 1 : 0, 0};
    check(voe_map_nearest(h_, (int)F, app.data(), n.data(), (int)cap, &p, ent.data(), st.data(), d2.data(), app.data(), &r.stats), "voe_map_nearest");
    r.entry.resize(F); r.status.resize(F); r.dist2.resize(F); r.canonical.resize(F);
    for (size_t f = 0; f < F; ++f) {
      const size_t m = appearances[f].size();
      r.entry[f].assign(ent.begin() + f * cap, ent.begin() + f * cap + m);
      r.status[f].assign(st.begin() + f * cap, st.begin() + f * cap + m);
      r.dist2[f].assign(d2.begin() + f * cap, d2.begin() + f * cap + m);
      r.canonical[f].resize(m);
      for (size_t i = 0; i < m; ++i) std::memcpy(r.canonical[f][i].data(), &app[(f * cap + i) * 10], sizeof(float) * 10);
    }
    return r;
  }

  //! the same for a tracker that has a pose prior per frame (p_cam = T p_map): only the entries that project within
  //! o.radius_px of a row's pixel are its candidates (voe_map_guided; the camera gives K and the depth gate).  `canonical`
  //! then feeds localise(..., T0 = the prior) with n_hypotheses == 0: tracking against the map.
  MapGuided guided(const Camera& camera, const std::vector<Vector2fVector>& pixels, const std::vector<Vector10fVector>& appearances,
                   const IsometryVector& poses, const GuidedOptions& o = GuidedOptions()) const {
    MapGuided r;
    const size_t F = appearances.size();
    if (pixels.size() != F || poses.size() != F) throw Error(VO_ERR_INVALID_ARG, "DeviceMap::guided: per-frame arrays differ in size");
    size_t cap = 0;
    for (size_t f = 0; f < F; ++f) {
      if (pixels[f].size() != appearances[f].size()) throw Error(VO_ERR_INVALID_ARG, "DeviceMap::guided: pixels and appearances differ in size");
      cap = appearances[f].size() > cap ? appearances[f].size() : cap;
    }
    std::vector<float> uv(F * cap * 2 + 2, 0.f), app(F * cap * 10 + 10, 0.f), d2(F * cap + 1, 0.f), g2(F * cap + 1, 0.f), T(F * 16 + 16, 0.f);
    std::vector<int> n(F + 1, 0);
    std::vector<int32_t> ent(F * cap + 1, -1), st(F * cap + 1, VOE_MAP_GUIDED_NOT_LIVE);
    for (size_t f = 0; f < F; ++f) {
      n[f] = (int)appearances[f].size();
      std::memcpy(&T[16 * f], poses[f].data(), sizeof(float) * 16);
      for (size_t i = 0; i < appearances[f].size(); ++i) {
        for (int k = 0; k < 2; ++k) uv[(f * cap + i) * 2 + k] = pixels[f][i][k];
        for (int k = 0; k < 10; ++k) app[(f * cap + i) * 10 + k] = appearances[f][i][k];
      }
    }
    const voe_map_guided_params p{o.radius_px, o.radius, o.ratio, o.unique ? 1 : 0, camera.zNear(), camera.zFar(), {0, 0}};
    check(voe_map_guided(h_, (int)F, camera.cameraMatrix().data(), uv.data(), app.data(), n.data(), (int)cap, T.data(), &p, ent.data(), st.data(),
                         d2.data(), g2.data(), app.data(), &r.stats), "voe_map_guided");
    r.entry.resize(F); r.status.resize(F); r.dist2.resize(F); r.pix2.resize(F); r.canonical.resize(F);
    for (size_t f = 0; f < F; ++f) {
      const size_t m = appearances[f].size();
      r.entry[f].assign(ent.begin() + f * cap, ent.begin() + f * cap + m);
      r.status[f].assign(st.begin() + f * cap, st.begin() + f * cap + m);
      r.dist2[f].assign(d2.begin() + f * cap, d2.begin() + f * cap + m);
      r.pix2[f].assign(g2.begin() + f * cap, g2.begin() + f * cap + m);
      r.canonical[f].resize(m);
      for (size_t i = 0; i < m; ++i) std::memcpy(r.canonical[f][i].data(), &app[(f * cap + i) * 10], sizeof(float) * 10);
    }
    return r;
  }

  //! duplicate landmarks fused (voe_map_fuse): two entries that are each other's nearest in appearance within o.radius among the
  //! entries within o.radius_xyz in space are one landmark; the higher index is absorbed, the survivors keep their order.  With
  //! frames (may be empty: none) the veto can be asked for, and `rows` comes back for the other calls of this class.
  MapFuse fuse(const FuseOptions& o = FuseOptions(), const std::vector<Vector10fVector>& appearances = std::vector<Vector10fVector>()) {
    MapFuse r;
    const size_t F = appearances.size(), S = (size_t)size();
    size_t cap = 0;
    for (const auto& a : appearances) cap = a.size() > cap ? a.size() : cap;
    std::vector<float> app(F * cap * 10 + 10, 0.f);
    std::vector<int> n(F + 1, 0);
    for (size_t f = 0; f < F; ++f) {
      n[f] = (int)appearances[f].size();
      for (size_t i = 0; i < appearances[f].size(); ++i)
        for (int k = 0; k < 10; ++k) app[(f * cap + i) * 10 + k] = appearances[f][i][k];
    }
    r.partner.assign(S + 1, -1); r.verdict.assign(S + 1, -1); r.remap.assign(S + 1, -1);
    r.dist2.assign(S + 1, 0.f); r.gap2.assign(S + 1, 0.f);
    const voe_map_fuse_params p{o.radius_xyz, o.radius, o.midpoint ? 1 : 0, o.veto_shared_frame ? 1 : 0, o.dry_run ? 1 : 0, {0, 0, 0}};
    check(voe_map_fuse(h_, (int)F, F ? app.data() : nullptr, F ? n.data() : nullptr, (int)cap, &p, r.partner.data(), r.dist2.data(), r.gap2.data(),
                       r.verdict.data(), r.remap.data(), F && cap ? app.data() : nullptr, &r.stats), "voe_map_fuse");
    r.partner.resize(S); r.verdict.resize(S); r.remap.resize(S); r.dist2.resize(S); r.gap2.resize(S);
    r.rows.resize(F);
    for (size_t f = 0; f < F; ++f) {
      r.rows[f].resize(appearances[f].size());
      for (size_t i = 0; i < appearances[f].size(); ++i) std::memcpy(r.rows[f][i].data(), &app[(f * cap + i) * 10], sizeof(float) * 10);
    }
    return r;
  }

  //! a trajectory's correction carried into the map (voe_map_apply_correction): every entry some row of the frames sees moves by
  //! S_new[f]^-1 S_old[f] of its reference frame f, the frame of its first observation.  *ref_frame: that frame per entry, -1 for
  //! an entry no row sees.  With dry_run the map stays as it is.
  voe_map_apply_stats applyCorrection(const std::vector<Vector10fVector>& appearances, const std::vector<Similarity3f>& S_old,
                                      const std::vector<Similarity3f>& S_new, bool dry_run = false, std::vector<int32_t>* ref_frame = nullptr) {
    const size_t F = appearances.size();
    if (S_old.size() != F || S_new.size() != F) throw Error(VO_ERR_INVALID_ARG, "DeviceMap::applyCorrection: one similarity per frame, before and after");
    size_t cap = 0;
    for (const auto& a : appearances) cap = a.size() > cap ? a.size() : cap;
    std::vector<float> app(F * cap * 10 + 10, 0.f);
    std::vector<int> n(F + 1, 0);
    for (size_t f = 0; f < F; ++f) {
      n[f] = (int)appearances[f].size();
      for (size_t i = 0; i < appearances[f].size(); ++i)
        for (int k = 0; k < 10; ++k) app[(f * cap + i) * 10 + k] = appearances[f][i][k];
    }
    std::vector<int32_t> ref((size_t)size() + 1, -1);
    voe_map_apply_stats st{};
    check(voe_map_apply_correction(h_, (int)F, nullptr, app.data(), n.data(), (int)cap, F ? S_old[0].m : nullptr, F ? S_new[0].m : nullptr,
                                   dry_run ? 1 : 0, ref.data(), &st), "voe_map_apply_correction");
    ref.resize((size_t)st.n_entries);
    if (ref_frame) *ref_frame = ref;
    return st;
  }

  //! the loop edges this map shows (voe_map_loops): frame j's candidate is the i < j - gap whose band holds the most entries j
  //! sees; the best max_loops candidates are measured by P3P RANSAC + PICP of frame j against the band of i, and the result goes
  //! to PoseGraph::addLoops.  S: the drifted similarities, one per frame (p_cam = S p_map).  The map is not written.
  MapLoops loops(const Camera& cam, const std::vector<Vector2fVector>& pixels, const std::vector<Vector10fVector>& appearances,
                 const std::vector<Similarity3f>& S, const LoopsOptions& opt = LoopsOptions(), bool want_hist = false, bool want_ref_frame = false) const {
    const size_t F = pixels.size();
    if (appearances.size() != F || S.size() != F) throw Error(VO_ERR_INVALID_ARG, "DeviceMap::loops: per-frame arrays differ in size");
    size_t cap = 1;
    for (size_t f = 0; f < F; ++f) {
      if (pixels[f].size() != appearances[f].size()) throw Error(VO_ERR_INVALID_ARG, "DeviceMap::loops: pixels and appearances differ in size");
      if (pixels[f].size() > cap) cap = pixels[f].size();
    }
    std::vector<float> uv(F * cap * 2 + 2, 0.f), app(F * cap * 10 + 10, 0.f);
    std::vector<int> n(F + 1, 0);
    for (size_t f = 0; f < F; ++f) {
      n[f] = (int)pixels[f].size();
      for (size_t i = 0; i < pixels[f].size(); ++i) {
        for (int k = 0; k < 2; ++k) uv[(f * cap + i) * 2 + k] = pixels[f][i][k];
        for (int k = 0; k < 10; ++k) app[(f * cap + i) * 10 + k] = appearances[f][i][k];
      }
    }
    const size_t L = (size_t)(opt.max_loops > 0 ? opt.max_loops : 1);
    MapLoops out;
    out.edges.assign(2 * L, -1); out.Z.assign(L, Similarity3f::Identity()); out.weights.assign(3 * L, 0.f); out.loops.assign(L, voe_map_loop_record{});
    if (want_hist) out.hist.assign((F ? F : 1) * (F ? F : 1), 0);
    if (want_ref_frame) out.ref_frame.assign((size_t)size() + 1, -1);
    voe_map_loops_params prm{};
    prm.gap = opt.gap; prm.ref_window = opt.ref_window; prm.min_shared = opt.min_shared; prm.separation = opt.separation; prm.max_loops = opt.max_loops;
    prm.ransac = opt.measure.ransac; prm.kernel_threshold = opt.measure.kernel_threshold; prm.n_iters = opt.measure.n_iters;
    prm.min_inliers = opt.measure.min_inliers;
    for (int k = 0; k < 3; ++k) prm.w_loop[k] = opt.w_loop[k];
    check(voe_map_loops(h_, (int)F, cam.rows(), cam.cols(), cam.zNear(), cam.zFar(), cam.cameraMatrix().data(), uv.data(), app.data(), n.data(), (int)cap,
                        F ? S[0].m : nullptr, &prm, out.edges.data(), out.Z[0].m, out.weights.data(), out.loops.data(),
                        want_hist ? out.hist.data() : nullptr, want_ref_frame ? out.ref_frame.data() : nullptr, &out.stats), "voe_map_loops");
    if (want_ref_frame) out.ref_frame.resize((size_t)out.stats.n_entries);
    return out;
  }

  //! the local window of frame `query` (voe_map_window) from the bit rows of covisibility(): the frames to free, the frames to
  //! hold, the landmarks between them.  *n_rows: the frames' live rows (what the result's n_rows hands on for the window's
  //! frames).  The result's n_rows and fixed go to bundle / adjust / cull over the SAME frames.
  MapWindow window(const Covisibility& cov, int query, const WindowOptions& opt = WindowOptions(), const std::vector<int>* n_rows = nullptr) const {
    const size_t F = cov.n_frames;
    if (n_rows && n_rows->size() != F) throw Error(VO_ERR_INVALID_ARG, "DeviceMap::window: one row count per frame");
    MapWindow w;
    w.role.assign(F ? F : 1, 0); w.n_rows.assign(F ? F : 1, 0); w.fixed.assign(F ? F : 1, 1); w.order.assign(F ? F : 1, -1);
    w.landmarks.assign(cov.n_words ? cov.n_words : 1, 0u);
    int cap = 0;
    if (n_rows) for (int v : *n_rows) cap = v > cap ? v : cap;
    const voe_map_window_params prm{query, opt.k_free, opt.k_fixed, opt.min_shared};
    check(voe_map_window(h_, (int)F, (int)cov.n_words, cov.bits.data(), n_rows ? n_rows->data() : nullptr, cap, &prm, w.role.data(),
                         w.n_rows.data(), w.fixed.data(), w.order.data(), w.landmarks.data(), &w.stats), "voe_map_window");
    w.role.resize(F); w.n_rows.resize(F); w.fixed.resize(F); w.order.resize(F);
    return w;
  }

  //! the frames to keep (voe_map_keyframes) from the bit rows of covisibility().  *flags: VOE_MAP_KEYFRAMES_FREE / _PROTECTED /
  //! _GONE per frame (default: all free); *n_rows: the frames' live rows.  The result's n_rows goes to refine / bundle / adjust /
  //! cull / grow / loops over the SAME frames: a dropped frame has no observation there.
  MapKeyframes keyframes(const Covisibility& cov, const KeyframesOptions& opt = KeyframesOptions(), const std::vector<uint8_t>* flags = nullptr,
                         const std::vector<int>* n_rows = nullptr) const {
    const size_t F = cov.n_frames;
    if (n_rows && n_rows->size() != F) throw Error(VO_ERR_INVALID_ARG, "DeviceMap::keyframes: one row count per frame");
    if (flags && flags->size() != F) throw Error(VO_ERR_INVALID_ARG, "DeviceMap::keyframes: one flag per frame");
    MapKeyframes k;
    const size_t n = F ? F : 1;
    k.verdict.assign(n, 0); k.n_rows.assign(n, 0); k.keep.assign(n, 1); k.step.assign(n, -1); k.order.assign(n, -1); k.seen.assign(n, 0); k.red.assign(n, 0);
    int cap = 0;
    if (n_rows) for (int v : *n_rows) cap = v > cap ? v : cap;
    const voe_map_keyframes_params prm{opt.min_observers, opt.share_permille, opt.min_seen, opt.max_gap, opt.max_dropped, {0, 0, 0}};
    check(voe_map_keyframes(h_, (int)F, (int)cov.n_words, cov.bits.data(), n_rows ? n_rows->data() : nullptr, cap, flags ? flags->data() : nullptr,
                            &prm, k.verdict.data(), k.n_rows.data(), k.keep.data(), k.step.data(), k.order.data(), k.seen.data(), k.red.data(),
                            &k.stats), "voe_map_keyframes");
    k.verdict.resize(F); k.n_rows.resize(F); k.keep.resize(F); k.step.resize(F); k.order.resize(F); k.seen.resize(F); k.red.resize(F);
    return k;
  }

  //! single observations pruned (voe_map_prune): every observation of the frames judged on its own at the poses (p_cam = T p_map,
  //! one per frame) given; the map is not written.  The result's appearances go to refine / bundle / cull / grow in place of the
  //! frames' own: a pruned row finds nothing there.  Named landmarks want DeviceMap::refine, named frames refinePoses.
  MapPrune prune(const Camera& cam, const std::vector<Vector2fVector>& pixels, const std::vector<Vector10fVector>& appearances,
                 const IsometryVector& poses, const PruneOptions& opt = PruneOptions()) const {
    const Window w = pack("DeviceMap::prune", pixels, appearances, poses);
    const size_t M = (size_t)size(), R = w.F * w.cap;
    MapPrune r;
    r.n_max = w.cap;
    r.entry.assign(R + 1, -1); r.status.assign(R + 1, VOE_MAP_PRUNE_NOT_LIVE); r.sq.assign(R + 1, 0.0);
    r.landmarks.assign(M + 1, voe_map_prune_landmark{}); r.frames.assign(w.F + 1, voe_map_prune_frame{});
    std::vector<float> out(w.app.size(), 0.f);
    const voe_map_prune_params prm{opt.max_err_px, opt.rel_factor, opt.rel_floor_px, opt.rel_min_obs, opt.unique ? 1 : 0, opt.max_share_landmark,
                                   opt.max_share_frame, 0};
    check(voe_map_prune(h_, (int)w.F, cam.cameraMatrix().data(), w.uv.data(), w.app.data(), w.n.data(), (int)w.cap, w.T.data(), &prm, r.entry.data(),
                        r.status.data(), r.sq.data(), out.data(), r.landmarks.data(), r.frames.data(), &r.stats), "voe_map_prune");
    r.entry.resize(R); r.status.resize(R); r.sq.resize(R); r.landmarks.resize(M); r.frames.resize(w.F);
    r.appearances = appearances;
    for (size_t f = 0; f < w.F; ++f)
      for (size_t i = 0; i < appearances[f].size(); ++i)
        for (int k = 0; k < 10; ++k) r.appearances[f][i][k] = out[(f * w.cap + i) * 10 + k];
    return r;
  }

  //! the map's points and appearances in entry order
  void read(Vector3fVector& points, Vector10fVector& appearances) const {
    const int n = size();
    points.resize((size_t)n); appearances.resize((size_t)n);
    int m = 0;
    if (n > 0) check(vo_map_read(h_, points[0].data(), appearances[0].data(), n, &m), "vo_map_read");
  }

 private:
  //! the frames of a window padded to the largest one, as the host forms of the refinement calls take them
  struct Window {
    size_t F = 0, cap = 0;
    std::vector<float> uv, app, T;
    std::vector<int> n;
  };
  static Window pack(const char* who, const std::vector<Vector2fVector>& pixels, const std::vector<Vector10fVector>& appearances,
                     const IsometryVector& poses, const std::vector<uint8_t>* fixed = nullptr) {
    Window w;
    const size_t F = w.F = pixels.size();
    if (appearances.size() != F || poses.size() != F || (fixed && fixed->size() != F))
      throw Error(VO_ERR_INVALID_ARG, std::string(who) + ": per-frame arrays differ in size");
    size_t cap = 0;
    for (size_t f = 0; f < F; ++f) {
      if (pixels[f].size() != appearances[f].size()) throw Error(VO_ERR_INVALID_ARG, std::string(who) + ": pixels and appearances differ in size");
      if (pixels[f].size() > cap) cap = pixels[f].size();
    }
    w.cap = cap;
    w.uv.assign(F * cap * 2 + 2, 0.f); w.app.assign(F * cap * 10 + 10, 0.f); w.T.assign(F * 16 + 16, 0.f);
    w.n.assign(F + 1, 0);
    for (size_t f = 0; f < F; ++f) {
      w.n[f] = (int)pixels[f].size();
      for (size_t i = 0; i < pixels[f].size(); ++i) {
        for (int k = 0; k < 2; ++k) w.uv[(f * cap + i) * 2 + k] = pixels[f][i][k];
        for (int k = 0; k < 10; ++k) w.app[(f * cap + i) * 10 + k] = appearances[f][i][k];
      }
      for (int k = 0; k < 16; ++k) w.T[16 * f + k] = poses[f].data()[k];
    }
    return w;
  }

  vo_ctx* ctx_ = nullptr;
  vo_map* h_ = nullptr;
};

//! free functions with the library's error behaviour
inline IntPairVector map_lookup(const DeviceMap& map, const Vector10fVector& appearances, Vector3fVector* points = nullptr) {
  return map.lookup(appearances, points);
}
inline Isometry3f map_localise(const DeviceMap& map, const Camera& cam, const Vector2fVector& pixels, const Vector10fVector& appearances,
                               const LocaliseOptions& opt = LocaliseOptions(), vo_map_localise_stats* stats = nullptr,
                               const Isometry3f* T0 = nullptr) {
  return map.localise(cam, pixels, appearances, opt, stats, T0);
}

}  // namespace vo
