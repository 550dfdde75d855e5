// vo/ransac.hpp -- estimate_transform behind RANSAC (vo_estimate_transform_ransac): an extension of the facade, not a
// reference interface.  n_hypotheses minimal 8-point fits are scored by Sampson distance on the GPU; the pose is the
// plain GPU estimate_transform of the best hypothesis's inliers (bit for bit vo_estimate_transform of those pairs).
// estimate_pose_ransac (vo_estimate_pose_ransac): the tracking counterpart -- minimal P3P fits over 2D-3D pairs scored by
// reprojection on the GPU; the winner's pose and inliers are the start and the input of the PICP rounds that follow.
// estimate_pose_ransac_batch (vo_estimate_pose_ransac_batch_dev): the same for many problems in device memory in one call.
#pragma once

#include <cstdint>
#include <vector>

#include "camera.hpp"
#include "context.hpp"
#include "utils.hpp"

namespace vo {

//! defaults of apps/vo_complete --ransac: 2048 hypotheses, 1 px, seed 0
inline vo_ransac_params ransac_params(float threshold_px = 1.f, int n_hypotheses = 2048, uint64_t seed = 0) {
  vo_ransac_params p;
  p.n_hypotheses = n_hypotheses; p.threshold_px = threshold_px; p.seed = seed;
  return p;
}

//! pose of the first camera in the frame of the second from the inliers of the best hypothesis; *inliers (if given)
//! receives one 0/1 per correspondence
inline Isometry3f estimate_transform_ransac(const Matrix3f& k, const IntPairVector& correspondences, const Vector2fVector& p1_img,
                                            const Vector2fVector& p2_img, const vo_ransac_params& params,
                                            std::vector<uint8_t>* inliers = nullptr) {
  const int n = (int)correspondences.size();
  if (inliers) inliers->assign(correspondences.size(), 0);
  Isometry3f X = Isometry3f::Identity();
  check(vo_estimate_transform_ransac(default_context().handle(), k.data(), n ? pair_data(correspondences) : nullptr, n,
                                     detail::ptr(p1_img), (int)p1_img.size(), detail::ptr(p2_img), (int)p2_img.size(), &params,
                                     X.data(), inliers && n ? inliers->data() : nullptr, nullptr),
        "estimate_transform_ransac");
  return X;
}

//! defaults of apps/vo_complete --track-ransac: 2048 hypotheses, 1 px, seed 0
inline vo_ransac_params track_ransac_params(float threshold_px = 1.f, int n_hypotheses = 2048, uint64_t seed = 0) {
  return ransac_params(threshold_px, n_hypotheses, seed);
}

//! pose of the camera (world in camera, what Camera::setWorldInCameraPose takes) from the best of n_hypotheses P3P fits
//! of the correspondences (meas_idx, world_idx) -- the solver's orientation; *inliers (if given) receives one 0/1 per
//! correspondence.  Throws vo::Error where vo_estimate_pose_ransac refuses (fewer than 4 pairs, no valid hypothesis, a
//! winner with fewer than 6 inliers, a bad index, bad parameters).
inline Isometry3f estimate_pose_ransac(const Camera& cam, const Vector3fVector& world_points, const Vector2fVector& image_points,
                                       const IntPairVector& correspondences, const vo_ransac_params& params,
                                       std::vector<uint8_t>* inliers = nullptr) {
  const int n = (int)correspondences.size();
  if (inliers) inliers->assign(correspondences.size(), 0);
  Isometry3f T = Isometry3f::Identity();
  check(vo_estimate_pose_ransac(default_context().handle(), cam.rows(), cam.cols(), cam.zNear(), cam.zFar(), cam.cameraMatrix().data(),
                                world_points.empty() ? nullptr : world_points[0].data(), (int)world_points.size(),
                                detail::ptr(image_points), (int)image_points.size(), n ? pair_data(correspondences) : nullptr, n,
                                &params, T.data(), inliers && n ? inliers->data() : nullptr, nullptr),
        "estimate_pose_ransac");
  return T;
}

//! defaults of the batched tracking options (apps/batch_frames --track-ransac): 128 hypotheses, 2 px, seed 0
inline vo_ransac_params ransac_batch_params(float threshold_px = 2.f, int n_hypotheses = 128, uint64_t seed = 0) {
  return ransac_params(threshold_px, n_hypotheses, seed);
}

//! estimate_pose_ransac for n_problems problems in DEVICE memory in one call (vo_estimate_pose_ransac_batch_dev): problem p
//! reads d_world_xyz + p * world_stride points, d_meas_uv + p * meas_stride pixels and d_n_pairs[p] (or, null, pairs_stride)
//! of the pairs at d_pairs + p * pairs_stride; its pose, pairs handed on, their count and its status (VO_POSE_RANSAC_*; 1-4:
//! the identity and every live pair) go to d_T16_out + 16 p, d_inlier_pairs + p * pairs_stride, d_n_inliers[p], d_status[p]
//! -- bit for bit vo_estimate_pose_ransac_dev on that problem alone, ready for vo_picp_solve_batch_dev.  Enqueues on the
//! default context's stream and returns; throws vo::Error on the refusals of the C call.
inline void estimate_pose_ransac_batch(const Camera& cam, int n_problems, const float* d_world_xyz, size_t world_stride, int n_world,
                                       const float* d_meas_uv, size_t meas_stride, int n_meas, const int32_t* d_pairs,
                                       size_t pairs_stride, const int* d_n_pairs, const vo_ransac_params& params, float* d_T16_out,
                                       int32_t* d_inlier_pairs, int* d_n_inliers, int* d_status, uint8_t* d_inlier_mask = nullptr,
                                       int32_t* d_hypothesis_counts = nullptr) {
  check(vo_estimate_pose_ransac_batch_dev(default_context().handle(), n_problems, cam.rows(), cam.cols(), cam.zNear(), cam.zFar(),
                                          cam.cameraMatrix().data(), d_world_xyz, world_stride, n_world, d_meas_uv, meas_stride, n_meas,
                                          d_pairs, pairs_stride, d_n_pairs, &params, d_T16_out, d_inlier_pairs, d_n_inliers,
                                          d_inlier_mask, d_hypothesis_counts, d_status),
        "estimate_pose_ransac_batch");
}

}  // namespace vo
