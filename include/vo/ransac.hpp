// vo/ransac.hpp -- estimate_transform behind RANSAC (vo_estimate_transform_ransac): an extension of the facade, not a
// reference interface.  n_hypotheses minimal 8-point fits are scored by Sampson distance on the GPU; the pose is the
// plain GPU estimate_transform of the best hypothesis's inliers (bit for bit vo_estimate_transform of those pairs).
#pragma once

#include <cstdint>
#include <vector>

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

}  // namespace vo
