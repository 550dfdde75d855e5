// vo/refine.hpp -- non-linear refit of the relative pose of two views (vo_refine_transform): an extension of the facade,
// not a reference interface.  Plain Gauss-Newton on the Sampson error of the 2D-2D pairs, 5 parameters (rotation,
// translation direction; |t| is kept), the sums on the GPU in double; include/vo_hip.h has the definition.
#pragma once

#include <cstdint>
#include <vector>

#include "context.hpp"
#include "utils.hpp"

namespace vo {

//! defaults of apps/vo_complete --refine-init: 10 rounds, Huber weight at 1 px (0: none)
inline vo_epi_refine_params refine_params(int n_rounds = 10, float huber_px = 1.f) {
  vo_epi_refine_params p;
  p.n_rounds = n_rounds; p.huber_px = huber_px;
  return p;
}

//! X (p_cur = X p_ref, e.g. from estimate_transform[_ransac]) refined over the correspondences (ref_idx, cur_idx); with
//! *inliers (one 0/1 per correspondence) only the marked ones take part, at their positions.  A refit that is not accepted
//! (*stats, if given, says why: VO_EPI_REFINE_*) returns X itself.  Throws vo::Error on bad parameters.
inline Isometry3f refine_transform(const Matrix3f& k, const IntPairVector& correspondences, const Vector2fVector& p1_img,
                                   const Vector2fVector& p2_img, const Isometry3f& X, const vo_epi_refine_params& params,
                                   const std::vector<uint8_t>* inliers = nullptr, vo_epi_refine_stats* stats = nullptr) {
  const int n = (int)correspondences.size();
  if (inliers && inliers->size() != correspondences.size())
    throw Error(VO_ERR_INVALID_ARG, "refine_transform: one inlier flag per correspondence");
  Isometry3f out = X;
  vo_epi_refine_stats s;
  check(vo_refine_transform(default_context().handle(), k.data(), n ? pair_data(correspondences) : nullptr, n,
                            inliers && n ? inliers->data() : nullptr, detail::ptr(p1_img), (int)p1_img.size(), detail::ptr(p2_img),
                            (int)p2_img.size(), X.data(), &params, out.data(), &s),
        "refine_transform");
  if (stats) *stats = s;
  return out;
}

}  // namespace vo
