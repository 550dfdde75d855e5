// vo/pose_graph.hpp -- a pose graph over similarities on the GPU (voe_pose_graph, include/vo_pose_graph.h): one S = [c R | t]
// per frame (p_cam = S p_map), relative-pose edges Z_ij ~ S_j S_i^-1 with three weights each, Levenberg-Marquardt rounds whose
// damped system is solved by PCG preconditioned with the odometry chain.  The correction is carried into a map by
// DeviceMap::applyCorrection (vo/localise.hpp), the rigid pose of a corrected frame is rigid_pose(S).
#pragma once

#include <cstdint>
#include <vector>

#include "context.hpp"
#include "localise.hpp"

namespace vo {

struct PoseGraphOptions {
  int n_rounds = 8;
  int n_cg = 8;
  float cg_tol = 1e-6f;
  float lambda0 = 1e-4f;
  float huber = 0.f;
  bool with_scale = true;
  int preconditioner = VOE_POSE_GRAPH_CHAIN;
};
inline const char* pose_graph_status_name(int status) {
  static const char* names[] = {"OK", "NOT_FINITE", "NOTHING_FREE", "NO_EDGES", "NO_STEP", "COST_ROSE"};
  return status >= 0 && status < 6 ? names[status] : "?";
}

class PoseGraph {
 public:
  explicit PoseGraph(Context& ctx = default_context()) : ctx_(ctx.handle()) {}

  //! the measured Z ~ S_j S_i^-1 (camera-i coordinates to camera-j) with weights on its translation, rotation and log-scale
  void addEdge(int i, int j, const Similarity3f& Z, float w_t = 1.f, float w_r = 1.f, float w_s = 1.f) {
    edges_.push_back(i); edges_.push_back(j);
    Z_.push_back(Z);
    weights_.push_back(w_t); weights_.push_back(w_r); weights_.push_back(w_s);
  }
  //! every slot of DeviceMap::loops, in order: a slot that is not OK carries the weights 0 0 0 and is skipped by the optimiser
  void addLoops(const MapLoops& r) {
    for (size_t l = 0; l < r.Z.size(); ++l)
      addEdge(r.edges[2 * l], r.edges[2 * l + 1], r.Z[l], r.weights[3 * l], r.weights[3 * l + 1], r.weights[3 * l + 2]);
  }
  size_t edges() const { return Z_.size(); }
  void clear() { edges_.clear(); Z_.clear(); weights_.clear(); }

  //! S in place; fixed: one byte per frame (or empty: none held).  *edge_status: VOE_POSE_GRAPH_EDGE_* per edge; *edge_cost: s^2 of
  //! every live edge at the state S holds afterwards (a false loop has the largest); *rounds: one record per round.
  voe_pose_graph_stats optimise(std::vector<Similarity3f>& S, const std::vector<uint8_t>& fixed = {}, const PoseGraphOptions& opt = PoseGraphOptions(),
                                std::vector<int32_t>* edge_status = nullptr, std::vector<double>* edge_cost = nullptr,
                                std::vector<voe_pose_graph_round>* rounds = nullptr) const {
    if (!fixed.empty() && fixed.size() != S.size()) throw Error(VO_ERR_INVALID_ARG, "PoseGraph::optimise: one byte per frame in `fixed`");
    const size_t E = Z_.size();
    std::vector<int32_t> es(E + 1, 0);
    std::vector<double> ec(E + 1, 0.0);
    std::vector<voe_pose_graph_round> rd((size_t)(opt.n_rounds > 0 ? opt.n_rounds : 0) + 1);
    const voe_pose_graph_params prm{opt.n_rounds, opt.n_cg, opt.cg_tol, opt.lambda0, opt.huber, opt.with_scale ? 1 : 0, opt.preconditioner};
    voe_pose_graph_stats st{};
    check(voe_pose_graph(ctx_, (int)S.size(), S.empty() ? nullptr : S[0].m, (int)E, E ? edges_.data() : nullptr, E ? Z_[0].m : nullptr,
                         E ? weights_.data() : nullptr, fixed.empty() ? nullptr : fixed.data(), &prm, es.data(), ec.data(), rd.data(), &st),
          "voe_pose_graph");
    es.resize(E); ec.resize(E); rd.resize((size_t)(opt.n_rounds > 0 ? opt.n_rounds : 0));
    if (edge_status) *edge_status = es;
    if (edge_cost) *edge_cost = ec;
    if (rounds) *rounds = rd;
    return st;
  }

 private:
  vo_ctx* ctx_;
  std::vector<int32_t> edges_;
  std::vector<Similarity3f> Z_;
  std::vector<float> weights_;
};

}  // namespace vo
