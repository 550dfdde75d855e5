// map_pose_refine.hip -- motion-only adjustment on the map's cost (vo_map_refine_poses*): the points are fixed, every frame's
// pose is re-estimated from ALL its rows that hit an entry.  The rules are those of include/vo_map_adjust.h; in short:
//   observation   a live row (frame f, position i) whose lookup returns entry e; consumed in ascending i; the point is the
//                 entry's float32 point widened to double
//   cost          rho(proj(K, T p) - uv), |e|^2 or Huber by IRLS -- the cost of vo_map_refine, term for term
//   round         H = sum w J^T J + damping I, b = sum w J^T e, dx = -H^-1 b (6x6 LDL^T in natural order), T <- v2t(dx) T,
//                 everything in double; T is rounded to float32 once, after the last round
// Launches behind the lookup (which wrote the entry of every query position):
//   map_pose_refine_kernel    ONE WORKGROUP PER FRAME, all rounds in this one launch: the pose never leaves the workgroup.  The
//                             rows are strided over the 256 threads (thread t takes the rows t, t + 256, ... in that order); the
//                             28 sums are reduced in double by frame_reduce (vo_internal.h; map_bundle.hip uses the same):
//                             the fixed DPP tree inside every row of 16 lanes, the 16 row sums through LDS, added in row order
//                             (thread k < 28 adds term k), the 28 totals back through LDS, so that all 256 threads hold the
//                             same bits and run the 6x6 solve and the pose update redundantly.  No scratch; two barriers per
//                             round, the second of which also gathers the "behind" flags
//   map_pose_stats_kernel     one workgroup: status census and the two cost sums in a fixed order (status_census)
// The observation is vo_math.h's map_pose_term on map_obs, the one model of the four adjustment files.
// A single frame therefore runs on one compute unit; the call fills the device from about 256 frames on.
#include "vo_internal.h"

namespace vo {

constexpr int PB = 256;                   // threads per workgroup
constexpr int PROWS = PB / 16;            // DPP rows per workgroup
static_assert(PB == MAP_WG, "frame_reduce (vo_internal.h) counts on this size");
constexpr int PSTAT = 1024;               // threads of the statistics workgroup

enum { PS_OK = 0, PS_FIXED = 1, PS_FEW_OBS = 2, PS_BEHIND = 3, PS_NOT_FINITE = 4, PS_COST_ROSE = 5 };

__global__ __launch_bounds__(PB) void map_pose_refine_kernel(MapPoseArgs a) {
  __shared__ double s_row[PROWS][NPOSE], s_tot[NPOSE];
  __shared__ int s_n;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int M = a.v.size(), n_max = a.v.n_max;
  const int32_t* ent = a.ent + (size_t)f * n_max;
  const float2* uv = reinterpret_cast<const float2*>(a.v.uv) + (size_t)f * a.v.uv_stride;
  if (tid == 0) s_n = 0;
  const float* T0 = a.v.T16 + 16 * (size_t)f;                // the frame's 64 bytes as they came (nobody else writes them)
  double T[12];                                              // R column-major, then t
  float Tf[12];
  a.v.load_pose(f, Tf);
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = (double)Tf[k];
  double K[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = a.v.K[k];
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < n_max; i += PB) { const int e = ent[i]; mine += e >= 0 && e < M; }
  if (mine) atomicAdd(&s_n, mine);                           // (an integer count does not depend on the order)
  __syncthreads();
  const int n = s_n;
  const bool fixed = a.fixed && a.fixed[f] != 0;
  bool run = !fixed && n >= a.min_obs;                       // (uniform in the workgroup, as everything below: every thread holds the same sums)
  bool not_finite = false, behind = false;
  double cost0 = 0.0, cost1 = 0.0;
  for (int r = 0; r <= a.n_rounds && run; ++r) {              // (run is uniform: a frame that stopped leaves the loop as one)
    double acc[NPOSE];
#pragma unroll
    for (int k = 0; k < NPOSE; ++k) acc[k] = 0.0;
    bool bh = false;
    if (run) {
      for (int i = tid; i < n_max; i += PB) {
        const int e = ent[i];
        if (e < 0 || e >= M) continue;
        const float pt[3] = {a.v.pts[3 * (size_t)e], a.v.pts[3 * (size_t)e + 1], a.v.pts[3 * (size_t)e + 2]};
        const float2 m = uv[i];
        bh |= !map_pose_term(K, T, pt, (double)m.x, (double)m.y, a.huber, acc);
      }
    }
    const bool any_behind = frame_reduce<NPOSE, NPOSE, true>(acc, s_row, s_tot, bh);      // every thread holds the same bits from here on
    if (run) {
      bool finite = true;
#pragma unroll
      for (int k = 0; k < NPOSE; ++k) finite &= refine_finite(acc[k]);
      if (!finite) {
        not_finite = true; run = false;
      } else {
        behind |= any_behind;
        if (r == 0) cost0 = acc[27];
        if (r == a.n_rounds) {
          cost1 = acc[27];
        } else {
          const int diag[6] = {0, 6, 11, 15, 18, 20};
#pragma unroll
          for (int k = 0; k < 6; ++k) acc[diag[k]] += a.damping;
          double x[6];
          if (!ldlt6d_solve(acc, acc + 21, x)) {
            not_finite = true; run = false;
          } else {
            if (a.H_out && tid == 0) {                        // the damped H of the last solved round stays
              double* h = a.H_out + 36 * (size_t)f;
              int k = 0;
#pragma unroll
              for (int rr = 0; rr < 6; ++rr)
#pragma unroll
                for (int c = rr; c < 6; ++c) { h[rr + 6 * c] = acc[k]; h[c + 6 * rr] = acc[k]; ++k; }
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) x[k] = -x[k];
            pose_apply_v2t(x, T);
            if (r == a.n_rounds - 1) {                       // rounded once: the cost that decides is the stored pose's
#pragma unroll
              for (int k = 0; k < 12; ++k) { Tf[k] = (float)T[k]; T[k] = (double)Tf[k]; }
            }
            bool ok = true;
#pragma unroll
            for (int k = 0; k < 12; ++k) ok &= refine_finite(T[k]);
            if (!ok) { not_finite = true; run = false; }
          }
        }
      }
    }
  }
  if (tid == 0) {
    int status = PS_OK;
    if (fixed) status = PS_FIXED;
    else if (n < a.min_obs) status = PS_FEW_OBS;
    else if (not_finite) status = PS_NOT_FINITE;
    else if (behind) status = PS_BEHIND;
    else if (cost1 > cost0) status = PS_COST_ROSE;
    const bool replace = status == PS_OK && a.n_rounds > 0;
    a.status[f] = status;
    a.n_obs[f] = n;
    a.cost[2 * (size_t)f] = cost0;
    a.cost[2 * (size_t)f + 1] = cost1;
    float* o = a.T_out + 16 * (size_t)f;
    if (replace) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        o[4 * c] = Tf[3 * c]; o[4 * c + 1] = Tf[3 * c + 1]; o[4 * c + 2] = Tf[3 * c + 2];
        o[4 * c + 3] = c == 3 ? 1.f : 0.f;
      }
    } else if (a.T_out != a.v.T16) {                          // as 32-bit words: a NaN keeps its payload
      const unsigned* src = reinterpret_cast<const unsigned*>(T0);
#pragma unroll
      for (int k = 0; k < 16; ++k) reinterpret_cast<unsigned*>(o)[k] = src[k];
    }
  }
}

// vo_map_pose_refine_stats: int32 n_frames, n_obs, by_status[6]; double cost_before, cost_after (status_census, vo_internal.h)
__global__ __launch_bounds__(PSTAT) void map_pose_stats_kernel(MapPoseArgs a) {
  status_census<PSTAT, true>(a.v.n_frames, a.status, a.cost, a.n_obs, nullptr, a.stats);
}

MapPoseWs map_pose_layout(void* base, int n_frames, int n_max, bool with_lookup) {
  MapPoseWs w{};
  WsCarver c(base);
  const size_t rows = (size_t)n_frames * (size_t)n_max, F = (size_t)n_frames;
  if (with_lookup) {
    w.ent = c.take<int32_t>(4 * (rows ? rows : 1));
    w.pairs = c.take<int32_t>(8 * (rows ? rows : 1));
    w.n_hits = c.take<int>(4 * F);
  }
  w.status = c.take<int32_t>(4 * F);
  w.n_obs = c.take<int>(4 * F);
  w.cost = c.take<double>(16 * F);
  w.bytes = c.bytes;
  return w;
}

hipError_t launch_map_pose_refine(hipStream_t st, const MapPoseArgs& a) {
  hipLaunchKernelGGL(map_pose_refine_kernel, dim3(a.v.n_frames), dim3(PB), 0, st, a);
  hipLaunchKernelGGL(map_pose_stats_kernel, dim3(1), dim3(PSTAT), 0, st, a);
  return hipGetLastError();
}

}  // namespace vo
