// map_refine.hip -- structure-only adjustment of the device map (vo_map_refine*): the poses are fixed, every landmark is
// re-estimated from ALL the rows of n_frames frames that see it.  The rules are those of include/vo_hip.h; in short:
//   observation   a live row (frame f, position i) whose lookup returns entry e; key f * n_max + i; consumed in ascending key order
//   cost          rho(proj(K, T_f p) - uv), |e|^2 or Huber by IRLS; the only gate is camera z > 0, and it is a status, not a weight
//   round         H = sum w J^T J + damping I, b = sum w J^T e, p <- p - H^-1 b (LDL^T in natural order), everything in double
// Launches behind the lookup (which wrote the entry of every query position):
//   memset                          counts and cursors of the entries
//   map_refine_count_kernel         observations per entry (integer atomics: a count does not depend on the order)
//   map_refine_offsets_kernel       exclusive scan inside every block of 256 entries + the block's total
//   scan_counts_kernel              (geom.hip) the block totals -> block offsets, the number of observations
//   map_refine_scatter_kernel       every observation's key into its entry's segment, at a cursor drawn by an atomic: the
//                                   ORDER inside a segment depends on scheduling, the SET does not
//   map_refine_order_kernel         one thread per scattered key: its rank among its segment's keys (they are distinct) is
//                                   its place in the ordered segment -- a function of the data alone from here on
//   map_refine_kernel               16 lanes per landmark, all rounds in this one launch: observations strided over the lanes,
//                                   the 10 sums reduced in double by a fixed DPP tree inside the 16 lanes (every lane ends
//                                   with the same bits), the 3x3 solve done redundantly by the 16
//   map_refine_stats_kernel         one workgroup: status census and the two cost sums in a fixed order, no float atomics
// Per-observation terms are evaluated in DOUBLE (vo_math.h: map_refine_term on map_obs, the one observation model of the four
// adjustment files): DESIGN.md section 4.13 says why.  Shared with them (vo_internal.h): the view of the map and the frames
// (MapView: size, load_pose, decode), the list offset (MapRefineWs::offset), the row helpers (refine_row_sum / _any), the
// census (status_census), the landmark kernels' grid (landmark_grid); the block scan is vo_math.h's block_exclusive_scan.
#include "vo_internal.h"

namespace vo {

constexpr int RB = 256;                   // threads per workgroup
constexpr int RG = 16;                    // lanes per landmark
constexpr int RLPB = RB / RG;             // landmarks per workgroup and trip
constexpr int REFINE_LDS_FRAMES = 512;    // poses staged in LDS up to here (12 floats each: 24 KiB), read through L2 beyond
constexpr int RSTAT = 1024;               // threads of the statistics workgroup

enum { ST_OK = 0, ST_UNSEEN = 1, ST_FEW_OBS = 2, ST_BEHIND = 3, ST_NOT_FINITE = 4, ST_COST_ROSE = 5 };

// the list kernels read the workspace alone: rows = n_frames * n_max positions, entries below bound
__global__ __launch_bounds__(RB) void map_refine_count_kernel(MapRefineWs w, size_t rows, int bound) {
  const size_t k = (size_t)blockIdx.x * RB + threadIdx.x;
  if (k >= rows) return;
  const int e = w.ent[k];
  if (e >= 0 && e < bound) atomicAdd(&w.cnt[e], 1);
}

__global__ __launch_bounds__(RB) void map_refine_offsets_kernel(MapRefineWs w, int bound) {
  __shared__ int s_wave[RB / 64];
  const int e = blockIdx.x * RB + threadIdx.x;
  int tot;
  const int x = block_exclusive_scan<RB>(e < bound ? w.cnt[e] : 0, s_wave, tot);
  if (e < bound) w.cnt[e] = x;
  if (threadIdx.x == 0) w.blk[blockIdx.x] = tot;
}

__global__ __launch_bounds__(RB) void map_refine_scatter_kernel(MapRefineWs w, size_t rows, int bound) {
  const size_t k = (size_t)blockIdx.x * RB + threadIdx.x;
  if (k >= rows) return;
  const int e = w.ent[k];
  if (e < 0 || e >= bound) return;
  const int at = atomicAdd(&w.cur[e], 1);
  const size_t o = (size_t)w.offset(e) + at;
  if (o < rows) w.tmp[o] = (int)k;                           // (always: the segments partition the observations)
}

__global__ __launch_bounds__(RB) void map_refine_order_kernel(MapRefineWs w, size_t rows, int bound) {
  const int total = *w.total;
  const size_t s = (size_t)blockIdx.x * RB + threadIdx.x;
  if (s >= rows || s >= (size_t)total) return;
  const int key = w.tmp[s];
  if (key < 0 || (size_t)key >= rows) return;
  const int e = w.ent[key];
  if (e < 0 || e >= bound) return;
  const int off = w.offset(e), n = w.cur[e];
  int rank = 0;
  for (int j = 0; j < n; ++j) rank += w.tmp[off + j] < key;
  w.keys[off + rank] = key;
}

static_assert(RB == MAP_WG && RG == MAP_ROW, "a landmark's lanes are one DPP row; the shared helpers of vo_internal.h count on both sizes");

template <bool LDS>
__global__ __launch_bounds__(RB) void map_refine_kernel(MapRefineArgs a) {
  __shared__ float s_pose[LDS ? REFINE_LDS_FRAMES * 12 : 12];
  if (LDS) {
    for (int k = threadIdx.x; k < a.v.n_frames * 12; k += RB) s_pose[k] = a.v.pose_at(k / 12, k % 12);
    __syncthreads();
  }
  const int M = a.v.size();
  const int lg = threadIdx.x & (RG - 1), grp = threadIdx.x / RG;
  double K[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = a.v.K[k];
  const int n_batches = (a.v.bound + RLPB - 1) / RLPB;
  for (int batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {      // (uniform in the workgroup: the shuffles below see whole waves)
    const int e = batch * RLPB + grp;
    const bool in = e < M;
    const int n = in ? a.w.cur[e] : 0;
    const int off = in ? a.w.offset(e) : 0;
    float p0[3] = {0.f, 0.f, 0.f};
    if (in) { p0[0] = a.v.pts[3 * (size_t)e]; p0[1] = a.v.pts[3 * (size_t)e + 1]; p0[2] = a.v.pts[3 * (size_t)e + 2]; }
    double p[3] = {(double)p0[0], (double)p0[1], (double)p0[2]};
    float pf[3] = {p0[0], p0[1], p0[2]};
    bool run = in && n >= a.min_obs;                         // (min_obs >= 2: an unseen entry does not run either)
    bool not_finite = false, behind = false;
    double cost0 = 0.0, cost1 = 0.0;
    for (int r = 0; r <= a.n_rounds; ++r) {
      double acc[NREF];
#pragma unroll
      for (int k = 0; k < NREF; ++k) acc[k] = 0.0;
      bool bh = false;
      if (run) {
        for (int j = lg; j < n; j += RG) {
          float2 m;
          const int f = a.v.decode(a.w.keys[off + j], m);
          float Rt[12];
          if (LDS) {
#pragma unroll
            for (int k = 0; k < 12; ++k) Rt[k] = s_pose[12 * f + k];
          } else {
            a.v.load_pose(f, Rt);
          }
          bh |= !map_refine_term(K, Rt, p, (double)m.x, (double)m.y, a.huber, acc);
        }
      }
#pragma unroll
      for (int k = 0; k < NREF; ++k) acc[k] = refine_row_sum(acc[k]);
      const bool any_behind = refine_row_any(bh);
      if (run) {
        bool finite = true;
#pragma unroll
        for (int k = 0; k < NREF; ++k) finite &= refine_finite(acc[k]);
        if (!finite) {
          not_finite = true; run = false;
        } else {
          behind |= any_behind;
          if (r == 0) cost0 = acc[9];
          if (r == a.n_rounds) {
            cost1 = acc[9];
          } else {
            const double H[6] = {acc[0] + a.damping, acc[1], acc[2], acc[3] + a.damping, acc[4], acc[5] + a.damping};
            double x[3];
            if (!ldlt3_solve(H, acc + 6, x)) {
              not_finite = true; run = false;
            } else {
              p[0] -= x[0]; p[1] -= x[1]; p[2] -= x[2];
              if (r == a.n_rounds - 1) {                     // rounded once: the cost that decides is the stored point's
                pf[0] = (float)p[0]; pf[1] = (float)p[1]; pf[2] = (float)p[2];
                p[0] = (double)pf[0]; p[1] = (double)pf[1]; p[2] = (double)pf[2];
              }
              if (!(refine_finite(p[0]) && refine_finite(p[1]) && refine_finite(p[2]))) { not_finite = true; run = false; }
            }
          }
        }
      }
    }
    if (in && lg == 0) {
      int status = ST_OK;
      if (n == 0) status = ST_UNSEEN;
      else if (n < a.min_obs) status = ST_FEW_OBS;
      else if (not_finite) status = ST_NOT_FINITE;
      else if (behind) status = ST_BEHIND;
      else if (cost1 > cost0) status = ST_COST_ROSE;
      const bool replace = status == ST_OK && a.n_rounds > 0;
      a.status[e] = status;
      a.w.cost[2 * (size_t)e] = cost0;
      a.w.cost[2 * (size_t)e + 1] = cost1;
      if (a.xyz_out) {
        float* o = a.xyz_out + 3 * (size_t)e;
        o[0] = replace ? pf[0] : p0[0]; o[1] = replace ? pf[1] : p0[1]; o[2] = replace ? pf[2] : p0[2];
      } else if (replace) {
        float* o = a.v.pts + 3 * (size_t)e;
        o[0] = pf[0]; o[1] = pf[1]; o[2] = pf[2];
      }
    }
  }
}

// vo_map_refine_stats: int32 n_entries, n_obs, by_status[6]; double cost_before, cost_after (status_census, vo_internal.h)
__global__ __launch_bounds__(RSTAT) void map_refine_stats_kernel(MapRefineArgs a) {
  status_census<RSTAT, false>(a.v.size(), a.status, a.w.cost, nullptr, a.w.total, a.stats);
}

MapRefineWs map_refine_layout(void* base, int n_frames, int n_max, int bound) {
  MapRefineWs w{};
  WsCarver c(base);
  const size_t rows = (size_t)n_frames * (size_t)n_max, B = (size_t)(bound > 0 ? bound : 1);
  w.ent = c.take<int32_t>(4 * (rows ? rows : 1));
  w.pairs = c.take<int32_t>(8 * (rows ? rows : 1));
  w.tmp = reinterpret_cast<int*>(w.pairs);
  w.keys = w.pairs ? reinterpret_cast<int*>(w.pairs) + rows : nullptr;
  w.n_hits = c.take<int>(4 * (size_t)n_frames);
  w.cnt = c.take<int>(8 * B);
  w.cur = w.cnt ? w.cnt + B : nullptr;
  w.blk = c.take<int>(4 * ((B + RB - 1) / RB));
  w.total = c.take<int>(4);
  w.status = c.take<int32_t>(4 * B);
  w.cost = c.take<double>(16 * B);
  w.bytes = c.bytes;
  return w;
}

hipError_t launch_map_refine_lists(hipStream_t st, const MapRefineWs& w, int n_frames, int n_max, int bound) {
  const size_t rows = (size_t)n_frames * (size_t)n_max, B = (size_t)(bound > 0 ? bound : 1);
  const int nbE = (int)((B + RB - 1) / RB);
  hipError_t e = hipMemsetAsync(w.cnt, 0, sizeof(int) * 2 * B, st);
  if (e != hipSuccess) return e;
  const unsigned row_blocks = (unsigned)((rows + RB - 1) / RB);
  if (rows) hipLaunchKernelGGL(map_refine_count_kernel, dim3(row_blocks), dim3(RB), 0, st, w, rows, bound);
  hipLaunchKernelGGL(map_refine_offsets_kernel, dim3(nbE), dim3(RB), 0, st, w, bound);
  e = launch_scan(st, w.blk, nbE, w.total);
  if (e != hipSuccess) return e;
  if (rows) {
    hipLaunchKernelGGL(map_refine_scatter_kernel, dim3(row_blocks), dim3(RB), 0, st, w, rows, bound);
    hipLaunchKernelGGL(map_refine_order_kernel, dim3(row_blocks), dim3(RB), 0, st, w, rows, bound);
  }
  return hipGetLastError();
}

hipError_t launch_map_refine(hipStream_t st, const MapRefineArgs& a, int n_cu) {
  const hipError_t e = launch_map_refine_lists(st, a.w, a.v.n_frames, a.v.n_max, a.v.bound);
  if (e != hipSuccess) return e;
  if (a.v.bound > 0) {
    // (102 VGPRs leave the 4 waves per SIMD landmark_grid counts on, and 4 x 24 KiB of LDS fit as well)
    const dim3 grid(landmark_grid(a.v.bound, n_cu));
    if (a.v.n_frames <= REFINE_LDS_FRAMES) hipLaunchKernelGGL(map_refine_kernel<true>, grid, dim3(RB), 0, st, a);
    else hipLaunchKernelGGL(map_refine_kernel<false>, grid, dim3(RB), 0, st, a);
  }
  hipLaunchKernelGGL(map_refine_stats_kernel, dim3(1), dim3(RSTAT), 0, st, a);
  return hipGetLastError();
}

}  // namespace vo
