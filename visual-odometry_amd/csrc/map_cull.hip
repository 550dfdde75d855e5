// map_cull.hip -- landmarks taken out of the device map (voe_map_cull*): every entry is scored from ALL the rows of n_frames
// frames that see it, the survivors are compacted in order, the table is rebuilt.  The rules are those of
// include/vo_map_cull.h.  An observation is vo_math.h's map_obs, the one model of the four adjustment files; the view of the map
// and the frames, the row helpers and the landmark kernels' grid are vo_internal.h's, the scans vo_math.h's.  Launches behind the
// lookup (which wrote the entry of every query position) and behind the ordered observation lists of map_refine.hip
// (launch_map_refine_lists, unchanged):
//   cull_score_kernel      16 lanes per landmark, the passes by map_score.h's score_list (shared with map_grow.hip).  Pass 1 strides the ordered list over the lanes (observation k in lane
//                          k mod 16): the sum of |e|^2 by the fixed DPP tree of refine_row_sum, the extrema (refine_row_max /
//                          _min) and the frame changes by the same four row steps.  Pass 2 (only with the parallax test on)
//                          visits the pairs in tiles of 16 x 16: a lane holds the unit ray of one observation of tile A and one of tile B, tile B's
//                          rays and their list positions go round the DPP row (row_ror:1, 16 steps), every lane keeps the
//                          minimum of its dot products, the 16 lanes are reduced by a row minimum.  The rays are ALWAYS
//                          recomputed from the keys -- once per lane and tile pair, 16 pairs of dot products each -- so there
//                          is no list length at which the path changes, no LDS and no scratch.  A minimum is exact in any
//                          order: the dealing of the pairs cannot show in the bits.
//   cull_count_kernel      survivors per block of 256 entries, and every survivor's rank inside its block
//   cull_scan_kernel       one workgroup: the block counts -> block offsets, 1024 at a time with a carry (any number of
//                          blocks); the control words: size before, survivors, whether the map changes
//   cull_scatter_kernel    remap of every entry; where the map changes, the survivor's 12 + 40 bytes into the STAGING area
//   cull_copy_kernel       the staging area back over the head of the arrays.  Entry j moves to r(j) <= j: compacting in
//                          place in one launch would let one workgroup write r(j') = j while another still reads j
//   cull_header_kernel     one thread: size, base and rows of the last update
//   (launch_map_rehash, guarded by the control word, enqueued by the caller)
// count .. header are also launch_map_cull_compact, which voe_map_fuse* enqueues behind keep flags of its own (map_fuse.hip)
//   cull_stats_kernel      one workgroup: an integer tally of the verdicts
// The count of launches is fixed; where nothing is dropped, or under dry_run, scatter, copy, header and rehash return at once.
#include "vo_internal.h"
#include "map_score.h"

namespace vo {

constexpr int CB = 256;                   // threads per workgroup
constexpr int CG = 16;                    // lanes per landmark: one DPP row
constexpr int CLPB = CB / CG;             // landmarks per workgroup and trip
constexpr int CSTAT = 1024;               // threads of the scan and of the statistics workgroup
static_assert(CB == MAP_WG && CG == MAP_ROW, "a landmark's lanes are one DPP row; the shared helpers of vo_internal.h count on both sizes");

struct CullEntry { int32_t verdict, n_obs, n_frames, reserved; double mean_sq, max_sq, min_z, cos_parallax; };
static_assert(sizeof(CullEntry) == 48, "voe_map_cull_entry");

__global__ __launch_bounds__(CB) void cull_score_kernel(MapCullArgs a) {
  const int M = a.v.size();
  const int lg = threadIdx.x & (CG - 1), grp = threadIdx.x / CG;
  double K[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = a.v.K[k];
  const MapScoreThr thr{a.max_mean_sq, a.max_sq, a.cos_thr, a.parallax};
  const auto load_pose = [&a](int f, float Rt[12]) { a.v.load_pose(f, Rt); };
  const int n_batches = (a.v.bound + CLPB - 1) / CLPB;
  for (int batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {      // (uniform in the workgroup: the ballot below sees whole waves)
    const int e = batch * CLPB + grp;
    const bool in = e < M;
    const int n = in ? a.l.cur[e] : 0;
    const int off = in ? a.l.offset(e) : 0;
    double p[3] = {0.0, 0.0, 0.0};
    if (in) { p[0] = (double)a.v.pts[3 * (size_t)e]; p[1] = (double)a.v.pts[3 * (size_t)e + 1]; p[2] = (double)a.v.pts[3 * (size_t)e + 2]; }
    // the statistics and the four tests: map_score.h, shared with map_grow.hip
    const MapScore sc = score_list(a.v, load_pose, K, p, a.l.keys + off, n, a.parallax != 0, lg);
    if (in && lg == 0) {
      double mean, cosp;
      const int judged = score_judge(sc, n, thr, mean, cosp);
      const double mx = sc.mx, mz = n == 0 ? 0.0 : sc.mz;
      const int n_fr = sc.n_fr;
      int v = judged;
      if (n == 0) v = CV_UNSEEN;
      else if (n < a.min_obs) v = CV_FEW_OBS;
      else if (n_fr < a.min_frames) v = CV_FEW_FRAMES;
      a.verdict[e] = v;
      a.w.rank[e] = (v == CV_KEPT || (v == CV_UNSEEN && !a.drop_unseen)) ? 1 : 0;
      if (a.entry_out) {
        CullEntry r;
        r.verdict = v; r.n_obs = n; r.n_frames = n_fr; r.reserved = 0;
        r.mean_sq = mean; r.max_sq = mx; r.min_z = mz; r.cos_parallax = cosp;
        static_cast<CullEntry*>(a.entry_out)[e] = r;
      }
    }
  }
}

__global__ __launch_bounds__(CB) void cull_count_kernel(MapCullArgs a) {
  __shared__ int s_wave[CB / 64];
  const int M = a.v.size();
  const int e = blockIdx.x * CB + threadIdx.x;
  const int v = e < M ? a.w.rank[e] : 0;
  int tot;
  const int x = block_exclusive_scan<CB>(v, s_wave, tot);
  if (e < M) a.w.rank[e] = v ? x : -1;
  if (threadIdx.x == 0) a.w.blk[blockIdx.x] = tot;
}

__global__ __launch_bounds__(CSTAT) void cull_scan_kernel(MapCullArgs a, int nb) {
  __shared__ int s_w[CSTAT / 64];
  __shared__ int s_carry;
  const int kept = scan_with_carry<CSTAT>(a.w.blk, nb, s_w, &s_carry);
  if (threadIdx.x == 0) {
    const int M = a.v.size();
    a.w.ctl[0] = M; a.w.ctl[1] = kept; a.w.ctl[2] = (kept != M && !a.dry_run) ? 1 : 0;
  }
}

__global__ __launch_bounds__(CB) void cull_scatter_kernel(MapCullArgs a) {
  const int M = a.w.ctl[0];
  const int e = blockIdx.x * CB + threadIdx.x;
  if (e >= M) return;
  const int r = a.w.rank[e];
  const int to = r >= 0 ? a.w.blk[blockIdx.x] + r : -1;
  a.remap[e] = to;
  if (to < 0 || a.w.ctl[2] == 0) return;
  a.w.stage_pts[3 * (size_t)to] = a.v.pts[3 * (size_t)e];
  a.w.stage_pts[3 * (size_t)to + 1] = a.v.pts[3 * (size_t)e + 1];
  a.w.stage_pts[3 * (size_t)to + 2] = a.v.pts[3 * (size_t)e + 2];
  const float2* src = reinterpret_cast<const float2*>(a.app) + 5 * (size_t)e;
  float2* dst = reinterpret_cast<float2*>(a.w.stage_app) + 5 * (size_t)to;
#pragma unroll
  for (int k = 0; k < 5; ++k) dst[k] = src[k];
}

__global__ __launch_bounds__(CB) void cull_copy_kernel(MapCullArgs a) {
  if (a.w.ctl[2] == 0) return;
  const int j = blockIdx.x * CB + threadIdx.x;
  if (j >= a.w.ctl[1]) return;
  a.v.pts[3 * (size_t)j] = a.w.stage_pts[3 * (size_t)j];
  a.v.pts[3 * (size_t)j + 1] = a.w.stage_pts[3 * (size_t)j + 1];
  a.v.pts[3 * (size_t)j + 2] = a.w.stage_pts[3 * (size_t)j + 2];
  const float2* src = reinterpret_cast<const float2*>(a.w.stage_app) + 5 * (size_t)j;
  float2* dst = reinterpret_cast<float2*>(a.app) + 5 * (size_t)j;
#pragma unroll
  for (int k = 0; k < 5; ++k) dst[k] = src[k];
}

__global__ void cull_header_kernel(MapCullArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || a.w.ctl[2] == 0) return;
  a.v.hdr[0] = a.w.ctl[1];          // the size
  a.v.hdr[1] = a.w.ctl[1];          // base of the last update: there is none
  a.v.hdr[2] = 0;                   // its rows
}

// voe_map_cull_stats: int32 status, n_before, n_kept, n_obs, by_verdict[8].  Whole numbers: any order gives the same tally.
__global__ __launch_bounds__(CSTAT) void cull_stats_kernel(MapCullArgs a) {
  __shared__ int s_n[8];
  const int M = a.w.ctl[0];
  if (threadIdx.x < 8) s_n[threadIdx.x] = 0;
  __syncthreads();
  int n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int e = threadIdx.x; e < M; e += CSTAT) {
    const int v = a.verdict[e];
#pragma unroll
    for (int k = 0; k < 8; ++k) n[k] += v == k;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) if (n[k]) atomicAdd(&s_n[k], n[k]);
  __syncthreads();
  if (threadIdx.x == 0) {
    int* si = static_cast<int*>(a.stats);
    si[0] = a.w.ctl[1] != M ? 0 : 1;
    si[1] = M; si[2] = a.w.ctl[1]; si[3] = *a.l.total;
    for (int k = 0; k < 8; ++k) si[4 + k] = s_n[k];
  }
}

MapCullWs map_cull_layout(void* base, int bound) {
  MapCullWs w{};
  WsCarver c(base);
  const size_t B = (size_t)(bound > 0 ? bound : 1);
  w.verdict = c.take<int32_t>(4 * B);
  w.remap = c.take<int32_t>(4 * B);
  w.rank = c.take<int>(4 * B);
  w.blk = c.take<int>(4 * ((B + CB - 1) / CB));
  w.stage_pts = c.take<float>(12 * B);
  w.stage_app = c.take<float>(40 * B);
  w.ctl = c.take<int>(16);
  w.bytes = c.bytes;
  return w;
}

hipError_t launch_map_cull(hipStream_t st, const MapCullArgs& a, int n_cu) {
  const hipError_t e = launch_map_refine_lists(st, a.l, a.v.n_frames, a.v.n_max, a.v.bound);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cull_score_kernel, dim3(landmark_grid(a.v.bound, n_cu)), dim3(CB), 0, st, a);
  return launch_map_cull_compact(st, a);
}

// the compaction behind the keep flags in w.rank: what voe_map_fuse* shares with the cull, kernel for kernel
hipError_t launch_map_cull_compact(hipStream_t st, const MapCullArgs& a) {
  const int B = a.v.bound > 0 ? a.v.bound : 1;
  const int nb = (B + CB - 1) / CB;
  hipLaunchKernelGGL(cull_count_kernel, dim3(nb), dim3(CB), 0, st, a);
  hipLaunchKernelGGL(cull_scan_kernel, dim3(1), dim3(CSTAT), 0, st, a, nb);
  hipLaunchKernelGGL(cull_scatter_kernel, dim3(nb), dim3(CB), 0, st, a);
  hipLaunchKernelGGL(cull_copy_kernel, dim3(nb), dim3(CB), 0, st, a);
  hipLaunchKernelGGL(cull_header_kernel, dim3(1), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_cull_stats(hipStream_t st, const MapCullArgs& a) {
  hipLaunchKernelGGL(cull_stats_kernel, dim3(1), dim3(CSTAT), 0, st, a);
  return hipGetLastError();
}

}  // namespace vo
