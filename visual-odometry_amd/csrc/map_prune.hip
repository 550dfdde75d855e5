// map_prune.hip -- single observations taken out of their frames (voe_map_prune*): every observation of every landmark is judged
// on its own reprojection error and camera depth, against the other rows of its frame on the same entry, and against the other
// observations of its landmark; two guards keep the rows of a landmark or of a frame that is itself at fault.  The rules are those
// of include/vo_hip.h (PRUNE); DESIGN.md section 4.27.  The map, its table and its header are only read.  An observation's terms
// are map_score.h's score_obs -- the device function of voe_map_cull, hence its bits --, the integer decisions prune_rules.h's.
// Launches behind the lookup (which wrote the entry of every query position), behind the ordered observation lists of
// map_refine.hip (launch_map_refine_lists, unchanged) and behind a memset of the statistics:
//   prune_landmark_kernel   16 lanes per landmark, landmark_grid's striding.  Pass 1 holds observation k in lane k mod 16:
//                           score_obs once per observation, rule 3.  A list of <= 16 observations stays in registers; a longer
//                           one puts |e|^2 and the status in LIST order into the workspace, and no later pass projects again.
//                           Rule 4 is a scan over the run of equal key / n_max around an observation (<= 16: the row goes round
//                           by row_ror:1 instead).  The lower median is an exact rank count over the pairs in tiles of 16 x 16,
//                           tile B going round the row as in pass 2 of score_list; (sq, list position) is the order, so ranks
//                           are distinct and exactly one observation holds the median's rank.  Then rule 6, the count of soft
//                           observations, rule 7, the provisional status (and |e|^2) at the rows' positions, the record.
//                           Two barriers per trip separate a pass that writes list slots from one that reads its neighbours'.
//   prune_frame_kernel      workgroups per frame (frame_block / frame_grid): the observations, the eligible and the soft ones of
//                           256 rows from the provisional statuses, by block counts; three integers per workgroup.
//   prune_finish_kernel     one row per lane, the same grid: every workgroup adds up its frame's partial counts (whole numbers:
//                           any order) and decides rule 8; then the final status, the entry, |e|^2 = +inf where there is no
//                           observation, the 40-byte row -- 80 B per row move here --, the frame's record, and the census: block counts
//                           per status, sixteen words per workgroup.  A soft row that its frame keeps is taken off its
//                           landmark's n_pruned by an integer atomicSub.
//   prune_stats_kernel      one workgroup: the workgroups' census words added up into the statistics.
// The sequence depends on (n_frames, n_max, bound) alone; no launch waits for another workgroup; no float atomic.
#include "vo_internal.h"
#include "map_score.h"
#include "prune_rules.h"

namespace vo {

constexpr int PB = 256;                   // threads per workgroup
constexpr int PG = 16;                    // lanes per landmark: one DPP row
constexpr int PLPB = PB / PG;             // landmarks per workgroup and trip
static_assert(PB == MAP_WG && PG == MAP_ROW, "a landmark's lanes are one DPP row; the shared helpers of vo_internal.h count on both sizes");

struct PruneLandmark { int32_t n_obs, n_el, n_soft, n_pruned, at_fault, reserved; double med_sq; };
struct PruneFrame { int32_t n_obs, n_el, n_soft, at_fault; };
static_assert(sizeof(PruneLandmark) == 32 && sizeof(PruneFrame) == 16, "voe_map_prune_landmark / voe_map_prune_frame");
// voe_map_prune_stats, word for word
enum { PST_N_FRAMES = 0, PST_N_ENTRIES = 1, PST_BY_STATUS = 2, PST_LANDMARKS_AT_FAULT = 12, PST_FRAMES_AT_FAULT = 13, PST_N_OBS = 14, PST_N_PRUNED = 15 };

// the words of a finishing workgroup's census behind the ten status counts, and the statistics workgroup
enum { PC_OBS = 10, PC_PRUNED = 11, PC_FRAME_FAULT = 12, PC_WORDS = 13 };
constexpr int PSTAT = 1024;

// a whole number below 2^31 per lane, summed over the row (exact in double)
__device__ __forceinline__ int prune_row_count(int x) { return (int)refine_row_sum((double)x); }

__global__ __launch_bounds__(PB) void prune_landmark_kernel(MapPruneArgs a) {
  const int M = a.v.size();
  const int lg = threadIdx.x & (PG - 1), grp = threadIdx.x / PG;
  const int n_max = a.v.n_max;
  double K[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = a.v.K[k];
  const auto load_pose = [&a](int f, float Rt[12]) { a.v.load_pose(f, Rt); };
  const int n_batches = (a.v.bound + PLPB - 1) / PLPB;
  int n_fault = 0;                                            // the landmarks this lane named, over its trips
  for (int batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {      // (uniform in the workgroup: the barriers below see all of it)
    const int e = batch * PLPB + grp;
    const bool in = e < M;
    const int n = in ? a.l.cur[e] : 0;
    const int off = in ? a.l.offset(e) : 0;
    const int* keys = a.l.keys + off;
    double* sqL = a.w.sq_list + off;
    int* stL = a.w.st_list + off;
    const bool big = n > PG;                                  // (the same in the 16 lanes of a row)
    const int tiles = (n + PG - 1) / PG;
    double p[3] = {0.0, 0.0, 0.0};
    if (in) { p[0] = (double)a.v.pts[3 * (size_t)e]; p[1] = (double)a.v.pts[3 * (size_t)e + 1]; p[2] = (double)a.v.pts[3 * (size_t)e + 2]; }
    // ---- pass 1: the terms, once, and rule 3 ----
    double sq0 = 0.0;                                         // the observation of this lane where n <= 16
    int st0 = PS_MISS;                                        // (no observation in this lane)
    for (int j = lg; j < n; j += PG) {
      double sq, z, u[3];
      score_obs(a.v, load_pose, K, p, keys[j], sq, z, u);
      const int st = !(refine_finite(sq) && refine_finite(z)) ? PS_NOT_FINITE : !(z > 0.0) ? PS_BEHIND : PS_KEPT;
      if (big) { sqL[j] = sq; stL[j] = st; }
      else { sq0 = sq; st0 = st; }
    }
    __syncthreads();                                          // the list slots of pass 1 are read by the row's other lanes
    // ---- rule 4: the best of a run of one frame stays ----
    // A slot changes KEPT -> DUPLICATE while neighbours read it: both mean "passed rule 3", which is all a reader asks.
    if (a.unique && n >= 2) {
      if (big) {
        for (int j = lg; j < n; j += PG) {
          if (stL[j] != PS_KEPT) continue;
          const int f = keys[j] / n_max;
          const double sq = sqL[j];
          bool dup = false;
          for (int k = j - 1; k >= 0 && keys[k] / n_max == f; --k) {
            const int s = stL[k];
            dup |= (s == PS_KEPT || s == PS_DUPLICATE) && prune_before(sqL[k], k, sq, j);
          }
          for (int k = j + 1; k < n && keys[k] / n_max == f; ++k) {
            const int s = stL[k];
            dup |= (s == PS_KEPT || s == PS_DUPLICATE) && prune_before(sqL[k], k, sq, j);
          }
          if (dup) stL[j] = PS_DUPLICATE;
        }
      } else {
        const int fa = lg < n ? keys[lg] / n_max : -1;
        double sqb = sq0;
        int fb = st0 == PS_KEPT ? fa : -1, ib = lg;         // the frame travels only with an observation that passed rule 3
        bool dup = false;
#pragma unroll
        for (int t = 0; t < PG; ++t) {
          dup |= st0 == PS_KEPT && fb == fa && ib != lg && prune_before(sqb, ib, sq0, lg);
          sqb = refine_dpp<0x121>(sqb); fb = score_ror1(fb); ib = score_ror1(ib);
        }
        if (dup) st0 = PS_DUPLICATE;
      }
    }
    __syncthreads();                                          // rule 4 has settled: KEPT now means eligible
    // ---- rule 5 ----
    int cnt = 0;
    if (big) { for (int j = lg; j < n; j += PG) cnt += stL[j] == PS_KEPT; }
    else cnt = st0 == PS_KEPT;
    const int n_el = prune_row_count(cnt);
    // ---- the lower median of the eligible |e|^2: the observation with exactly rank (n_el - 1) / 2 ----
    const bool rel = a.rel_on && n_el >= a.rel_min_obs && n_el >= 1;
    double med = 0.0;
    if (rel) {                                                // (the same in the 16 lanes of a row: the row's DPP moves see all of them)
      const int target = prune_median_rank(n_el);
      double found = -1.0;                                    // (|e|^2 >= 0)
      for (int ta = 0; ta < tiles; ++ta) {
        const int ja = ta * PG + lg;
        const bool ela = ja < n && (big ? stL[ja] : st0) == PS_KEPT;
        const double sqa = ela ? (big ? sqL[ja] : sq0) : 0.0;
        int rank = 0;
        for (int tb = 0; tb < tiles; ++tb) {
          const int jb = tb * PG + lg;
          const bool elb = jb < n && (big ? stL[jb] : st0) == PS_KEPT;
          double sqb = elb ? (big ? sqL[jb] : sq0) : 0.0;
          int ib = elb ? jb : -1;                             // the list position that travels with the value
#pragma unroll
          for (int t = 0; t < PG; ++t) {
            rank += ela && ib >= 0 && prune_before(sqb, ib, sqa, ja);
            sqb = refine_dpp<0x121>(sqb);
            ib = score_ror1(ib);
          }
        }
        if (ela && rank == target) found = sqa;
      }
      med = refine_row_max(found);
    }
    // ---- rule 6 ----
    const double rel_thr = a.rf2 * med;
    int soft = 0;
    if (big) {
      for (int j = lg; j < n; j += PG) {
        if (stL[j] != PS_KEPT) continue;
        const double sq = sqL[j];
        const int s = (a.max_sq > 0.0 && sq > a.max_sq) ? PS_HIGH_ERROR : (rel && sq > rel_thr && sq > a.floor2) ? PS_RELATIVE : PS_KEPT;
        if (s != PS_KEPT) { stL[j] = s; ++soft; }           // (read back below by this lane alone)
      }
    } else if (st0 == PS_KEPT) {
      st0 = (a.max_sq > 0.0 && sq0 > a.max_sq) ? PS_HIGH_ERROR : (rel && sq0 > rel_thr && sq0 > a.floor2) ? PS_RELATIVE : PS_KEPT;
      soft = st0 != PS_KEPT;
    }
    const int n_soft = prune_row_count(soft);
    // ---- rule 7, and the provisional status at the rows' positions ----
    const bool fault = prune_guard_fires(n_soft, n_el, a.share_landmark);
    for (int j = lg; j < n; j += PG) {
      int s = big ? stL[j] : st0;
      if (fault && prune_soft(s)) s = PS_LANDMARK_AT_FAULT;
      const int key = keys[j];
      a.w.row_st[key] = s;
      if (a.sq_out) a.sq_out[key] = big ? sqL[j] : sq0;
    }
    if (in && lg == 0) {
      if (a.landmark_out) {
        PruneLandmark r;
        r.n_obs = n; r.n_el = n_el; r.n_soft = n_soft; r.n_pruned = (n - n_el) + (fault ? 0 : n_soft); r.at_fault = fault; r.reserved = 0;
        r.med_sq = med;
        static_cast<PruneLandmark*>(a.landmark_out)[e] = r;
      }
      n_fault += fault;
    }
  }
  // the named landmarks: an LDS tally, then ONE integer atomicAdd per workgroup onto the statistics
  __shared__ int s_fault;
  if (threadIdx.x == 0) s_fault = 0;
  __syncthreads();
  if (n_fault) atomicAdd(&s_fault, n_fault);
  __syncthreads();
  if (threadIdx.x == 0 && s_fault) atomicAdd(a.stats + PST_LANDMARKS_AT_FAULT, s_fault);
}

// what the row at position i of frame f is before the frame's guard: NOT_LIVE, MISS, or the landmark kernel's status
__device__ __forceinline__ int prune_row_status(const MapPruneArgs& a, int M, int f, int i, int& e) {
  e = -1;
  if (i >= live_rows(a.d_n ? a.d_n + f : nullptr, a.v.n_max)) return PS_NOT_LIVE;
  const size_t k = (size_t)f * a.v.n_max + i;
  e = a.l.ent[k];
  if (e < 0 || e >= M) { e = -1; return PS_MISS; }
  return a.w.row_st[k];
}

__global__ __launch_bounds__(PB) void prune_frame_kernel(MapPruneArgs a) {
  const FrameBlock fb = frame_block(a.nb, a.v.n_frames);
  if (!fb.live) return;                                       // (the whole workgroup)
  const int M = a.v.size();
  const int i = fb.b * PB + threadIdx.x;
  int e, s = PS_NOT_LIVE;
  if (i < a.v.n_max) s = prune_row_status(a, M, fb.f, i, e);
  const int n_obs = __syncthreads_count(s >= PS_NOT_FINITE || s == PS_KEPT);
  const int n_el = __syncthreads_count(prune_eligible(s));
  const int n_soft = __syncthreads_count(prune_soft(s));
  if (threadIdx.x == 0) {
    int* o = a.w.fpart + 4 * ((size_t)fb.f * a.nb + fb.b);
    o[0] = n_obs; o[1] = n_el; o[2] = n_soft; o[3] = 0;
  }
}

__global__ __launch_bounds__(PB) void prune_finish_kernel(MapPruneArgs a) {
  __shared__ int s_f[3];
  const FrameBlock fb = frame_block(a.nb, a.v.n_frames);
  if (!fb.live) return;                                       // (the whole workgroup)
  const int M = a.v.size();
  const int f = fb.f, tid = threadIdx.x;
  if (tid < 3) s_f[tid] = 0;
  __syncthreads();
  // ---- rule 8: the frame's counts, from the partial counts of its workgroups.  Every workgroup of the frame reads all nb of
  // them again -- nb * nb * 16 B per frame out of L2: 0.6 MB at n_max 50 000 (nb 196); beyond n_max of a few hundred thousand a
  // launch of its own for the decision would be the cheaper form ----
  {
    int c[3] = {0, 0, 0};
    for (int b = tid; b < a.nb; b += PB) {
      const int* o = a.w.fpart + 4 * ((size_t)f * a.nb + b);
      c[0] += o[0]; c[1] += o[1]; c[2] += o[2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) if (c[k]) atomicAdd(&s_f[k], c[k]);
  }
  __syncthreads();
  const int n_obs_f = s_f[0], n_el_f = s_f[1], n_soft_f = s_f[2];
  const bool fault = prune_guard_fires(n_soft_f, n_el_f, a.share_frame);
  // ---- the row ----
  const int i = fb.b * PB + tid;
  int s = -1;                                                 // (no row in this lane)
  if (i < a.v.n_max) {
    const size_t k = (size_t)f * a.v.n_max + i;
    int e;
    s = prune_row_status(a, M, f, i, e);
    if (fault && prune_soft(s)) {
      s = PS_FRAME_AT_FAULT;
      if (a.landmark_out) atomicSub(&static_cast<PruneLandmark*>(a.landmark_out)[e].n_pruned, 1);
    }
    a.entry_out[k] = (s == PS_KEPT || s == PS_LANDMARK_AT_FAULT || s == PS_FRAME_AT_FAULT) ? e : -1;
    if (a.status_out) a.status_out[k] = s;
    if (a.sq_out && (s == PS_NOT_LIVE || s == PS_MISS)) a.sq_out[k] = __longlong_as_double(0x7FF0000000000000ll);
    if (a.app_out && s != PS_NOT_LIVE) {
      const size_t r = 5 * ((size_t)f * a.app_stride + i);
      const float2* src = reinterpret_cast<const float2*>(a.app) + r;
      float2* dst = reinterpret_cast<float2*>(a.app_out) + r;
      const bool pruned = prune_pruned(s);
      if (pruned || a.app_out != a.app) {                     // (in place a row that stays is not touched)
        float2 v0 = src[0];
        if (pruned) v0.x = __int_as_float(0x7FC00000);
        const float2 v1 = src[1], v2 = src[2], v3 = src[3], v4 = src[4];
        dst[0] = v0; dst[1] = v1; dst[2] = v2; dst[3] = v3; dst[4] = v4;
      }
    }
  }
  // ---- the census: block counts per status (whole numbers), sixteen words per workgroup for prune_stats_kernel.  (Forty
  // thousand workgroups adding onto the same sixteen words of the statistics serialise: that form took 1.3 ms) ----
  int n[PS_COUNT];
#pragma unroll
  for (int k = 0; k < PS_COUNT; ++k) n[k] = __syncthreads_count(s == k);
  int obs = n[PS_KEPT], pruned = 0;
#pragma unroll
  for (int k = PS_NOT_FINITE; k < PS_COUNT; ++k) { obs += n[k]; pruned += prune_pruned(k) ? n[k] : 0; }
  if (tid < 16) {
    int mine = tid == PC_OBS ? obs : tid == PC_PRUNED ? pruned : tid == PC_FRAME_FAULT ? (fb.b == 0 && fault) : 0;
#pragma unroll
    for (int k = 0; k < PS_COUNT; ++k) mine = tid == k ? n[k] : mine;
    a.w.cpart[16 * ((size_t)f * a.nb + fb.b) + tid] = mine;
  }
  if (tid == 0 && fb.b == 0 && a.frame_out) {
    PruneFrame r;
    r.n_obs = n_obs_f; r.n_el = n_el_f; r.n_soft = n_soft_f; r.at_fault = fault;
    static_cast<PruneFrame*>(a.frame_out)[f] = r;
  }
}

// voe_map_prune_stats from the workgroups' words: one workgroup, integer sums (any order gives the same numbers).  The named
// landmarks were counted by the landmark kernel into the word the memset cleared; that word is not touched here.
__global__ __launch_bounds__(PSTAT) void prune_stats_kernel(MapPruneArgs a) {
  __shared__ int s_t[16];
  if (threadIdx.x < 16) s_t[threadIdx.x] = 0;
  __syncthreads();
  const size_t blocks = (size_t)a.v.n_frames * a.nb;
  int acc[PC_WORDS] = {};
  for (size_t i = threadIdx.x; i < blocks; i += PSTAT) {
    const int4* w = reinterpret_cast<const int4*>(a.w.cpart + 16 * i);
    const int4 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
    acc[0] += w0.x; acc[1] += w0.y; acc[2] += w0.z; acc[3] += w0.w; acc[4] += w1.x; acc[5] += w1.y; acc[6] += w1.z; acc[7] += w1.w;
    acc[8] += w2.x; acc[9] += w2.y; acc[10] += w2.z; acc[11] += w2.w; acc[12] += w3.x;
  }
#pragma unroll
  for (int k = 0; k < PC_WORDS; ++k) if (acc[k]) atomicAdd(&s_t[k], acc[k]);
  __syncthreads();
  if (threadIdx.x == 0) {
    a.stats[PST_N_FRAMES] = a.v.n_frames; a.stats[PST_N_ENTRIES] = a.v.size();
    for (int k = 0; k < PS_COUNT; ++k) a.stats[PST_BY_STATUS + k] = s_t[k];
    a.stats[PST_N_OBS] = s_t[PC_OBS]; a.stats[PST_N_PRUNED] = s_t[PC_PRUNED]; a.stats[PST_FRAMES_AT_FAULT] = s_t[PC_FRAME_FAULT];
  }
}

int map_prune_blocks(int n_max) { return n_max > 0 ? (n_max + PB - 1) / PB : 1; }

MapPruneWs map_prune_layout(void* base, int n_frames, int n_max) {
  MapPruneWs w{};
  WsCarver c(base);
  const size_t rows = (size_t)n_frames * (size_t)(n_max > 0 ? n_max : 0), R = rows > 0 ? rows : 1;
  w.sq_list = c.take<double>(8 * R);
  w.st_list = c.take<int>(4 * R);
  w.row_st = c.take<int>(4 * R);
  w.fpart = c.take<int>(16 * (size_t)n_frames * (size_t)map_prune_blocks(n_max));
  w.cpart = c.take<int>(64 * (size_t)n_frames * (size_t)map_prune_blocks(n_max));
  w.bytes = c.bytes;
  return w;
}

hipError_t launch_map_prune(hipStream_t st, const MapPruneArgs& a, int n_cu) {
  hipError_t e = hipMemsetAsync(a.stats, 0, sizeof(int) * 16, st);
  if (e != hipSuccess) return e;
  e = launch_map_refine_lists(st, a.l, a.v.n_frames, a.v.n_max, a.v.bound);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(prune_landmark_kernel, dim3(landmark_grid(a.v.bound, n_cu)), dim3(PB), 0, st, a);
  hipLaunchKernelGGL(prune_frame_kernel, frame_grid(a.nb, a.v.n_frames), dim3(PB), 0, st, a);
  hipLaunchKernelGGL(prune_finish_kernel, frame_grid(a.nb, a.v.n_frames), dim3(PB), 0, st, a);
  hipLaunchKernelGGL(prune_stats_kernel, dim3(1), dim3(PSTAT), 0, st, a);
  return hipGetLastError();
}

}  // namespace vo
