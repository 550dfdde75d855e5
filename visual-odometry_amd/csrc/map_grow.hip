// map_grow.hip -- landmarks the device map GAINS from the frames it is asked to work on (voe_map_grow*): the live rows of n_frames
// frames that find no entry are grouped into tracks by equal appearance, every track's point is triangulated from ALL its rows
// at the given poses, refined, scored with the cull's statistics, and the tracks that pass are appended by the update's own
// launches.  The rules are those of include/vo_map_grow.h.  An observation is vo_math.h's map_obs, the score is map_score.h's
// (the cull's own device function); the view of the frames, the row helpers and the landmark kernels' grid are vo_internal.h's.
// Launches behind the lookup (which wrote the map's entry of every query position into w.hit):
//   grow_open_kernel       every position: open or not, the open rows counted per block of 256 and ranked inside it
//   scan_counts_kernel     (geom.hip) the block counts -> block offsets, the number of open rows
//   grow_compact_kernel    the open rows' 40 bytes, in key order, into the cloud of the private update (stable: rank = key order)
//   (memsets, launch_map_update, launch_map_lookup on the PRIVATE table: an empty map that the update's own launches fill from
//    that cloud numbers the classes by first occurrence, whatever the scheduling -- which is the track numbering of the rules --
//    and the lookup reads every open row's track back)
//   grow_ent_kernel        the track of every query position (-1: not open) where the refinement's list launches expect the entry
//   (launch_map_refine_lists, unchanged: every track's keys in ascending order)
//   grow_track_kernel      THE HOT PATH.  16 lanes per track, all passes over the ordered list in this one launch: the nine ray sums
//                          (observation k in lane k mod 16, the lanes by refine_row_sum's tree), the 3x3 LDL^T done redundantly by
//                          the 16 lanes, n_rounds rounds of map_refine_kernel's round from the double point, the score of the
//                          float32 point by score_list.  Poses in LDS up to 512 frames, through L2 beyond.
//   grow_count_kernel      the tracks that would be added, per block of 256 tracks, and every one's rank inside its block
//   grow_scan_kernel       one workgroup: block offsets; the control words: how many qualify, how many are added, whether the map changes
//   grow_place_kernel      ADDED or NO_ROOM by the rank; where the map changes, the ADDED track's 12 + 40 bytes into the staging area
//   (launch_map_update of the staging area on the map, guarded by the control word, enqueued by the caller)
//   grow_rows_kernel       the entry every row is found at afterwards
//   grow_stats_kernel      one workgroup: an integer tally of rows and verdicts
// The count of launches is fixed by n_frames, n_max and the parameters; no launch waits for another workgroup; no float atomics.
#include "vo_internal.h"
#include "map_score.h"

namespace vo {

constexpr int GB = 256;                   // threads per workgroup
constexpr int GG = 16;                    // lanes per track: one DPP row
constexpr int GLPB = GB / GG;             // tracks per workgroup and trip
constexpr int GROW_LDS_FRAMES = 512;      // poses staged in LDS up to here (12 floats each: 24 KiB), read through L2 beyond
constexpr int GSTAT = 1024;               // threads of the scan and of the statistics workgroup
constexpr int NRAY = 9;                   // sums of the linear system: A upper triangle row by row (NREF's 0 .. 5), then b (6 .. 8)
static_assert(GB == MAP_WG && GG == MAP_ROW, "a track's lanes are one DPP row; the shared helpers of vo_internal.h count on both sizes");

// the verdicts: 4 .. 7 are the cull's own values, so that score_judge's answer is the verdict
enum { GV_ADDED = 0, GV_FEW_OBS = 1, GV_FEW_FRAMES = 2, GV_DEGENERATE = 3, GV_NOT_FINITE = 4, GV_BEHIND = 5, GV_HIGH_ERROR = 6, GV_LOW_PARALLAX = 7,
       GV_NO_ROOM = 8, GV_COUNT = 12 };
static_assert(GV_NOT_FINITE == CV_NOT_FINITE && GV_BEHIND == CV_BEHIND && GV_HIGH_ERROR == CV_HIGH_ERROR && GV_LOW_PARALLAX == CV_LOW_PARALLAX && CV_KEPT == GV_ADDED,
              "score_judge's answer is the track's verdict");
enum { OC_NOT_LIVE = -1, OC_NAN = -2, OC_HIT = -3 };
enum { GC_OPEN = 0, GC_PRIV_HITS = 1, GC_QUALIFY = 2, GC_ADDED = 3, GC_BEFORE = 4, GC_CHANGES = 5 };

struct GrowTrack { int32_t verdict, n_obs, n_frames, entry, first_key, refined, reserved[2]; float xyz[3]; int32_t reserved2; double mean_sq, max_sq, min_z, cos_parallax; };
static_assert(sizeof(GrowTrack) == 80, "voe_map_grow_track");

__device__ __forceinline__ size_t grow_rows(const MapGrowArgs& a) { return (size_t)a.v.n_frames * (size_t)a.v.n_max; }
// the 40 bytes of the row with the key k
__device__ __forceinline__ const float2* grow_row(const MapGrowArgs& a, size_t k) {
  const size_t f = k / (size_t)a.v.n_max, i = k - f * (size_t)a.v.n_max;
  return reinterpret_cast<const float2*>(a.app + f * a.app_stride) + 5 * i;
}

__global__ __launch_bounds__(GB) void grow_open_kernel(MapGrowArgs a) {
  __shared__ int s_wave[GB / 64];
  const size_t rows = grow_rows(a), k = (size_t)blockIdx.x * GB + threadIdx.x;
  int code = OC_NOT_LIVE;
  bool open = false;
  if (k < rows) {
    const int f = (int)(k / (size_t)a.v.n_max), i = (int)(k - (size_t)f * a.v.n_max);
    if (i < live_rows(a.d_n ? a.d_n + f : nullptr, a.v.n_max)) {
      const float2* p = grow_row(a, k);
      bool nan = false;
#pragma unroll
      for (int c = 0; c < 5; ++c) { const float2 t = p[c]; nan |= (t.x != t.x) | (t.y != t.y); }
      if (nan) code = OC_NAN;
      else if (a.w.hit[k] >= 0) code = OC_HIT;
      else open = true;
    }
  }
  int tot;
  const int r = block_rank<GB>(open, s_wave, tot);
  if (k < rows) a.w.ocode[k] = open ? r : code;
  if (threadIdx.x == 0) a.w.oblk[blockIdx.x] = tot;
}

__global__ __launch_bounds__(GB) void grow_compact_kernel(MapGrowArgs a) {
  const size_t rows = grow_rows(a), k = (size_t)blockIdx.x * GB + threadIdx.x;
  if (k >= rows) return;
  const int c = a.w.ocode[k];
  if (c < 0) return;
  const size_t j = (size_t)a.w.oblk[blockIdx.x] + c;        // < rows: one place per open row
  const float2* src = grow_row(a, k);
  float2* dst = reinterpret_cast<float2*>(a.w.oapp) + 5 * j;
#pragma unroll
  for (int q = 0; q < 5; ++q) dst[q] = src[q];
}

__global__ __launch_bounds__(GB) void grow_ent_kernel(MapGrowArgs a) {
  const size_t rows = grow_rows(a), k = (size_t)blockIdx.x * GB + threadIdx.x;
  if (k >= rows) return;
  const int c = a.w.ocode[k];
  a.l.ent[k] = c >= 0 ? a.w.otrack[(size_t)a.w.oblk[blockIdx.x] + c] : -1;
}

// One observation's terms of the linear system: d = R^T K^-1 (mu, mv, 1), u = d / |d|, c = -R^T t; acc += I - u u^T (upper triangle
// row by row), then (I - u u^T) c.  Returns whether |d| > 0 (a NaN is not).
__device__ __forceinline__ bool grow_ray_term(const double Kinv[9], const float Rt[12], double mu, double mv, double acc[NRAY]) {
  double m[3], d[3], c[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) m[r] = __builtin_fma(Kinv[r + 3], mv, __builtin_fma(Kinv[r], mu, Kinv[r + 6]));
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    d[q] = __builtin_fma((double)Rt[2 + 3 * q], m[2], __builtin_fma((double)Rt[1 + 3 * q], m[1], (double)Rt[3 * q] * m[0]));
    c[q] = -__builtin_fma((double)Rt[2 + 3 * q], (double)Rt[11], __builtin_fma((double)Rt[1 + 3 * q], (double)Rt[10], (double)Rt[3 * q] * (double)Rt[9]));
  }
  const double nrm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  const double u[3] = {d[0] / nrm, d[1] / nrm, d[2] / nrm};
  const double uc = u[0] * c[0] + u[1] * c[1] + u[2] * c[2];
  acc[0] += 1.0 - u[0] * u[0]; acc[1] -= u[0] * u[1]; acc[2] -= u[0] * u[2];
  acc[3] += 1.0 - u[1] * u[1]; acc[4] -= u[1] * u[2]; acc[5] += 1.0 - u[2] * u[2];
  acc[6] += c[0] - u[0] * uc; acc[7] += c[1] - u[1] * uc; acc[8] += c[2] - u[2] * uc;
  return nrm > 0.0;
}

template <bool LDS>
__global__ __launch_bounds__(GB) void grow_track_kernel(MapGrowArgs a) {
  __shared__ float s_pose[LDS ? GROW_LDS_FRAMES * 12 : 12];
  if (LDS) {
    for (int k = threadIdx.x; k < a.v.n_frames * 12; k += GB) s_pose[k] = a.v.pose_at(k / 12, k % 12);
    __syncthreads();
  }
  const int T = a.v.size(), n_max = a.v.n_max;               // (v.hdr is the private header: the number of tracks)
  const int lg = threadIdx.x & (GG - 1), grp = threadIdx.x / GG;
  double K[9], Kinv[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) { K[k] = a.v.K[k]; Kinv[k] = a.Kinv[k]; }
  const MapScoreThr thr{a.max_mean_sq, a.max_sq, a.cos_thr, a.parallax};
  const auto load_pose = [&](int f, float Rt[12]) {
    if (LDS) {
#pragma unroll
      for (int k = 0; k < 12; ++k) Rt[k] = s_pose[12 * f + k];
    } else {
      a.v.load_pose(f, Rt);
    }
  };
  const int n_batches = (T + GLPB - 1) / GLPB;               // (the grid is sized by the rows, the work by the tracks there are)
  for (int batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {      // (uniform in the workgroup: the row steps below see whole waves)
    const int t = batch * GLPB + grp;
    const bool in = t < T;
    const int n = in ? a.l.cur[t] : 0;
    const int* keys = a.l.keys + (in ? a.l.offset(t) : 0);
    // ---- the linear point: the ray sums and the frame changes ----
    double ray[NRAY];
#pragma unroll
    for (int k = 0; k < NRAY; ++k) ray[k] = 0.0;
    double changes = 0.0;
    bool zero = false;
    for (int j = lg; j < n; j += GG) {
      const int key = keys[j];
      const int prev = j > 0 ? keys[j - 1] / n_max : -1;
      changes += (key / n_max != prev) ? 1.0 : 0.0;
      float2 m;
      const int f = a.v.decode(key, m);
      float Rt[12];
      load_pose(f, Rt);
      zero |= !grow_ray_term(Kinv, Rt, (double)m.x, (double)m.y, ray);
    }
#pragma unroll
    for (int k = 0; k < NRAY; ++k) ray[k] = refine_row_sum(ray[k]);
    const int n_fr = (int)refine_row_sum(changes);           // (whole numbers below 2^31: exact)
    const bool any_zero = refine_row_any(zero);
    const bool few_obs = n < a.min_obs, few_fr = n_fr < a.min_frames;
    bool degenerate = false;
    double p[3] = {0.0, 0.0, 0.0};
    if (in && !few_obs && !few_fr) {
      bool finite = true;
#pragma unroll
      for (int k = 0; k < NRAY; ++k) finite &= refine_finite(ray[k]);
      degenerate = !finite || any_zero || !ldlt3_solve(ray, ray + 6, p);
    }
    const bool solved = in && !few_obs && !few_fr && !degenerate;
    float pf[3] = {(float)p[0], (float)p[1], (float)p[2]};   // p_lin rounded once: stands unless the refined point is taken
    // ---- the rounds: map_refine_kernel's, from p_lin in double ----
    bool run = solved && a.n_rounds > 0;
    bool not_finite = false, behind = false;
    double cost0 = 0.0, cost1 = 0.0;
    float rf[3] = {pf[0], pf[1], pf[2]};
    if (a.n_rounds > 0) {
      for (int r = 0; r <= a.n_rounds; ++r) {
        double acc[NREF];
#pragma unroll
        for (int k = 0; k < NREF; ++k) acc[k] = 0.0;
        bool bh = false;
        if (run) {
          for (int j = lg; j < n; j += GG) {
            float2 m;
            const int f = a.v.decode(keys[j], m);
            float Rt[12];
            load_pose(f, Rt);
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
                if (r == a.n_rounds - 1) {                   // rounded once: the cost that decides is the stored point's
                  rf[0] = (float)p[0]; rf[1] = (float)p[1]; rf[2] = (float)p[2];
                  p[0] = (double)rf[0]; p[1] = (double)rf[1]; p[2] = (double)rf[2];
                }
                if (!(refine_finite(p[0]) && refine_finite(p[1]) && refine_finite(p[2]))) { not_finite = true; run = false; }
              }
            }
          }
        }
      }
    }
    // refine's own status would be OK: finite, camera z > 0 in every round, cost not risen
    const bool refined = solved && a.n_rounds > 0 && !not_finite && !behind && !(cost1 > cost0);
    if (refined) { pf[0] = rf[0]; pf[1] = rf[1]; pf[2] = rf[2]; }
    // ---- the score of the float32 point, widened again ----
    const double pw[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
    const MapScore sc = score_list(a.v, load_pose, K, pw, keys, solved ? n : 0, a.parallax != 0, lg);
    if (in && lg == 0) {
      double mean = 0.0, cosp = 1.0, mx = 0.0, mz = 0.0;
      int v;
      if (few_obs) v = GV_FEW_OBS;
      else if (few_fr) v = GV_FEW_FRAMES;
      else if (degenerate) v = GV_DEGENERATE;
      else { v = score_judge(sc, n, thr, mean, cosp); mx = sc.mx; mz = sc.mz; }
      if (!solved) { pf[0] = 0.f; pf[1] = 0.f; pf[2] = 0.f; }
      a.w.verdict[t] = v;
      a.w.rank[t] = v == GV_ADDED ? 1 : 0;
      a.w.xyz[3 * (size_t)t] = pf[0]; a.w.xyz[3 * (size_t)t + 1] = pf[1]; a.w.xyz[3 * (size_t)t + 2] = pf[2];
      if (a.track_out && t < a.track_cap) {
        GrowTrack r;
        r.verdict = v; r.n_obs = n; r.n_frames = n_fr; r.entry = -1; r.first_key = n > 0 ? keys[0] : -1; r.refined = refined ? 1 : 0;
        r.reserved[0] = 0; r.reserved[1] = 0; r.reserved2 = 0;
        r.xyz[0] = pf[0]; r.xyz[1] = pf[1]; r.xyz[2] = pf[2];
        r.mean_sq = mean; r.max_sq = mx; r.min_z = mz; r.cos_parallax = cosp;
        static_cast<GrowTrack*>(a.track_out)[t] = r;
      }
    }
  }
}

__global__ __launch_bounds__(GB) void grow_count_kernel(MapGrowArgs a) {
  __shared__ int s_wave[GB / 64];
  const int T = a.v.size();
  const int t = blockIdx.x * GB + threadIdx.x;
  const int v = t < T ? a.w.rank[t] : 0;
  int tot;
  const int x = block_exclusive_scan<GB>(v, s_wave, tot);
  if (t < T) a.w.rank[t] = v ? x : -1;
  if (threadIdx.x == 0) a.w.blk[blockIdx.x] = tot;
}

__global__ __launch_bounds__(GSTAT) void grow_scan_kernel(MapGrowArgs a, int nb) {
  __shared__ int s_w[GSTAT / 64];
  __shared__ int s_carry;
  const int qualify = scan_with_carry<GSTAT>(a.w.blk, nb, s_w, &s_carry);
  if (threadIdx.x == 0) {
    int M = a.map_hdr[0];
    M = M < a.map_cap ? M : a.map_cap;
    const int added = qualify < a.max_added ? qualify : a.max_added;
    a.w.ctl[GC_QUALIFY] = qualify; a.w.ctl[GC_ADDED] = added; a.w.ctl[GC_BEFORE] = M;
    a.w.ctl[GC_CHANGES] = (added > 0 && !a.dry_run) ? 1 : 0;
  }
}

__global__ __launch_bounds__(GB) void grow_place_kernel(MapGrowArgs a) {
  const int T = a.v.size();
  const int t = blockIdx.x * GB + threadIdx.x;
  if (t >= T) return;
  const int r = a.w.rank[t];
  int v = a.w.verdict[t], entry = -1;
  if (r >= 0) {
    const int g = a.w.blk[blockIdx.x] + r;                   // the track's rank among those that qualify, in track order
    if (g < a.max_added) {
      entry = a.w.ctl[GC_BEFORE] + g;
      if (a.w.ctl[GC_CHANGES] && a.l.cur[t] > 0) {             // (a track has a row, always)
        a.w.stage_pts[3 * (size_t)g] = a.w.xyz[3 * (size_t)t];
        a.w.stage_pts[3 * (size_t)g + 1] = a.w.xyz[3 * (size_t)t + 1];
        a.w.stage_pts[3 * (size_t)g + 2] = a.w.xyz[3 * (size_t)t + 2];
        const float2* src = grow_row(a, (size_t)a.l.keys[a.l.offset(t)]);      // the track keeps the bits of its first row
        float2* dst = reinterpret_cast<float2*>(a.w.stage_app) + 5 * (size_t)g;
#pragma unroll
        for (int q = 0; q < 5; ++q) dst[q] = src[q];
      }
    } else {
      v = GV_NO_ROOM;
    }
  }
  a.w.verdict[t] = v;
  a.w.entry[t] = entry;
  if (a.track_out && t < a.track_cap) {
    GrowTrack* rec = static_cast<GrowTrack*>(a.track_out) + t;
    rec->verdict = v; rec->entry = entry;
  }
}

__global__ __launch_bounds__(GB) void grow_rows_kernel(MapGrowArgs a) {
  const size_t rows = grow_rows(a), k = (size_t)blockIdx.x * GB + threadIdx.x;
  if (k >= rows) return;
  const int c = a.w.ocode[k];
  int out = -1;
  if (c == OC_HIT) {
    out = a.w.hit[k];
  } else if (c >= 0) {
    const int t = a.l.ent[k];
    if (t >= 0) out = a.w.verdict[t] == GV_ADDED ? a.w.entry[t] : -2 - t;      // (always: every open row has a track)
  }
  a.row_out[k] = out;
}

// voe_map_grow_stats: int32 status, n_live, n_hits, n_nan, n_open, n_tracks, n_added, n_before, n_after, by_verdict[12], reserved[3].
// Whole numbers: any order gives the same tally.
__global__ __launch_bounds__(GSTAT) void grow_stats_kernel(MapGrowArgs a) {
  __shared__ int s_n[GV_COUNT + 3];
  const size_t rows = grow_rows(a);
  const int T = a.v.size();
  if (threadIdx.x < GV_COUNT + 3) s_n[threadIdx.x] = 0;
  __syncthreads();
  int hits = 0, nan = 0, dead = 0;
  for (size_t k = threadIdx.x; k < rows; k += GSTAT) {
    const int c = a.w.ocode[k];
    hits += c == OC_HIT; nan += c == OC_NAN; dead += c == OC_NOT_LIVE;
  }
  int n[GV_COUNT];
#pragma unroll
  for (int k = 0; k < GV_COUNT; ++k) n[k] = 0;
  for (int t = threadIdx.x; t < T; t += GSTAT) {
    const int v = a.w.verdict[t];
#pragma unroll
    for (int k = 0; k < GV_COUNT; ++k) n[k] += v == k;
  }
#pragma unroll
  for (int k = 0; k < GV_COUNT; ++k) if (n[k]) atomicAdd(&s_n[k], n[k]);
  if (hits) atomicAdd(&s_n[GV_COUNT], hits);
  if (nan) atomicAdd(&s_n[GV_COUNT + 1], nan);
  if (dead) atomicAdd(&s_n[GV_COUNT + 2], dead);
  __syncthreads();
  if (threadIdx.x == 0) {
    int* si = static_cast<int*>(a.stats);
    const int open = a.w.ctl[GC_OPEN], added = a.w.ctl[GC_ADDED], M = a.w.ctl[GC_BEFORE];
    si[0] = open == 0 ? 1 : (added == 0 ? 2 : 0);
    si[1] = (int)(rows - (size_t)s_n[GV_COUNT + 2]); si[2] = s_n[GV_COUNT]; si[3] = s_n[GV_COUNT + 1]; si[4] = open; si[5] = T;
    si[6] = added; si[7] = M; si[8] = M + added;
    for (int k = 0; k < GV_COUNT; ++k) si[9 + k] = s_n[k];
    si[21] = 0; si[22] = 0; si[23] = 0;
  }
}

MapGrowWs map_grow_layout(void* base, size_t rows, int stage_rows, unsigned tcap) {
  MapGrowWs w{};
  WsCarver c(base);
  const size_t R = rows ? rows : 1, A = (size_t)(stage_rows > 0 ? stage_rows : 1), nb = (R + GB - 1) / GB;
  w.hit = c.take<int32_t>(4 * R);
  w.ocode = c.take<int>(4 * R);
  w.oblk = c.take<int>(4 * nb);
  w.oapp = c.take<float>(40 * R);
  w.otrack = c.take<int32_t>(4 * R);
  w.verdict = c.take<int32_t>(4 * R);
  w.entry = c.take<int32_t>(4 * R);
  w.xyz = c.take<float>(12 * R);
  w.rank = c.take<int>(4 * R);
  w.blk = c.take<int>(4 * nb);
  w.stage_pts = c.take<float>(12 * A);
  w.stage_app = c.take<float>(40 * A);
  w.upd = c.take<int>(sizeof(int) * map_scratch_ints((int)R));
  w.look = c.take<int>(sizeof(int) * map_lookup_scratch_ints((int)R, 1, false));
  w.priv.cap = (int)R; w.priv.tcap = tcap;
  w.priv.pts = c.take<float>(12 * R);
  w.priv.app = c.take<float>(40 * R);
  w.priv.table = c.take<unsigned long long>(sizeof(unsigned long long) * (size_t)tcap);
  w.priv.last = c.take<int>(sizeof(int) * (size_t)tcap);
  w.priv.hdr = c.take<int>(64);
  w.ctl = c.take<int>(64);
  w.bytes = c.bytes;
  return w;
}

hipError_t launch_map_grow(hipStream_t st, const MapGrowArgs& a, int n_cu) {
  const size_t rows = (size_t)a.v.n_frames * (size_t)a.v.n_max, R = rows ? rows : 1;
  const unsigned nb = (unsigned)((R + GB - 1) / GB);
  hipError_t e = hipMemsetAsync(a.w.ctl, 0, 64, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(grow_open_kernel, dim3(nb), dim3(GB), 0, st, a);
  e = launch_scan(st, a.w.oblk, (int)nb, a.w.ctl + GC_OPEN);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(grow_compact_kernel, dim3(nb), dim3(GB), 0, st, a);
  // the tracks: an empty private map, filled by the update's own launches from the compacted open rows, read back by the lookup's
  e = hipMemsetAsync(a.w.priv.hdr, 0, 64, st);
  if (e != hipSuccess) return e;
  e = launch_map_rehash(st, a.w.priv, 0);
  if (e != hipSuccess) return e;
  // (the private map's points are read by nobody; the commit still copies three floats per open row, so the cloud's points are
  // the compacted rows -- written above, 10 floats a row -- not w.xyz, which this call writes only in grow_track_kernel)
  e = launch_map_update(st, a.w.priv, a.w.oapp, a.w.oapp, (int)R, a.w.ctl + GC_OPEN, nullptr, a.w.upd);
  if (e != hipSuccess) return e;
  e = launch_map_lookup(st, a.w.priv, a.w.oapp, R, (int)R, a.w.ctl + GC_OPEN, 1, nullptr, a.w.ctl + GC_PRIV_HITS, nullptr, nullptr, a.w.otrack, a.w.look);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(grow_ent_kernel, dim3(nb), dim3(GB), 0, st, a);
  e = launch_map_refine_lists(st, a.l, a.v.n_frames, a.v.n_max, a.v.bound);
  if (e != hipSuccess) return e;
  // (the registers of map_refine_kernel's round, and 4 x 24 KiB of LDS: the 4 waves per SIMD landmark_grid counts on)
  const dim3 grid(landmark_grid(a.v.bound, n_cu));
  if (a.v.n_frames <= GROW_LDS_FRAMES) hipLaunchKernelGGL(grow_track_kernel<true>, grid, dim3(GB), 0, st, a);
  else hipLaunchKernelGGL(grow_track_kernel<false>, grid, dim3(GB), 0, st, a);
  hipLaunchKernelGGL(grow_count_kernel, dim3(nb), dim3(GB), 0, st, a);
  hipLaunchKernelGGL(grow_scan_kernel, dim3(1), dim3(GSTAT), 0, st, a, (int)nb);
  hipLaunchKernelGGL(grow_place_kernel, dim3(nb), dim3(GB), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_grow_finish(hipStream_t st, const MapGrowArgs& a) {
  const size_t rows = (size_t)a.v.n_frames * (size_t)a.v.n_max, R = rows ? rows : 1;
  if (a.row_out) hipLaunchKernelGGL(grow_rows_kernel, dim3((unsigned)((R + GB - 1) / GB)), dim3(GB), 0, st, a);
  hipLaunchKernelGGL(grow_stats_kernel, dim3(1), dim3(GSTAT), 0, st, a);
  return hipGetLastError();
}

}  // namespace vo
