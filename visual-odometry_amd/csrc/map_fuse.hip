// map_fuse.hip -- voe_map_fuse*: duplicate landmarks of the map found as mutual nearest neighbours in space and appearance, and
// fused (the rules: include/vo_hip.h, FUSE).  The hot path is a SELF-JOIN of the map within radius_xyz:
// a uniform 3-D grid over the bounding box of the finite points, built by the call and kept by none, as map_nearest.hip builds
// its 4-D grid over appearances and map_guided.hip its pixel grids.  This file holds no compaction kernel: the survivors are
// compacted, header and table rebuilt, by voe_map_cull's own kernels (launch_map_cull_compact, launch_map_rehash), which the
// caller enqueues between launch_map_fuse and launch_map_fuse_finish.
//
// Launches, a fixed sequence (behind two memsets: the box's lower corner to 0xFF; the accumulators and the cell counts to 0):
//   fuse_box_kernel        at most 2048 workgroups stride over the entries: is an entry finite (point and appearance)?  The bounding
//                          box of the finite points by a workgroup reduction and ONE integer atomicMin / atomicMax per word and
//                          workgroup on order-preserving bit keys (exact in any order); the defaults of partner, distance and gap.
//   fuse_grid_kernel       one thread: per axis nc = clamp(floor(extent / R), 1, lim) cells of width >= R = 1.001 radius_xyz,
//                          lim = the smallest of 2 .. FUSE_NC with lim^3 >= size (about one entry per cell where the extents
//                          allow it).  Zero extent, no finite point, R not finite: one cell on that axis.
//   fuse_count_kernel      one finite entry per lane: an integer atomicAdd on its cell's count
//   fuse_sums_kernel, fuse_starts_kernel   the start table (map_nearest.hip's two-launch scan)
//   fuse_place_kernel      one finite entry per lane: its 16-byte record {x, y, z, entry} at the cell's cursor.  The order INSIDE
//                          a cell is whatever the atomics make it; no result depends on it (ties go to the lowest entry index).
//   fuse_search_kernel     one RECORD per lane, in record order -- the lanes of a wave sit in the same or in neighbouring cells
//                          and walk the same records --: the cells [cell(x - R), cell(x + R)] per axis (<= 3 each, contiguous
//                          along z: <= 9 runs), g2 on the record alone, the 40-byte appearance row of the survivors only (8-byte
//                          loads), best (d2, lowest index) in registers.  n_gated: one 64-bit integer atomicAdd per workgroup.
//   (launch_map_refine_lists with frames: the ordered observation lists of the lookup the caller enqueued)
//   fuse_verdict_kernel    one entry per lane and trip (at most 2048 workgroups; the tallies go out once per workgroup): mutual? vetoed (a merge walk of the two ordered lists)? the verdict, the keep flag
//                          for the compaction, and the survivor's midpoint (position == 1, no dry run).  A survivor writes its
//                          own point and reads its partner's, which is ABSORBED and written by nobody.
//   fuse_rows_kernel       one row per lane (with frames): a live row that hit an ABSORBED entry gets its survivor's 40 bytes
//   fuse_finish_kernel     (behind the compaction and the rehash) an ABSORBED entry's remap = its survivor's; the statistics
//
// EXACTNESS.  The grid changes no decision:
//  * cell(x) = trunc(clamp((x - lo) * scale, 0, nc - 1)) is monotone non-decreasing in x for every lo and every scale >= 0, and
//    float rounding is monotone.  A candidate b of a has g2 < fl(radius_xyz^2), so on every axis |x_b - x_a| < radius_xyz in real
//    numbers (if |d| >= r then fl(d)^2 >= fl(r * r), and a sum of non-negative terms rounded to nearest never falls below a term),
//    hence x_a - R <= x_b <= x_a + R, fl(x_a - R) <= x_b <= fl(x_a + R) and cell(fl(x_a - R)) <= cell(x_b) <= cell(fl(x_a + R)): the
//    walked box holds b whatever the bounding box, the widths and the roundings were -- also when an axis has one cell.
//  * count and place form the cell with the same instructions on the same data, so the counts add up to the records placed.
//  * NOT_FINITE entries get no record: they are nobody's candidate and walk nothing.
#include "vo_internal.h"

namespace vo {

constexpr int FB = 256;                   // threads per workgroup
constexpr unsigned FUSE_GRID = 2048;      // workgroups of the two kernels that end in atomics on a few words: they stride over the entries
static_assert(FUSE_SCAN % FB == 0, "the scan gives every thread the same number of cells");

enum { FV_NOT_FINITE = 0, FV_ALONE = 1, FV_NOT_MUTUAL = 2, FV_CONFLICT = 3, FV_SURVIVOR = 4, FV_ABSORBED = 5 };      // VOE_MAP_FUSE_*
enum { FA_PAIRS = 6, FA_CONFLICTS = 7, FA_ROWS = 8, FA_GATED = 10, FA_BOX_HI = 12 };                                // MapFuseWs::acc

struct FuseGrid { float lo[3], scale[3]; int nc[3]; float R; int n_cells, M; int pad[4]; };
static_assert(sizeof(FuseGrid) == 64, "MapFuseWs::grid");

__device__ __forceinline__ int fuse_size(const MapFuseArgs& a) {
  int M = a.hdr[0];
  M = M < a.cap ? M : a.cap;
  M = M < a.bound ? M : a.bound;
  return M > 0 ? M : 0;
}
__device__ __forceinline__ bool ffinite(float x) { return (x - x) == 0.f; }
// unsigned keys that order as the floats do (-0 below +0)
__device__ __forceinline__ unsigned fkey(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float funkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
__device__ __forceinline__ int fcell1(float x, float lo, float scale, int nc) {      // cell1 of map_nearest.hip
  float v = (x - lo) * scale;                               // monotone non-decreasing in x
  v = fminf(fmaxf(v, 0.f), (float)(nc - 1));                // NaN -> 0, +-inf clamp
  return (int)v;
}
__device__ __forceinline__ int fuse_cell(const FuseGrid& g, float x, float y, float z) {
  return (fcell1(x, g.lo[0], g.scale[0], g.nc[0]) * g.nc[1] + fcell1(y, g.lo[1], g.scale[1], g.nc[1])) * g.nc[2] + fcell1(z, g.lo[2], g.scale[2], g.nc[2]);
}
__device__ __forceinline__ Row fuse_load_row(const float* app, size_t i) {
  const float2* p = reinterpret_cast<const float2*>(app) + 5 * i;
  Row r;
#pragma unroll
  for (int k = 0; k < 5; ++k) { const float2 t = p[k]; r.v[2 * k] = t.x; r.v[2 * k + 1] = t.y; }
  return r;
}

__global__ __launch_bounds__(FB) void fuse_box_kernel(MapFuseArgs a) {
  __shared__ unsigned s_lo[FB / 64][3], s_hi[FB / 64][3];
  const int M = fuse_size(a);
  unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
  for (int e = blockIdx.x * FB + threadIdx.x; e < M; e += gridDim.x * FB) {
    const Row r = fuse_load_row(a.app, (size_t)e);
    bool fin = true;
    float p[3];
#pragma unroll
    for (int k = 0; k < 10; ++k) fin = fin && ffinite(r.v[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) { p[k] = a.pts[3 * (size_t)e + k]; fin = fin && ffinite(p[k]); }
    a.w.fin[e] = fin ? 1 : 0;
    a.partner[e] = -1;
    if (a.dist2) a.dist2[e] = INFINITY;
    if (a.gap2) a.gap2[e] = INFINITY;
    if (fin) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { const unsigned key = fkey(p[k]); lo[k] = key < lo[k] ? key : lo[k]; hi[k] = key > hi[k] ? key : hi[k]; }
    }
  }
  // the workgroup's corner: a wave reduction, the waves through LDS, then ONE integer atomic per word (a grid of at most
  // FUSE_GRID workgroups: a few thousand atomics on six words, whatever the size)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned l2 = (unsigned)__shfl_xor((int)lo[k], d), h2 = (unsigned)__shfl_xor((int)hi[k], d);
      lo[k] = l2 < lo[k] ? l2 : lo[k]; hi[k] = h2 > hi[k] ? h2 : hi[k];
    }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6][k] = lo[k]; s_hi[threadIdx.x >> 6][k] = hi[k]; }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    unsigned l = s_lo[0][k], h = s_hi[0][k];
    for (int w = 1; w < FB / 64; ++w) { l = s_lo[w][k] < l ? s_lo[w][k] : l; h = s_hi[w][k] > h ? s_hi[w][k] : h; }
    if (l <= h) {                                           // (some finite point)
      atomicMin(&a.w.box_lo[k], l);
      atomicMax(reinterpret_cast<unsigned*>(a.w.acc) + FA_BOX_HI + k, h);
    }
  }
}

__global__ void fuse_grid_kernel(MapFuseArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int M = fuse_size(a);
  int lim = 2;
  while (lim < FUSE_NC && (long long)lim * lim * lim < (long long)M) ++lim;
  FuseGrid g{};
  g.R = a.radius_xyz * 1.001f;
  g.M = M; g.n_cells = 1;
  const unsigned* hi_keys = reinterpret_cast<const unsigned*>(a.w.acc) + FA_BOX_HI;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    g.lo[k] = 0.f; g.scale[k] = 0.f; g.nc[k] = 1;           // no finite point, zero or infinite extent, R not finite: one cell
    const unsigned kl = a.w.box_lo[k], kh = hi_keys[k];
    if (kl <= kh) {
      const float l = funkey(kl), h = funkey(kh), span = h - l;
      if (span > 0.f && span < INFINITY && g.R > 0.f && g.R < INFINITY) {
        const float q = span / g.R;
        int nc = q >= (float)lim ? lim : (int)q;
        if (nc < 1) nc = 1;
        g.lo[k] = l; g.nc[k] = nc; g.scale[k] = (float)nc / span;      // cell width span / nc >= R up to the rounding of q
      }
    }
    g.n_cells *= g.nc[k];
  }
  *reinterpret_cast<FuseGrid*>(a.w.grid) = g;
}

__global__ __launch_bounds__(FB) void fuse_count_kernel(MapFuseArgs a) {
  const FuseGrid& g = *reinterpret_cast<const FuseGrid*>(a.w.grid);
  const int e = blockIdx.x * FB + threadIdx.x;
  if (e >= g.M || !a.w.fin[e]) return;
  const float* p = a.pts + 3 * (size_t)e;
  atomicAdd(&a.w.counts[fuse_cell(g, p[0], p[1], p[2])], 1);
}

__global__ __launch_bounds__(FB) void fuse_sums_kernel(MapFuseArgs a) {
  __shared__ int s_w[FB / 64];
  const int n_cells = reinterpret_cast<const FuseGrid*>(a.w.grid)->n_cells;
  if ((int)blockIdx.x * FUSE_SCAN >= n_cells) {             // (the whole workgroup)
    if (threadIdx.x == 0) a.w.bsum[blockIdx.x] = 0;
    return;
  }
  const int i0 = blockIdx.x * FUSE_SCAN + threadIdx.x * (FUSE_SCAN / FB);
  int v = 0;
#pragma unroll
  for (int k = 0; k < FUSE_SCAN / FB; ++k) v += i0 + k < n_cells ? a.w.counts[i0 + k] : 0;
  const int tot = block_sum(v, s_w);
  if (threadIdx.x == 0) a.w.bsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(FB) void fuse_starts_kernel(MapFuseArgs a) {
  __shared__ int s_w[FB / 64];
  const int n_cells = reinterpret_cast<const FuseGrid*>(a.w.grid)->n_cells;
  if ((int)blockIdx.x * FUSE_SCAN > n_cells) return;        // (the whole workgroup)
  int pre = 0;
  for (int j = threadIdx.x; j < (int)blockIdx.x; j += FB) pre += a.w.bsum[j];
  pre = block_sum(pre, s_w);
  const int i0 = blockIdx.x * FUSE_SCAN + threadIdx.x * (FUSE_SCAN / FB);
  int c[FUSE_SCAN / FB], mine = 0;
#pragma unroll
  for (int k = 0; k < FUSE_SCAN / FB; ++k) { c[k] = i0 + k < n_cells ? a.w.counts[i0 + k] : 0; mine += c[k]; }
  __syncthreads();                                          // (s_w is read by block_sum's last step)
  int tot;
  int run = pre + block_exclusive_scan<FB>(mine, s_w, tot);
#pragma unroll
  for (int k = 0; k < FUSE_SCAN / FB; ++k) {
    if (i0 + k <= n_cells) a.w.starts[i0 + k] = run;        // [n_cells]: the records in all
    if (i0 + k < n_cells) a.w.counts[i0 + k] = run;         // the cell's cursor
    run += c[k];
  }
}

__global__ __launch_bounds__(FB) void fuse_place_kernel(MapFuseArgs a) {
  const FuseGrid& g = *reinterpret_cast<const FuseGrid*>(a.w.grid);
  const int e = blockIdx.x * FB + threadIdx.x;
  if (e >= g.M || !a.w.fin[e]) return;
  const float* p = a.pts + 3 * (size_t)e;
  const float x = p[0], y = p[1], z = p[2];
  const int pos = atomicAdd(&a.w.counts[fuse_cell(g, x, y, z)], 1);
  if (pos >= 0 && pos < g.M) a.w.rec[pos] = make_float4(x, y, z, __int_as_float(e));      // (always: the counts add up to <= M)
}

__global__ __launch_bounds__(FB) void fuse_search_kernel(MapFuseArgs a) {
  __shared__ unsigned long long s_gated[FB / 64];
  const FuseGrid g = *reinterpret_cast<const FuseGrid*>(a.w.grid);
  int n_rec = a.w.starts[g.n_cells];
  n_rec = n_rec < g.M ? n_rec : g.M;
  const int p = blockIdx.x * FB + threadIdx.x;
  unsigned long long gated = 0;
  if (p < n_rec) {
    const float4 me = a.w.rec[p];
    const int e = __float_as_int(me.w);
    const Row q = fuse_load_row(a.app, (size_t)e);
    const float r2 = a.radius * a.radius, x2 = a.radius_xyz * a.radius_xyz;
    const float xyz[3] = {me.x, me.y, me.z};
    int lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lo[k] = fcell1(xyz[k] - g.R, g.lo[k], g.scale[k], g.nc[k]);
      hi[k] = fcell1(xyz[k] + g.R, g.lo[k], g.scale[k], g.nc[k]);
    }
    int bi = -1;
    float bd = INFINITY, bg = INFINITY;
    for (int c0 = lo[0]; c0 <= hi[0]; ++c0)
      for (int c1 = lo[1]; c1 <= hi[1]; ++c1) {
        const int base = (c0 * g.nc[1] + c1) * g.nc[2];
        int s1 = a.w.starts[base + hi[2] + 1];
        s1 = s1 < n_rec ? s1 : n_rec;
        for (int s = a.w.starts[base + lo[2]]; s < s1; ++s) {
          const float4 t = a.w.rec[s];
          const int b = __float_as_int(t.w);
          if (b == e) continue;
          // the spatial gate, on the record alone (rule 1: unfused, in this order)
          const float dx = t.x - me.x, dy = t.y - me.y, dz = t.z - me.z;
          const float g2 = (dx * dx + dy * dy) + dz * dz;
          if (!(g2 < x2)) continue;
          ++gated;
          const Row r = fuse_load_row(a.app, (size_t)b);
          // the appearance distance: the unfused left-to-right sum (NEAREST's rule 1; match.hip)
          float d = r.v[0] - q.v[0];
          float d2 = d * d;
#pragma unroll
          for (int k = 1; k < 10; ++k) { d = r.v[k] - q.v[k]; d2 += d * d; }
          if (!(d2 < r2)) continue;
          if (d2 < bd || (d2 == bd && b < bi)) { bd = d2; bg = g2; bi = b; }
        }
      }
    a.partner[e] = bi;
    if (a.dist2) a.dist2[e] = bd;
    if (a.gap2) a.gap2[e] = bg;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) gated += (unsigned long long)__shfl_xor((long long)gated, d);
  if ((threadIdx.x & 63) == 0) s_gated[threadIdx.x >> 6] = gated;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long tot = 0;
    for (int w = 0; w < FB / 64; ++w) tot += s_gated[w];
    if (tot) atomicAdd(reinterpret_cast<unsigned long long*>(a.w.acc + FA_GATED), tot);
  }
}

// rule 4 for the pair (x, y): does some frame hold an observation of each?  The lists are ascending in the key f * n_max + i.
__device__ __forceinline__ bool fuse_share_a_frame(const MapFuseArgs& a, int x, int y) {
  const int nx = a.l.cur[x], ny = a.l.cur[y];
  const int* kx = a.l.keys + a.l.offset(x);
  const int* ky = a.l.keys + a.l.offset(y);
  int i = 0, j = 0;
  while (i < nx && j < ny) {
    const int fx = kx[i] / a.n_max, fy = ky[j] / a.n_max;
    if (fx == fy) return true;
    if (fx < fy) ++i; else ++j;
  }
  return false;
}

__global__ __launch_bounds__(FB) void fuse_verdict_kernel(MapFuseArgs a, int* rank) {
  __shared__ int s_w[FB / 64];
  const int M = fuse_size(a);
  int n[8] = {0, 0, 0, 0, 0, 0, 0, 0};                      // by_verdict, pairs, conflicts
  for (int e = blockIdx.x * FB + threadIdx.x; e < M; e += gridDim.x * FB) {
    const int p = a.partner[e];
    int v;
    if (!a.w.fin[e]) v = FV_NOT_FINITE;
    else if (p < 0) v = FV_ALONE;
    else if (p >= M || a.partner[p] != e) v = FV_NOT_MUTUAL;      // (p < M always: a record's entry)
    else {
      const int lo = e < p ? e : p, hi = e < p ? p : e;
      if (a.veto && a.frames && a.n_max > 0 && fuse_share_a_frame(a, lo, hi)) { v = FV_CONFLICT; n[7] += e == lo; }
      else v = e == lo ? FV_SURVIVOR : FV_ABSORBED;
    }
    a.verdict[e] = v;
    rank[e] = v != FV_ABSORBED ? 1 : 0;
    if (v == FV_SURVIVOR && a.position == 1 && !a.dry_run) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        a.pts[3 * (size_t)e + k] = (float)(((double)a.pts[3 * (size_t)e + k] + (double)a.pts[3 * (size_t)p + k]) * 0.5);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) n[k] += v == k;
    n[6] += v == FV_SURVIVOR;
  }
  // whole numbers: any order gives the same tally.  One atomic per word and workgroup.
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int tot = block_sum(n[k], s_w);
    if (threadIdx.x == 0 && tot) atomicAdd(&a.w.acc[k], tot);
  }
}

__global__ __launch_bounds__(FB) void fuse_rows_kernel(MapFuseArgs a) {
  const int M = fuse_size(a);
  const int f = blockIdx.y, i = blockIdx.x * FB + threadIdx.x;
  bool hit = false;
  if (i < a.n_max && i < live_rows(a.d_n ? a.d_n + f : nullptr, a.n_max)) {
    const int e = a.l.ent[(size_t)f * a.n_max + i];
    hit = e >= 0 && e < M && a.verdict[e] == FV_ABSORBED;
    if (a.app_out && !a.dry_run) {
      const size_t o = (size_t)f * a.q_stride;
      float2* dst = reinterpret_cast<float2*>(a.app_out + o) + 5 * (size_t)i;
      if (hit) {
        const float2* src = reinterpret_cast<const float2*>(a.app) + 5 * (size_t)a.partner[e];
#pragma unroll
        for (int k = 0; k < 5; ++k) dst[k] = src[k];
      } else if (a.app_out != a.q_app) {
        const float2* src = reinterpret_cast<const float2*>(a.q_app + o) + 5 * (size_t)i;
#pragma unroll
        for (int k = 0; k < 5; ++k) dst[k] = src[k];
      }
    }
  }
  const unsigned long long m = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.w.acc[FA_ROWS], __popcll(m));
}

// voe_map_fuse_stats: int32 status, n_before, n_after, n_pairs, n_conflicts, n_rows_rewritten, by_verdict[6]; int64 n_gated
__global__ __launch_bounds__(FB) void fuse_finish_kernel(MapFuseArgs a) {
  const int M = a.cull_ctl[0];
  const int e = blockIdx.x * FB + threadIdx.x;
  if (e < M && a.verdict[e] == FV_ABSORBED) a.remap[e] = a.remap[a.partner[e]];      // (the survivor's word is written by nobody here)
  if (e != 0) return;
  int* si = static_cast<int*>(a.stats);
  si[0] = a.cull_ctl[1] != M ? 0 : 1;
  si[1] = M; si[2] = a.cull_ctl[1];
  si[3] = a.w.acc[FA_PAIRS]; si[4] = a.w.acc[FA_CONFLICTS]; si[5] = a.w.acc[FA_ROWS];
  for (int k = 0; k < 6; ++k) si[6 + k] = a.w.acc[k];
  *reinterpret_cast<unsigned long long*>(si + 12) = *reinterpret_cast<const unsigned long long*>(a.w.acc + FA_GATED);
}

MapFuseWs map_fuse_layout(void* base, int cap) {
  WsCarver c(base);
  MapFuseWs w{};
  const size_t B = (size_t)(cap > 0 ? cap : 1);
  w.grid = c.take<char>(64);
  w.box_lo = c.take<unsigned>(16);
  static_assert((sizeof(int) * FUSE_ACC) % 8 == 0, "n_gated is a 64-bit word");
  w.acc = c.take<int>(sizeof(int) * (FUSE_ACC + (size_t)FUSE_CELLS + 1));
  w.counts = w.acc ? w.acc + FUSE_ACC : nullptr;
  w.starts = c.take<int>(sizeof(int) * ((size_t)FUSE_CELLS + 1));
  w.bsum = c.take<int>(sizeof(int) * FUSE_SCAN_BLOCKS);
  w.rec = c.take<float4>(sizeof(float4) * B);
  w.fin = c.take<int32_t>(4 * B);
  w.partner = c.take<int32_t>(4 * B);
  w.verdict = c.take<int32_t>(4 * B);
  w.remap = c.take<int32_t>(4 * B);
  w.bytes = c.bytes;
  return w;
}

hipError_t launch_map_fuse(hipStream_t st, const MapFuseArgs& a, int* rank) {
  hipError_t e = hipMemsetAsync(a.w.box_lo, 0xFF, 16, st);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(a.w.acc, 0, sizeof(int) * (FUSE_ACC + (size_t)FUSE_CELLS + 1), st)) != hipSuccess) return e;
  const unsigned eb = (unsigned)(((a.bound > 0 ? a.bound : 1) + FB - 1) / FB), gb = eb < FUSE_GRID ? eb : FUSE_GRID;
  hipLaunchKernelGGL(fuse_box_kernel, dim3(gb), dim3(FB), 0, st, a);
  hipLaunchKernelGGL(fuse_grid_kernel, dim3(1), dim3(64), 0, st, a);
  hipLaunchKernelGGL(fuse_count_kernel, dim3(eb), dim3(FB), 0, st, a);
  hipLaunchKernelGGL(fuse_sums_kernel, dim3(FUSE_SCAN_BLOCKS), dim3(FB), 0, st, a);
  hipLaunchKernelGGL(fuse_starts_kernel, dim3(FUSE_SCAN_BLOCKS), dim3(FB), 0, st, a);
  hipLaunchKernelGGL(fuse_place_kernel, dim3(eb), dim3(FB), 0, st, a);
  hipLaunchKernelGGL(fuse_search_kernel, dim3(eb), dim3(FB), 0, st, a);
  if (a.frames && (e = launch_map_refine_lists(st, a.l, a.n_frames, a.n_max, a.bound)) != hipSuccess) return e;
  hipLaunchKernelGGL(fuse_verdict_kernel, dim3(gb), dim3(FB), 0, st, a, rank);
  const unsigned nb = (unsigned)((a.n_max + FB - 1) / FB);
  if (a.frames && nb > 0) hipLaunchKernelGGL(fuse_rows_kernel, dim3(nb, (unsigned)a.n_frames), dim3(FB), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_fuse_finish(hipStream_t st, const MapFuseArgs& a) {
  const unsigned eb = (unsigned)(((a.bound > 0 ? a.bound : 1) + FB - 1) / FB);
  hipLaunchKernelGGL(fuse_finish_kernel, dim3(eb), dim3(FB), 0, st, a);
  return hipGetLastError();
}

}  // namespace vo
