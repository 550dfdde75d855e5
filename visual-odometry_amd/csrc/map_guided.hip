// map_guided.hip -- voe_map_guided*: for every live row of a window of frames the nearest entry of the map AMONG THOSE THAT PROJECT,
// under the frame's pose prior, within radius_px of the row's pixel; the rows canonicalised as voe_map_nearest* leaves them (the
// rules: include/vo_hip.h, GUIDED).  map_nearest.hip is the model and the owner of what the two calls
// share: the claim / resolve and finish kernels run here unchanged, on the same best / distance / status arrays.
//
// Launches, a fixed sequence (behind a memset of the statistics).  The frames are processed in GROUPS whose records, claim words
// and cell tables fit GUIDED_GROUP_BYTES (vo_internal.h says how that number was chosen); per group, behind a memset of the cell
// counts:
//   guided_box_kernel       one workgroup per frame: the bounding box of the frame's live rows' finite pixels and its grid -- per
//                           axis nc = clamp(floor(span / R), 1, GUIDED_NC - 4) cells of width w = span / nc, >= R = 1.001 radius_px up to rounding
//                           over the box, and two more cells of that width on either side (a row within R of the box's edge then
//                           walks ring cells that hold only entries within 2 w of the box; everything further out sits in the
//                           outermost cells, which no row reaches)
//   guided_count_kernel     one lane per (entry, frame): project_point (rule 1); an entry in view adds 1 to its cell's count (an
//                           integer atomicAdd: exact in any order) and to n_in_view
//   guided_starts_kernel    one workgroup per frame: exclusive scan of the frame's <= 4096 counts: the start table, and the same
//                           numbers as the cells' cursors
//   guided_place_kernel     the same lanes, the same arithmetic: the record (u, v, entry) at the cell's cursor.  The order of the
//                           records INSIDE a cell is whatever the atomics make it; no result depends on it (ties are decided on the
//                           entry index, n_gated is a sum).
//   guided_search_kernel    one row per lane: the cells [cell(u - R), cell(u + R)] x [cell(v - R), cell(v + R)] (contiguous along
//                           v: 3 runs at most where w >= R holds), rule 2 on the record, the 40-byte appearance row of the
//                           survivors only, rule 3, best (ties: lowest entry) and second best, the ratio, the status so far, and
//                           the row's pix2
//   nearest_claim_kernel, nearest_resolve_kernel   (unique; map_nearest.hip) behind a memset of the group's claim words
// and behind the last group nearest_finish_kernel (map_nearest.hip): entry, status, distance, canonical rows, the eight counts.
//
// EXACTNESS.  The grid changes no decision:
//  * cell(x) = trunc(clamp((x - lo) * scale, 0, nc - 1)) is monotone non-decreasing in x for every lo and every scale >= 0 (cell1
//    of map_nearest.hip), float rounding is monotone, and NOTHING is dropped on account of the box: an entry in view whose pixel
//    lies outside it -- by a little, by 1e30, at +-infinity -- is clamped into a border cell, a NaN pixel into cell 0.
//  * an entry e that passes rule 2 for a row q has |u_e - u_q| < radius_px in real numbers (if |u_e - u_q| >= radius_px then
//    fl(u_e - u_q)^2 >= fl(radius_px * radius_px), and a sum of two non-negative terms rounded to nearest never falls below a
//    term), so u_q - R < u_e < u_q + R, fl(u_q - R) <= u_e <= fl(u_q + R) and cell(fl(u_q - R)) <= cell(u_e) <= cell(fl(u_q + R));
//    the same for v.  The walked rectangle holds the record whatever the box, the widths and the roundings were, also when the
//    grid is a single cell (no finite pixel, R not finite).  That the rectangle is <= 3 x 3 cells (where w >= R: nc = floor(fl(span / R)), and fl may round up to the next integer, which leaves w
//    an ulp below R; R itself lies 0.1 % above radius_px), and that the ring keeps far
//    entries out of it, is speed only.
//  * a row whose pixel is not finite gates nothing (g2 is NaN or +inf) and walks nothing.
//  * count and place project with the same instructions on the same data, so the counts add up to the records placed.
// Everything runs on global memory, as in map_nearest.hip and for its reason: rows arrive in the frame's order, not the grid's.
#include "vo_internal.h"

namespace vo {

constexpr int GB = 256;                   // threads per workgroup
static_assert(GUIDED_CELLS % GB == 0, "the scan gives every thread the same number of cells");

enum { GS_MATCHED = 0, GS_NO_ENTRY = 1, GS_AMBIGUOUS = 2, GS_DISPLACED = 3, GS_NAN_ROW = 4, GS_NOT_LIVE = 5 };      // = NS_* of map_nearest.hip

struct GuidedGrid { float lo[2], scale[2]; int nc[2]; int pad[2]; };
static_assert(sizeof(GuidedGrid) == 32, "MapGuidedWs::grids");

__device__ __forceinline__ int guided_size(const MapNearestArgs& a) {
  int M = a.hdr[0];
  M = M < a.cap ? M : a.cap;
  M = M < a.bound ? M : a.bound;
  return M > 0 ? M : 0;
}
__device__ __forceinline__ int gcell1(float x, float lo, float scale, int nc) {      // cell1 of map_nearest.hip
  float v = (x - lo) * scale;                               // monotone non-decreasing in x
  v = fminf(fmaxf(v, 0.f), (float)(nc - 1));                // NaN -> 0, +-inf clamp
  return (int)v;
}
__device__ __forceinline__ bool gfinite(float x) { return (x - x) == 0.f; }

__device__ __forceinline__ Row guided_load_row(const float* app, size_t i) {
  const float2* p = reinterpret_cast<const float2*>(app) + 5 * i;
  Row r;
#pragma unroll
  for (int k = 0; k < 5; ++k) { const float2 t = p[k]; r.v[2 * k] = t.x; r.v[2 * k + 1] = t.y; }
  return r;
}

// rule 1 for entry e in frame f: the pixel, and whether the entry is in view
__device__ __forceinline__ bool guided_project(const MapGuidedArgs& a, int f, int e, float& u, float& v) {
  CamK cam;
#pragma unroll
  for (int k = 0; k < 9; ++k) cam.K[k] = a.K[k];
  cam.rows = cam.cols = 1; cam.z_near = a.z_near; cam.z_far = a.z_far;
  const Pose T = pose_from_T16(a.T16 + 16 * (size_t)f);
  const float* p = a.pts + 3 * (size_t)e;
  float pc[3], ph[3], inv;
  (void)project_point(cam, T, p[0], p[1], p[2], u, v, pc, ph, inv);      // (its image gate is not this call's: rule 1)
  return pc[2] > 0.f && !(pc[2] > (float)a.z_far || pc[2] < (float)a.z_near);
}

__global__ __launch_bounds__(GB) void guided_box_kernel(MapGuidedArgs a, int f0) {
  __shared__ float s_lo[GB / 64][2], s_hi[GB / 64][2];
  const int f = f0 + blockIdx.x;
  const int n = live_rows(a.n.d_n ? a.n.d_n + f : nullptr, a.n.n_max);
  const float2* uv = reinterpret_cast<const float2*>(a.uv + (size_t)f * a.uv_stride);
  float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
  for (int i = threadIdx.x; i < n; i += GB) {
    const float2 p = uv[i];
    if (gfinite(p.x) && gfinite(p.y)) {
      lo[0] = fminf(lo[0], p.x); hi[0] = fmaxf(hi[0], p.x);
      lo[1] = fminf(lo[1], p.y); hi[1] = fmaxf(hi[1], p.y);
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], d)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], d)); }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6][k] = lo[k]; s_hi[threadIdx.x >> 6][k] = hi[k]; }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float R = a.radius_px * 1.001f;
  GuidedGrid g{};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    float l = s_lo[0][k], h = s_hi[0][k];
    for (int w = 1; w < GB / 64; ++w) { l = fminf(l, s_lo[w][k]); h = fmaxf(h, s_hi[w][k]); }
    const float span = h - l;
    g.lo[k] = 0.f; g.scale[k] = 0.f; g.nc[k] = 1;           // no finite pixel, an infinite span or R: one cell
    if (h >= l && span < INFINITY && R > 0.f && R < INFINITY) {
      const float sp = span > R ? span : R;                 // (a box of one pixel still gets cells of width R)
      const float q = sp / R;
      int nc = q >= (float)(GUIDED_NC - 4) ? GUIDED_NC - 4 : (int)q;
      if (nc < 1) nc = 1;
      const float w = sp / (float)nc;                       // >= R up to the rounding of q
      g.lo[k] = l - 2.f * w; g.scale[k] = (float)nc / sp; g.nc[k] = nc + 4;
    }
  }
  reinterpret_cast<GuidedGrid*>(a.w.grids)[blockIdx.x] = g;
}

__global__ __launch_bounds__(GB) void guided_count_kernel(MapGuidedArgs a, int f0) {
  const int fl = blockIdx.y, e = blockIdx.x * GB + threadIdx.x;
  bool in = false;
  if (e < guided_size(a.n)) {
    float u, v;
    in = guided_project(a, f0 + fl, e, u, v);
    if (in) {
      const GuidedGrid g = reinterpret_cast<const GuidedGrid*>(a.w.grids)[fl];
      const int c = gcell1(u, g.lo[0], g.scale[0], g.nc[0]) * g.nc[1] + gcell1(v, g.lo[1], g.scale[1], g.nc[1]);
      atomicAdd(&a.w.counts[(size_t)fl * (GUIDED_CELLS + 1) + c], 1);
    }
  }
  if (!a.stats64) return;
  const unsigned long long m = __ballot(in);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.stats64[0], (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(GB) void guided_starts_kernel(MapGuidedArgs a) {
  __shared__ int s_w[GB / 64];
  constexpr int PER = GUIDED_CELLS / GB;
  int* counts = a.w.counts + (size_t)blockIdx.x * (GUIDED_CELLS + 1);
  int* starts = a.w.starts + (size_t)blockIdx.x * (GUIDED_CELLS + 1);
  const int i0 = threadIdx.x * PER;
  int c[PER], mine = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) { c[k] = counts[i0 + k]; mine += c[k]; }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int run = inc - mine;
#pragma unroll
  for (int w = 0; w < GB / 64; ++w) if (w < wave) run += s_w[w];
#pragma unroll
  for (int k = 0; k < PER; ++k) { starts[i0 + k] = run; counts[i0 + k] = run; run += c[k]; }
  if (threadIdx.x == GB - 1) starts[GUIDED_CELLS] = run;    // the records in all
}

__global__ __launch_bounds__(GB) void guided_place_kernel(MapGuidedArgs a, int f0) {
  const int fl = blockIdx.y, e = blockIdx.x * GB + threadIdx.x;
  if (e >= guided_size(a.n)) return;
  float u, v;
  if (!guided_project(a, f0 + fl, e, u, v)) return;
  const GuidedGrid g = reinterpret_cast<const GuidedGrid*>(a.w.grids)[fl];
  const int c = gcell1(u, g.lo[0], g.scale[0], g.nc[0]) * g.nc[1] + gcell1(v, g.lo[1], g.scale[1], g.nc[1]);
  const int pos = atomicAdd(&a.w.counts[(size_t)fl * (GUIDED_CELLS + 1) + c], 1);
  if (pos >= 0 && pos < a.n.cap) a.w.rec[(size_t)fl * a.n.cap + pos] = GuidedRec{u, v, e};      // (always: the counts add up to <= size)
}

__global__ __launch_bounds__(GB) void guided_search_kernel(MapGuidedArgs a, int f0) {
  const int fl = blockIdx.y, f = f0 + fl, i = blockIdx.x * GB + threadIdx.x;
  unsigned long long gated = 0;
  if (i < a.n.n_max) {
    const size_t o = (size_t)f * a.n.n_max + i;
    const int n = live_rows(a.n.d_n ? a.n.d_n + f : nullptr, a.n.n_max);
    int st = GS_NOT_LIVE, bi = -1;
    float bd = INFINITY, bg = INFINITY;
    if (i < n) {
      const Row q = guided_load_row(a.n.q_app + (size_t)f * a.n.q_stride, (size_t)i);
      const float2 px = reinterpret_cast<const float2*>(a.uv + (size_t)f * a.uv_stride)[i];
      float d2nd = INFINITY;
      if (gfinite(px.x) && gfinite(px.y)) {
        const GuidedGrid g = reinterpret_cast<const GuidedGrid*>(a.w.grids)[fl];
        const float R = a.radius_px * 1.001f, rp2 = a.radius_px * a.radius_px, r2 = a.n.radius * a.n.radius;
        const int u0 = gcell1(px.x - R, g.lo[0], g.scale[0], g.nc[0]), u1 = gcell1(px.x + R, g.lo[0], g.scale[0], g.nc[0]);
        const int v0 = gcell1(px.y - R, g.lo[1], g.scale[1], g.nc[1]), v1 = gcell1(px.y + R, g.lo[1], g.scale[1], g.nc[1]);
        const int* starts = a.w.starts + (size_t)fl * (GUIDED_CELLS + 1);
        const GuidedRec* rec = a.w.rec + (size_t)fl * a.n.cap;
        for (int cu = u0; cu <= u1; ++cu) {
          const int p1 = starts[cu * g.nc[1] + v1 + 1];
          for (int p = starts[cu * g.nc[1] + v0]; p < p1; ++p) {
            const GuidedRec t = rec[p];
            // rule 2: unfused, left to right
            const float du = t.u - px.x, dv = t.v - px.y;
            const float g2 = du * du + dv * dv;
            if (!(g2 < rp2)) continue;
            ++gated;
            const Row w = guided_load_row(a.n.app, (size_t)t.e);
            // rule 3 = NEAREST's rule 1 (map_nearest.hip, the decision itself)
            float d = w.v[0] - q.v[0];
            float s = d * d;
#pragma unroll
            for (int k = 1; k < 10; ++k) { d = w.v[k] - q.v[k]; s += d * d; }
            if (!(s < r2)) continue;
            if (s < bd || (s == bd && t.e < bi)) { d2nd = bd; bd = s; bi = t.e; bg = g2; }
            else if (s < d2nd) d2nd = s;
          }
        }
      }
      if (map_row_has_nan(q)) st = GS_NAN_ROW;              // (no candidate: every d2 with a NaN is a NaN)
      else if (bi < 0) st = GS_NO_ENTRY;
      else {
        st = GS_MATCHED;
        if (a.n.ratio != 0.f && d2nd < INFINITY && !(bd < (a.n.ratio * a.n.ratio) * d2nd)) st = GS_AMBIGUOUS;
      }
    }
    a.n.w.best[o] = bi;
    a.n.w.d2[o] = __float_as_uint(bd);
    a.n.w.st[o] = st;
    if (a.pix2) a.pix2[o] = bg;                             // +inf unless the row has a best candidate; uniqueness changes neither
  }
  if (!a.stats64) return;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) gated += __shfl_xor(gated, d);
  if ((threadIdx.x & 63) == 0 && gated) atomicAdd(&a.stats64[1], gated);
}

static size_t guided_group(int n_frames, int cap) {
  const size_t per = (sizeof(GuidedRec) + sizeof(unsigned long long)) * (size_t)(cap > 0 ? cap : 1) + 2 * sizeof(int) * (GUIDED_CELLS + 1);
  size_t g = GUIDED_GROUP_BYTES / per;
  return g < 1 ? 1 : (g > (size_t)n_frames ? (size_t)n_frames : g);
}

MapGuidedWs map_guided_layout(void* base, int n_frames, int n_max, int cap, bool unique) {
  WsCarver c(base);
  MapGuidedWs w{};
  const size_t rows = (size_t)n_frames * (size_t)(n_max > 0 ? n_max : 0), g = guided_group(n_frames, cap);
  w.grids = c.take<char>(sizeof(GuidedGrid) * g);
  w.counts = c.take<int>(sizeof(int) * (GUIDED_CELLS + 1) * g);
  w.starts = c.take<int>(sizeof(int) * (GUIDED_CELLS + 1) * g);
  w.rec = c.take<GuidedRec>(sizeof(GuidedRec) * g * (size_t)cap);
  w.n.best = c.take<int32_t>(sizeof(int32_t) * rows);
  w.n.d2 = c.take<uint32_t>(sizeof(uint32_t) * rows);
  w.n.st = c.take<int32_t>(sizeof(int32_t) * rows);
  w.n.group = (int)g;
  w.n.claim = unique && rows > 0 ? c.take<unsigned long long>(sizeof(unsigned long long) * g * (size_t)cap) : nullptr;
  w.bytes = w.n.bytes = c.bytes;
  return w;
}

hipError_t launch_map_guided(hipStream_t st, const MapGuidedArgs& a) {
  hipError_t e;
  if (a.n.stats && (e = hipMemsetAsync(a.n.stats, 0, 48, st)) != hipSuccess) return e;
  const unsigned eb = (unsigned)(((a.n.bound > 0 ? a.n.bound : 1) + GB - 1) / GB), nb = (unsigned)((a.n.n_max + GB - 1) / GB);
  const int group = a.n.w.group;
  for (int f0 = 0; f0 < a.n.n_frames; f0 += group) {        // (n_max == 0: the index is still built, n_in_view is a fact of the map)
    const int gf = a.n.n_frames - f0 < group ? a.n.n_frames - f0 : group;
    if ((e = hipMemsetAsync(a.w.counts, 0, sizeof(int) * (GUIDED_CELLS + 1) * (size_t)gf, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(guided_box_kernel, dim3((unsigned)gf), dim3(GB), 0, st, a, f0);
    hipLaunchKernelGGL(guided_count_kernel, dim3(eb, (unsigned)gf), dim3(GB), 0, st, a, f0);
    hipLaunchKernelGGL(guided_starts_kernel, dim3((unsigned)gf), dim3(GB), 0, st, a);
    hipLaunchKernelGGL(guided_place_kernel, dim3(eb, (unsigned)gf), dim3(GB), 0, st, a, f0);
    if (nb == 0) continue;
    hipLaunchKernelGGL(guided_search_kernel, dim3(nb, (unsigned)gf), dim3(GB), 0, st, a, f0);
    if (a.n.unique && a.n.w.claim)
      if ((e = launch_nearest_unique(st, a.n, f0, gf)) != hipSuccess) return e;
  }
  return launch_nearest_finish(st, a.n);
}

}  // namespace vo
