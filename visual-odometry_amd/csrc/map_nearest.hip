// map_nearest.hip -- voe_map_nearest*: for every live row of a window of frames the NEAREST entry of the map within a radius, and
// the rows canonicalised (the rules: include/vo_hip.h, NEAREST).  The matcher's cell-hash search
// (match.hip) is the model: a 4-D grid over four appearance components, an 8-bit x 4 filter word per entry, the decision on the
// full float row.  Here ONE index of the map serves every frame of the call, it is built by the call and kept by none.
//
// Launches, a fixed sequence (behind a memset of the cell counts and of the statistics):
//   nearest_grid_kernel     one workgroup: bounds of a strided sample of <= 2048 entries, the four components with the largest
//                           spreads (the matcher's choice), nc_k = clamp(floor(spread_k / R), 1, lim) cells of width >= R =
//                           1.001 r each, lim = the smallest of 2 .. 32 with lim^4 >= size (about one entry per cell where the
//                           spreads allow it), and the filter's scale and bound T = floor(2 R s) + 7.
//   nearest_count_kernel    one entry per lane: an integer atomicAdd on its cell's count (a sum: exact in any order)
//   nearest_sums_kernel     the counts' sums per block of 2048 cells
//   nearest_starts_kernel   every block adds up the sums in front of it and scans its own cells: the start table, and the same
//                           numbers as the cells' cursors
//   nearest_place_kernel    one entry per lane: its 8-byte record (filter word, entry) at the cell's cursor.  The order of the
//                           records INSIDE a cell is whatever the atomics make it; no result depends on it (ties are decided on
//                           the entry index, below).
//   nearest_search_kernel   one query per lane over all frames: the cells [cell(q - R), cell(q + R)] per component (<= 3 each
//                           by the matcher's argument, <= 81 in all, contiguous along the last component: <= 27 runs), one
//                           v_sad_u8 per record against the query's word, and every survivor's full row through rule 1.  Best
//                           (ties: lowest entry) and second best, rule 3, the status so far.
//   nearest_claim_kernel, nearest_resolve_kernel   (unique) per group of frames whose claim words fit 256 MiB, behind a memset
//                           of the words: an integer atomicMin of (distance bits, row) per (frame, entry) -- non-negative float
//                           bits order as integers --, then the rows that did not win become DISPLACED.
//   nearest_finish_kernel   entry, status, distance, the canonical row, the statistics (integer atomicAdds of wave counts)
//
// EXACTNESS.  Pruning changes no decision:
//  * cell(x) = trunc(clamp((x - lo) * scale, 0, nc - 1)) is monotone non-decreasing in x for every lo and every scale >= 0, and
//    float rounding is monotone.  An entry t that passes rule 2 has, in every component, |t - q| < r in real numbers (if
//    |t - q| >= r then fl(t - q)^2 >= fl(r * r), and a sum of non-negative terms rounded to nearest never falls below a term), so
//    q - R < t < q + R, fl(q - R) <= t <= fl(q + R) and cell(fl(q - R)) <= cell(t) <= cell(fl(q + R)): the box holds it whatever
//    the sample, the bounds and the roundings were.  (That the box is <= 3 cells wide is the matcher's argument and only speed.)
//  * the filter word and its bound are the matcher's, formula for formula (match.hip, "The filter"): SAD > T proves that the
//    entry cannot pass; any lo / scale only changes how many survivors reach the decision.
//  * rows with a NaN are NAN_ROW and rows with an infinity NO_ENTRY before any cell is formed: no arithmetic on them can pass.
// Everything runs on global memory: records and start table of a query's box are a few hundred bytes that neighbouring lanes do
// not share (queries arrive in the frame's order, not the grid's), so there is no LDS staging and hence no staging budget to fall
// back from.
#include "vo_internal.h"

namespace vo {

constexpr int NB = 256;                   // threads per workgroup
constexpr int NSAMPLE = 2048;             // entries that define the grid's bounds
constexpr int NSCAN = 2048;               // cells per block of the scan
constexpr int NSCAN_BLOCKS = (NEAREST_CELLS + 1 + NSCAN - 1) / NSCAN;
static_assert(NSCAN_BLOCKS <= 1024, "bsum holds 1024 sums");

enum { NS_MATCHED = 0, NS_NO_ENTRY = 1, NS_AMBIGUOUS = 2, NS_DISPLACED = 3, NS_NAN_ROW = 4, NS_NOT_LIVE = 5 };

struct NearestGrid {
  int dim[4]; float lo[4], scale[4]; int nc[4];
  float R;
  float qlo[4], qscale; int T;            // filter words: quant8 of components 0..3
  int n_cells, M;
};
static_assert(sizeof(NearestGrid) <= 256, "MapNearestWs::grid");

__device__ __forceinline__ int nearest_size(const MapNearestArgs& a) {
  int M = a.hdr[0];
  M = M < a.cap ? M : a.cap;
  M = M < a.bound ? M : a.bound;
  return M > 0 ? M : 0;
}

__device__ __forceinline__ int cell1(float x, float lo, float scale, int nc) {
  float v = (x - lo) * scale;                               // monotone non-decreasing in x
  v = fminf(fmaxf(v, 0.f), (float)(nc - 1));                // NaN -> 0, +-inf clamp
  return (int)v;
}
__device__ __forceinline__ unsigned quant8(float x, float lo, float scale) {      // match.hip
  float v = (x - lo) * scale;
  v = fminf(fmaxf(v, 0.f), 255.f);
  return (unsigned)v;
}
__device__ __forceinline__ unsigned filter_word(const float* row, const NearestGrid& g) {
  return quant8(row[0], g.qlo[0], g.qscale) | (quant8(row[1], g.qlo[1], g.qscale) << 8) | (quant8(row[2], g.qlo[2], g.qscale) << 16) |
         (quant8(row[3], g.qlo[3], g.qscale) << 24);
}
__device__ __forceinline__ int cell_of(const float* row, const NearestGrid& g) {
  int c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) c = c * g.nc[j] + cell1(row[g.dim[j]], g.lo[j], g.scale[j], g.nc[j]);
  return c;
}
__device__ __forceinline__ bool finite_f(float x) { return (x - x) == 0.f; }

__device__ __forceinline__ Row nearest_load_row(const float* app, size_t i) {
  const float2* p = reinterpret_cast<const float2*>(app) + 5 * i;
  Row r;
#pragma unroll
  for (int k = 0; k < 5; ++k) { const float2 t = p[k]; r.v[2 * k] = t.x; r.v[2 * k + 1] = t.y; }
  return r;
}

__global__ __launch_bounds__(NB) void nearest_grid_kernel(MapNearestArgs a) {
  __shared__ float s_lo[NB / 64][10], s_hi[NB / 64][10];
  __shared__ float s_span[10], s_l[10];
  const int M = nearest_size(a);
  const int ns = M < NSAMPLE ? M : NSAMPLE;
  const int stride = ns > 0 ? M / ns : 1;
  float lo[10], hi[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
  for (int s = threadIdx.x; s < ns; s += NB) {
    const Row r = nearest_load_row(a.app, (size_t)s * stride);
#pragma unroll
    for (int k = 0; k < 10; ++k)
      if (finite_f(r.v[k])) { lo[k] = fminf(lo[k], r.v[k]); hi[k] = fmaxf(hi[k], r.v[k]); }
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], d)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], d)); }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6][k] = lo[k]; s_hi[threadIdx.x >> 6][k] = hi[k]; }
  }
  __syncthreads();
  if (threadIdx.x < 10) {
    const int k = threadIdx.x;
    float l = s_lo[0][k], h = s_hi[0][k];
    for (int w = 1; w < NB / 64; ++w) { l = fminf(l, s_lo[w][k]); h = fmaxf(h, s_hi[w][k]); }
    const float sp = h - l;
    s_span[k] = (h >= l && sp < INFINITY) ? sp : -1.f;      // empty / infinite ranges rank last
    s_l[k] = h >= l ? l : 0.f;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  // the four largest spans, ties to the lower component; the four largest among components 4..9 when none of them is flatter
  // than half its counterpart, so that the filter on components 0..3 keeps its selectivity (match.hip, make_cell_params_wave)
  int all4[4], tail4[4];
  unsigned used_all = 0, used_tail = 0;
  bool tail_ok = true;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int ba = -1, bt = -1;
    for (int k = 0; k < 10; ++k) {
      if (!((used_all >> k) & 1u) && (ba < 0 || s_span[k] > s_span[ba])) ba = k;
      if (k >= 4 && !((used_tail >> k) & 1u) && (bt < 0 || s_span[k] > s_span[bt])) bt = k;
    }
    used_all |= 1u << ba; used_tail |= 1u << bt;
    all4[j] = ba; tail4[j] = bt;
    tail_ok = tail_ok && s_span[bt] >= 0.5f * s_span[ba];
  }
  int lim = 2;
  while (lim < NEAREST_NC && (long long)lim * lim * lim * lim < (long long)M) ++lim;
  NearestGrid g;
  g.R = a.radius * 1.001f;
  int cells = 1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = tail_ok ? tail4[j] : all4[j];
    const float sp = s_span[k];
    int nc = 1;
    if (sp > 0.f && g.R > 0.f) {
      const float f = sp / g.R;
      nc = f >= (float)lim ? lim : (int)f;
      if (nc < 1) nc = 1;
    }
    g.dim[j] = k; g.lo[j] = s_l[k]; g.nc[j] = nc;
    g.scale[j] = sp > 0.f ? (float)nc / sp : 0.f;           // cell width sp / nc >= R
    cells *= nc;
  }
  float wide = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    g.qlo[k] = s_span[k] >= 0.f ? s_l[k] : 0.f;
    wide = s_span[k] > wide ? s_span[k] : wide;
  }
  g.qscale = wide > 0.f ? 255.f / wide : 0.f;
  {
    const float t = 2.f * g.R * g.qscale;                   // NaN / inf / huge -> every word passes (1020 is the largest SAD)
    g.T = (t >= 0.f && t < 1000.f) ? (int)t + 7 : 1020;
  }
  g.n_cells = cells; g.M = M;
  *reinterpret_cast<NearestGrid*>(a.w.grid) = g;
}

__global__ __launch_bounds__(NB) void nearest_count_kernel(MapNearestArgs a) {
  const NearestGrid& g = *reinterpret_cast<const NearestGrid*>(a.w.grid);
  const int e = blockIdx.x * NB + threadIdx.x;
  if (e >= g.M) return;
  atomicAdd(&a.w.counts[cell_of(a.app + 10 * (size_t)e, g)], 1);
}

__global__ __launch_bounds__(NB) void nearest_sums_kernel(MapNearestArgs a) {
  __shared__ int s_w[NB / 64];
  const int n_cells = reinterpret_cast<const NearestGrid*>(a.w.grid)->n_cells;
  const int i0 = blockIdx.x * NSCAN + threadIdx.x * (NSCAN / NB);
  int v = 0;
#pragma unroll
  for (int k = 0; k < NSCAN / NB; ++k) v += i0 + k < n_cells ? a.w.counts[i0 + k] : 0;
  const int tot = block_sum(v, s_w);
  if (threadIdx.x == 0) a.w.bsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(NB) void nearest_starts_kernel(MapNearestArgs a) {
  __shared__ int s_w[NB / 64];
  const int n_cells = reinterpret_cast<const NearestGrid*>(a.w.grid)->n_cells;
  if ((int)blockIdx.x * NSCAN > n_cells) return;            // (the whole workgroup)
  int pre = 0;
  for (int j = threadIdx.x; j < (int)blockIdx.x; j += NB) pre += a.w.bsum[j];
  pre = block_sum(pre, s_w);
  const int i0 = blockIdx.x * NSCAN + threadIdx.x * (NSCAN / NB);
  int c[NSCAN / NB], mine = 0;
#pragma unroll
  for (int k = 0; k < NSCAN / NB; ++k) { c[k] = i0 + k < n_cells ? a.w.counts[i0 + k] : 0; mine += c[k]; }
  // exclusive scan of `mine` over the workgroup
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
  __syncthreads();
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int run = pre + inc - mine;
#pragma unroll
  for (int w = 0; w < NB / 64; ++w) if (w < wave) run += s_w[w];
#pragma unroll
  for (int k = 0; k < NSCAN / NB; ++k) {
    if (i0 + k <= n_cells) a.w.starts[i0 + k] = run;        // [n_cells]: the records in all
    if (i0 + k < n_cells) a.w.counts[i0 + k] = run;         // the cell's cursor
    run += c[k];
  }
}

__global__ __launch_bounds__(NB) void nearest_place_kernel(MapNearestArgs a) {
  const NearestGrid& g = *reinterpret_cast<const NearestGrid*>(a.w.grid);
  const int e = blockIdx.x * NB + threadIdx.x;
  if (e >= g.M) return;
  const float* row = a.app + 10 * (size_t)e;
  const int pos = atomicAdd(&a.w.counts[cell_of(row, g)], 1);
  if (pos >= 0 && pos < g.M) a.w.rec[pos] = make_uint2(filter_word(row, g), (unsigned)e);      // (always: the counts add up to M)
}

__global__ __launch_bounds__(NB) void nearest_search_kernel(MapNearestArgs a) {
  const int f = blockIdx.y, i = blockIdx.x * NB + threadIdx.x;
  if (i >= a.n_max) return;
  const size_t o = (size_t)f * a.n_max + i;
  const int n = live_rows(a.d_n ? a.d_n + f : nullptr, a.n_max);
  int st = NS_NOT_LIVE, bi = -1;
  float bd = INFINITY;
  if (i < n) {
    const float* qrow = a.q_app + (size_t)f * a.q_stride + 10 * (size_t)i;
    const Row q = nearest_load_row(a.q_app + (size_t)f * a.q_stride, (size_t)i);
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 10; ++k) fin = fin && finite_f(q.v[k]);
    if (map_row_has_nan(q)) st = NS_NAN_ROW;
    else if (!fin) st = NS_NO_ENTRY;                        // an infinity: no difference with it is below r
    else {
      const NearestGrid g = *reinterpret_cast<const NearestGrid*>(a.w.grid);
      const float r2 = a.radius * a.radius;
      const unsigned qw = filter_word(qrow, g), T = (unsigned)g.T;
      int lo[4], hi[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x = qrow[g.dim[j]];
        lo[j] = cell1(x - g.R, g.lo[j], g.scale[j], g.nc[j]);
        hi[j] = cell1(x + g.R, g.lo[j], g.scale[j], g.nc[j]);
      }
      float d2nd = INFINITY;
      for (int c0 = lo[0]; c0 <= hi[0]; ++c0)
        for (int c1 = lo[1]; c1 <= hi[1]; ++c1)
          for (int c2 = lo[2]; c2 <= hi[2]; ++c2) {
            const int base = ((c0 * g.nc[1] + c1) * g.nc[2] + c2) * g.nc[3];
            const int p1 = a.w.starts[base + hi[3] + 1];
            for (int p = a.w.starts[base + lo[3]]; p < p1; ++p) {
              const uint2 rec = a.w.rec[p];
              if (__builtin_amdgcn_sad_u8(rec.x, qw, 0u) > T) continue;
              const Row t = nearest_load_row(a.app, (size_t)rec.y);
              // the decision itself: the unfused left-to-right sum (rule 1; match.hip)
              float d = t.v[0] - q.v[0];
              float s = d * d;
#pragma unroll
              for (int k = 1; k < 10; ++k) { d = t.v[k] - q.v[k]; s += d * d; }
              if (!(s < r2)) continue;
              const int e = (int)rec.y;
              if (s < bd || (s == bd && e < bi)) { d2nd = bd; bd = s; bi = e; }
              else if (s < d2nd) d2nd = s;
            }
          }
      if (bi < 0) st = NS_NO_ENTRY;
      else {
        st = NS_MATCHED;
        if (a.ratio != 0.f && d2nd < INFINITY && !(bd < (a.ratio * a.ratio) * d2nd)) st = NS_AMBIGUOUS;
      }
    }
  }
  a.w.best[o] = bi;
  a.w.d2[o] = __float_as_uint(bd);
  a.w.st[o] = st;
}

// frames [f0, f0 + group) of the call: the claim words are [frame - f0][cap]
__global__ __launch_bounds__(NB) void nearest_claim_kernel(MapNearestArgs a, int f0) {
  const int f = f0 + blockIdx.y, i = blockIdx.x * NB + threadIdx.x;
  if (f >= a.n_frames || i >= a.n_max) return;
  const size_t o = (size_t)f * a.n_max + i;
  if (a.w.st[o] != NS_MATCHED) return;
  const int e = a.w.best[o];
  if (e < 0 || e >= a.cap) return;                          // (never: a best entry is below the size)
  atomicMin(&a.w.claim[(size_t)blockIdx.y * a.cap + e], ((unsigned long long)a.w.d2[o] << 32) | (unsigned)i);
}
__global__ __launch_bounds__(NB) void nearest_resolve_kernel(MapNearestArgs a, int f0) {
  const int f = f0 + blockIdx.y, i = blockIdx.x * NB + threadIdx.x;
  if (f >= a.n_frames || i >= a.n_max) return;
  const size_t o = (size_t)f * a.n_max + i;
  if (a.w.st[o] != NS_MATCHED) return;
  const int e = a.w.best[o];
  if (e < 0 || e >= a.cap) return;
  if (a.w.claim[(size_t)blockIdx.y * a.cap + e] != (((unsigned long long)a.w.d2[o] << 32) | (unsigned)i)) a.w.st[o] = NS_DISPLACED;
}

__global__ __launch_bounds__(NB) void nearest_finish_kernel(MapNearestArgs a) {
  const int f = blockIdx.y, i = blockIdx.x * NB + threadIdx.x;
  int st = -1;
  if (i < a.n_max) {
    const size_t o = (size_t)f * a.n_max + i;
    st = a.w.st[o];
    const int e = a.w.best[o];
    const bool has = st == NS_MATCHED || st == NS_AMBIGUOUS || st == NS_DISPLACED;
    a.entry[o] = st == NS_MATCHED ? e : -1;
    if (a.status) a.status[o] = st;
    if (a.dist2) a.dist2[o] = has ? __uint_as_float(a.w.d2[o]) : INFINITY;
    if (a.app_out && st != NS_NOT_LIVE) {
      Row r = st == NS_MATCHED ? nearest_load_row(a.app, (size_t)e) : nearest_load_row(a.q_app + (size_t)f * a.q_stride, (size_t)i);
      if (st == NS_AMBIGUOUS || st == NS_DISPLACED) r.v[0] = __uint_as_float(0x7FC00000u);
      float2* p = reinterpret_cast<float2*>(a.app_out + (size_t)f * a.q_stride) + 5 * (size_t)i;
#pragma unroll
      for (int k = 0; k < 5; ++k) p[k] = make_float2(r.v[2 * k], r.v[2 * k + 1]);
    }
  }
  if (!a.stats) return;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { a.stats[0] = a.n_frames; a.stats[1] = nearest_size(a); }
  // [2] live [3] matched [4] no entry [5] ambiguous [6] displaced [7] NaN: sums of integers, exact in any order
  const int word[6] = {-1, NS_MATCHED, NS_NO_ENTRY, NS_AMBIGUOUS, NS_DISPLACED, NS_NAN_ROW};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const unsigned long long m = __ballot(k == 0 ? (st >= 0 && st != NS_NOT_LIVE) : st == word[k]);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.stats[2 + k], __popcll(m));
  }
}

MapNearestWs map_nearest_layout(void* base, int n_frames, int n_max, int cap, bool unique) {
  WsCarver c(base);
  MapNearestWs w{};
  const size_t rows = (size_t)n_frames * (size_t)(n_max > 0 ? n_max : 0);
  w.grid = c.take<char>(256);
  w.counts = c.take<int>(sizeof(int) * (NEAREST_CELLS + 1));
  w.starts = c.take<int>(sizeof(int) * (NEAREST_CELLS + 1));
  w.bsum = c.take<int>(sizeof(int) * 1024);
  w.rec = c.take<uint2>(sizeof(uint2) * (size_t)cap);
  w.best = c.take<int32_t>(sizeof(int32_t) * rows);
  w.d2 = c.take<uint32_t>(sizeof(uint32_t) * rows);
  w.st = c.take<int32_t>(sizeof(int32_t) * rows);
  size_t g = NEAREST_CLAIM_BYTES / (sizeof(unsigned long long) * (size_t)(cap > 0 ? cap : 1));
  g = g < 1 ? 1 : (g > (size_t)n_frames ? (size_t)n_frames : g);
  w.group = (int)g;
  w.claim = unique && rows > 0 ? c.take<unsigned long long>(sizeof(unsigned long long) * g * (size_t)cap) : nullptr;
  w.bytes = c.bytes;
  return w;
}

// what voe_map_guided* (map_guided.hip) shares with this call, kernel for kernel: uniqueness over the frames [f0, f0 + gf) of a.w
// (a memset of the claim words, claim, resolve), and the finish over all frames
hipError_t launch_nearest_unique(hipStream_t st, const MapNearestArgs& a, int f0, int gf) {
  const unsigned nb = (unsigned)((a.n_max + NB - 1) / NB);
  hipError_t e = hipMemsetAsync(a.w.claim, 0xFF, sizeof(unsigned long long) * (size_t)gf * (size_t)a.cap, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(nearest_claim_kernel, dim3(nb, (unsigned)gf), dim3(NB), 0, st, a, f0);
  hipLaunchKernelGGL(nearest_resolve_kernel, dim3(nb, (unsigned)gf), dim3(NB), 0, st, a, f0);
  return hipSuccess;
}
hipError_t launch_nearest_finish(hipStream_t st, const MapNearestArgs& a) {
  const unsigned nb = (unsigned)((a.n_max + NB - 1) / NB);
  hipLaunchKernelGGL(nearest_finish_kernel, dim3(nb > 0 ? nb : 1, (unsigned)a.n_frames), dim3(NB), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_nearest(hipStream_t st, const MapNearestArgs& a) {
  hipError_t e = hipMemsetAsync(a.w.counts, 0, sizeof(int) * (NEAREST_CELLS + 1), st);
  if (e != hipSuccess) return e;
  if (a.stats && (e = hipMemsetAsync(a.stats, 0, 32, st)) != hipSuccess) return e;
  const unsigned eb = (unsigned)(((a.bound > 0 ? a.bound : 1) + NB - 1) / NB), nb = (unsigned)((a.n_max + NB - 1) / NB);
  hipLaunchKernelGGL(nearest_grid_kernel, dim3(1), dim3(NB), 0, st, a);
  hipLaunchKernelGGL(nearest_count_kernel, dim3(eb), dim3(NB), 0, st, a);
  hipLaunchKernelGGL(nearest_sums_kernel, dim3(NSCAN_BLOCKS), dim3(NB), 0, st, a);
  hipLaunchKernelGGL(nearest_starts_kernel, dim3(NSCAN_BLOCKS), dim3(NB), 0, st, a);
  hipLaunchKernelGGL(nearest_place_kernel, dim3(eb), dim3(NB), 0, st, a);
  if (nb > 0) {
    hipLaunchKernelGGL(nearest_search_kernel, dim3(nb, (unsigned)a.n_frames), dim3(NB), 0, st, a);
    if (a.unique && a.w.claim)
      for (int f0 = 0; f0 < a.n_frames; f0 += a.w.group) {
        const int gf = a.n_frames - f0 < a.w.group ? a.n_frames - f0 : a.w.group;
        if ((e = launch_nearest_unique(st, a, f0, gf)) != hipSuccess) return e;
      }
  }
  return launch_nearest_finish(st, a);
}

}  // namespace vo
