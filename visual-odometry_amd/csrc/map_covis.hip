// map_covis.hip -- the covisibility of frames (voe_map_covis*) and the window chosen from it (voe_map_window*).  The rules are
// those of include/vo_map_covis.h; the addressing, the tile numbering and the rank key are the inline functions of
// covis_rules.h.  Everything here is an integer: every sum is exact in any order, and the file forms no real number.
// Launches of voe_map_covis*, behind the lookup (which wrote the entry of every query position) and a memset of the bit rows:
//   covis_bits_kernel      one thread per (frame, position): an integer atomicOr of the hit's bit.  An OR does not depend on the
//                          order, so this is the one place an atomic is in order.
//   covis_count_kernel     (when counts are wanted) C = B B^T with popcount(x & y) in place of the product.  One workgroup owns a
//                          tile of 32 x 32 frame pairs; only the tiles on or above the diagonal are launched and the others are
//                          mirrored on the store.  The workgroup walks the words in chunks of 64, staged in LDS (two panels of
//                          32 rows, 17 KiB together) while the next chunk is already on its way into registers: a word of B is
//                          read from memory once per tile it takes part in, not once per pair.  Each of the four waves covers the
//                          WHOLE tile -- every lane keeps 4 x 4 pair sums in registers -- for a quarter of every chunk's words,
//                          and the four shares are added through LDS at the end.  A tile's sums are complete within its
//                          workgroup: nothing is added up between workgroups, no atomics, no spinning.
//   covis_rowpop_kernel    one workgroup per frame: the entries it sees (the diagonal), by an integer tree
//   covis_union_kernel     one thread per word: the OR over the frames, its population count summed per workgroup
//   covis_stats_kernel     one workgroup: the five statistics
// Launches of voe_map_window*:
//   window_count_kernel    one workgroup per frame: c(g), the common bits with row query
//   window_free_kernel     one workgroup: the candidates ranked by counting rank on the key (count, frame); the free frames
//   window_union_kernel    one thread per word: U, the OR of the free frames' rows; its population count per workgroup
//   window_count_kernel    again, against U: s(h)
//   window_fixed_kernel    one workgroup: the fixed candidates ranked, the fixed frames, every output and the statistics
#include "vo_internal.h"
#include "covis_rules.h"

namespace vo {

constexpr int VB = 256;                   // threads per workgroup
constexpr int VR = 1024;                  // threads of the two ranking workgroups
constexpr int VT = COVIS_TILE;            // frames along a tile's edge
constexpr int VW = COVIS_CHUNK;           // words per staged chunk
constexpr int VS = VW + 2;                // a staged row's stride in words: 33 pairs, odd, so the 8 rows a wave reads at one pair
                                          // index fall into 8 different pairs of banks
constexpr int VA = 4;                     // pair sums per thread along each edge
constexpr int VK = VB / 64;               // waves of a workgroup: each counts its share of a chunk's words for the whole tile
constexpr int VL = VT * VW / VB;          // words of each panel a thread stages per chunk
constexpr int MAX_F = 4096;               // VOE_MAP_COVIS_MAX_FRAMES
static_assert(VT == 8 * VA, "a tile is one wave: 8 x 8 lanes of VA x VA pairs");
static_assert(VW % (2 * VK) == 0 && (VT * VW) % VB == 0 && VB % VW == 0, "the staging loop deals whole rows of a chunk; a wave takes whole pairs of words");
static_assert((VK - 1) * VA * VA * 64 <= 2 * VT * VS, "the waves' sums fit the staging area");

enum { WR_OUTSIDE = 0, WR_FREE = 1, WR_FIXED = 2 };
enum { WS_OK = 0, WS_NO_FIXED = 1, WS_QUERY_UNSEEN = 2 };

__global__ __launch_bounds__(VB) void covis_bits_kernel(MapCovisArgs a) {
  const int f = blockIdx.y, i = blockIdx.x * VB + threadIdx.x;
  if (i >= live_rows(a.d_n ? a.d_n + f : nullptr, a.n_max)) return;
  int M = a.hdr[0];
  M = M < a.cap ? M : a.cap;
  const int e = a.w.ent[(size_t)f * a.n_max + i];
  if (e < 0 || e >= M || covis_word(e) >= a.n_words) return;          // (the lookup returns entries below the size)
  atomicOr(a.bits + covis_row(f, a.n_words) + covis_word(e), covis_bit(e));
}

__global__ __launch_bounds__(VB) void covis_count_kernel(MapCovisArgs a, int T) {
  __shared__ uint32_t s_all[2 * VT * VS];
  uint32_t* sA = s_all;
  uint32_t* sB = s_all + VT * VS;
  int ti, tj;
  covis_tile(blockIdx.x, T, &ti, &tj);
  const int f0 = ti * VT, g0 = tj * VT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tx = lane & 7, ty = lane >> 3;                    // a wave covers the whole tile: 8 x 8 lanes of VA x VA pairs
  const int lw = threadIdx.x % VW, lr = threadIdx.x / VW;    // the word and the first row this thread stages
  int acc[VA][VA];
#pragma unroll
  for (int i = 0; i < VA; ++i)
#pragma unroll
    for (int j = 0; j < VA; ++j) acc[i][j] = 0;
  uint32_t ra[VL], rb[VL];                                    // the next chunk, on its way from memory while this one is counted
  auto fetch = [&](int w0) {
    const int w = w0 + lw;
#pragma unroll
    for (int k = 0; k < VL; ++k) {
      const int f = f0 + lr + k * (VB / VW), g = g0 + lr + k * (VB / VW);
      ra[k] = (f < a.n_frames && w < a.n_words) ? a.bits[covis_row(f, a.n_words) + w] : 0u;
      rb[k] = (g < a.n_frames && w < a.n_words) ? a.bits[covis_row(g, a.n_words) + w] : 0u;
    }
  };
  fetch(0);
  for (int w0 = 0; w0 < a.n_words; w0 += VW) {
#pragma unroll
    for (int k = 0; k < VL; ++k) {
      sA[(lr + k * (VB / VW)) * VS + lw] = ra[k];
      sB[(lr + k * (VB / VW)) * VS + lw] = rb[k];
    }
    __syncthreads();
    if (w0 + VW < a.n_words) fetch(w0 + VW);                  // (uniform in the workgroup)
    const int k0 = wave * (VW / VK);                          // this wave's share of the chunk's words
#pragma unroll
    for (int k = k0; k < k0 + VW / VK; k += 2) {
      uint32_t a0[VA], a1[VA], b0[VA], b1[VA];
#pragma unroll
      for (int i = 0; i < VA; ++i) { a0[i] = sA[(ty + 8 * i) * VS + k]; a1[i] = sA[(ty + 8 * i) * VS + k + 1]; }
#pragma unroll
      for (int j = 0; j < VA; ++j) { b0[j] = sB[(tx + 8 * j) * VS + k]; b1[j] = sB[(tx + 8 * j) * VS + k + 1]; }
#pragma unroll
      for (int i = 0; i < VA; ++i)
#pragma unroll
        for (int j = 0; j < VA; ++j) acc[i][j] += __popc(a0[i] & b0[j]) + __popc(a1[i] & b1[j]);      // one 64-bit count
    }
    __syncthreads();
  }
  // the four waves' shares of every pair, added inside the workgroup (whole numbers: any order gives the same sum)
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < VA; ++i)
#pragma unroll
      for (int j = 0; j < VA; ++j) s_all[((wave - 1) * VA * VA + i * VA + j) * 64 + lane] = (uint32_t)acc[i][j];
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int i = 0; i < VA; ++i)
#pragma unroll
    for (int j = 0; j < VA; ++j) {
      int sum = acc[i][j];
#pragma unroll
      for (int v = 0; v < VK - 1; ++v) sum += (int)s_all[(v * VA * VA + i * VA + j) * 64 + lane];
      const int f = f0 + ty + 8 * i, g = g0 + tx + 8 * j;
      if (f >= a.n_frames || g >= a.n_frames) continue;
      a.counts[(size_t)f * a.n_frames + g] = sum;
      if (ti != tj) a.counts[(size_t)g * a.n_frames + f] = sum;      // the mirrored tile (a diagonal tile holds both triangles)
    }
}

__global__ __launch_bounds__(VB) void covis_rowpop_kernel(MapCovisArgs a) {
  __shared__ int s_w[16];
  const uint32_t* row = a.bits + covis_row(blockIdx.x, a.n_words);
  int n = 0;
  for (int w = threadIdx.x; w < a.n_words; w += VB) n += __popc(row[w]);
  n = block_sum(n, s_w);
  if (threadIdx.x == 0) a.w.row_pop[blockIdx.x] = n;
}

__global__ __launch_bounds__(VB) void covis_union_kernel(MapCovisArgs a) {
  __shared__ int s_w[16];
  const int w = blockIdx.x * VB + threadIdx.x;
  uint32_t u = 0u;
  if (w < a.n_words)
    for (int f = 0; f < a.n_frames; ++f) u |= a.bits[covis_row(f, a.n_words) + w];
  const int n = block_sum(__popc(u), s_w);
  if (threadIdx.x == 0) a.w.part[blockIdx.x] = n;
}

// voe_map_covis_stats: int32 n_frames, n_entries, n_hits, n_seen, n_entries_seen, three reserved words
__global__ __launch_bounds__(VB) void covis_stats_kernel(MapCovisArgs a, int n_parts) {
  __shared__ int s_w[16];
  int hits = 0, seen = 0, any = 0;
  for (int f = threadIdx.x; f < a.n_frames; f += VB) { hits += a.n_max > 0 ? a.w.n_hits[f] : 0; seen += a.w.row_pop[f]; }
  for (int b = threadIdx.x; b < n_parts; b += VB) any += a.w.part[b];
  hits = block_sum(hits, s_w);
  seen = block_sum(seen, s_w);
  any = block_sum(any, s_w);
  if (threadIdx.x == 0) {
    int M = a.hdr[0];
    M = M < a.cap ? M : a.cap;
    int* si = static_cast<int*>(a.stats);
    si[0] = a.n_frames; si[1] = M; si[2] = hits; si[3] = seen; si[4] = any; si[5] = 0; si[6] = 0; si[7] = 0;
  }
}

// ---- the window ------------------------------------------------------------------------------------------------------------
// cnt[g] = the common bits of row g and of row query (against_union == 0) or of U (against_union != 0)
__global__ __launch_bounds__(VB) void window_count_kernel(MapWindowArgs a, int against_union) {
  __shared__ int s_w[16];
  const uint32_t* row = a.bits + covis_row(blockIdx.x, a.n_words);
  const uint32_t* other = against_union ? a.uni : a.bits + covis_row(a.query, a.n_words);
  int n = 0;
  for (int w = threadIdx.x; w < a.n_words; w += VB) n += __popc(row[w] & other[w]);
  n = block_sum(n, s_w);
  if (threadIdx.x == 0) a.w.cnt[blockIdx.x] = n;
}

// the rank of every candidate among the candidates, by counting the smaller keys: exact, and the same in any schedule
__device__ __forceinline__ int window_rank(const uint64_t* s_key, int n_frames, uint64_t key) {
  int r = 0;
  for (int h = 0; h < n_frames; ++h) r += s_key[h] < key;
  return r;
}

__global__ __launch_bounds__(VR) void window_free_kernel(MapWindowArgs a) {
  __shared__ uint64_t s_key[MAX_F];
  __shared__ int s_w[16];
  const int seen = a.w.cnt[a.query];
  int n_cand = 0;
  for (int g = threadIdx.x; g < a.n_frames; g += VR) {
    const int c = a.w.cnt[g];
    const bool cand = g != a.query && seen > 0 && c >= a.min_shared;
    s_key[g] = cand ? covis_rank_key(c, g) : ~0ull;         // (no candidate's key reaches it)
    n_cand += cand;
  }
  n_cand = block_sum(n_cand, s_w);                      // (its barriers also publish the keys)
  for (int g = threadIdx.x; g < a.n_frames; g += VR) {
    int role = WR_OUTSIDE;
    if (g == a.query) {
      if (seen > 0) { role = WR_FREE; a.order[0] = g; }
    } else if (s_key[g] != ~0ull) {
      const int r = window_rank(s_key, a.n_frames, s_key[g]);
      if (r < a.k_free - 1) { role = WR_FREE; a.order[1 + r] = g; }
    }
    a.role[g] = role;
  }
  if (threadIdx.x == 0) {
    const int more = n_cand < a.k_free - 1 ? n_cand : a.k_free - 1;
    a.w.ctl[0] = seen > 0 ? 1 + more : 0;
    a.w.ctl[1] = n_cand;
    a.w.ctl[2] = seen;
  }
}

__global__ __launch_bounds__(VB) void window_union_kernel(MapWindowArgs a) {
  __shared__ int s_w[16];
  const int w = blockIdx.x * VB + threadIdx.x;
  const int n_free = a.w.ctl[0];
  uint32_t u = 0u;
  if (w < a.n_words) {
    for (int j = 0; j < n_free; ++j) u |= a.bits[covis_row(a.order[j], a.n_words) + w];
    a.uni[w] = u;
  }
  const int n = block_sum(__popc(u), s_w);
  if (threadIdx.x == 0) a.w.part[blockIdx.x] = n;
}

// voe_map_window_stats: int32 status, n_free, n_fixed, n_candidates, n_fixed_candidates, n_points, query_seen, reserved
__global__ __launch_bounds__(VR) void window_fixed_kernel(MapWindowArgs a, int n_parts) {
  __shared__ uint64_t s_key[MAX_F];
  __shared__ int s_w[16];
  const int n_free = a.w.ctl[0];
  int n_cand = 0, points = 0;
  for (int h = threadIdx.x; h < a.n_frames; h += VR) {
    const int s = a.w.cnt[h];
    const bool cand = a.role[h] != WR_FREE && s >= a.min_shared;
    s_key[h] = cand ? covis_rank_key(s, h) : ~0ull;
    n_cand += cand;
  }
  for (int b = threadIdx.x; b < n_parts; b += VR) points += a.w.part[b];
  n_cand = block_sum(n_cand, s_w);
  points = block_sum(points, s_w);
  const int n_fixed = n_cand < a.k_fixed ? n_cand : a.k_fixed;
  for (int h = threadIdx.x; h < a.n_frames; h += VR) {
    int role = a.role[h];
    if (s_key[h] != ~0ull) {
      const int r = window_rank(s_key, a.n_frames, s_key[h]);
      if (r < a.k_fixed) { role = WR_FIXED; a.order[n_free + r] = h; }
    }
    a.role[h] = role;
    a.n_rows_out[h] = role != WR_OUTSIDE ? (a.d_n ? a.d_n[h] : a.n_max) : 0;
    a.fixed_out[h] = role == WR_FREE ? 0 : 1;
  }
  for (int j = n_free + n_fixed + threadIdx.x; j < a.n_frames; j += VR) a.order[j] = -1;
  if (threadIdx.x == 0) {
    int* si = static_cast<int*>(a.stats);
    si[0] = a.w.ctl[2] == 0 ? WS_QUERY_UNSEEN : n_fixed == 0 ? WS_NO_FIXED : WS_OK;
    si[1] = n_free; si[2] = n_fixed; si[3] = a.w.ctl[1]; si[4] = n_cand; si[5] = points; si[6] = a.w.ctl[2]; si[7] = 0;
  }
}

static int covis_parts(int n_words) { return (n_words + VB - 1) / VB; }

MapCovisWs map_covis_layout(void* base, int n_frames, int n_max, int n_words) {
  MapCovisWs w{};
  WsCarver c(base);
  const size_t F = (size_t)n_frames, N = (size_t)(n_max > 0 ? n_max : 1);
  w.pairs = c.take<int32_t>(8 * F * N);
  w.ent = c.take<int32_t>(4 * F * N);
  w.n_hits = c.take<int>(4 * F);
  w.row_pop = c.take<int>(4 * F);
  w.part = c.take<int>(4 * (size_t)covis_parts(n_words));
  w.bytes = c.bytes;
  return w;
}

hipError_t launch_map_covis_bits(hipStream_t st, const MapCovisArgs& a) {
  const hipError_t e = hipMemsetAsync(a.bits, 0, sizeof(uint32_t) * (size_t)a.n_frames * (size_t)a.n_words, st);
  if (e != hipSuccess) return e;
  if (a.n_max > 0) hipLaunchKernelGGL(covis_bits_kernel, dim3((a.n_max + VB - 1) / VB, a.n_frames), dim3(VB), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_covis(hipStream_t st, const MapCovisArgs& a) {
  const hipError_t e = launch_map_covis_bits(st, a);
  if (e != hipSuccess) return e;
  if (a.counts) hipLaunchKernelGGL(covis_count_kernel, dim3(covis_tiles(a.n_frames)), dim3(VB), 0, st, a, covis_tiles_edge(a.n_frames));
  hipLaunchKernelGGL(covis_rowpop_kernel, dim3(a.n_frames), dim3(VB), 0, st, a);
  hipLaunchKernelGGL(covis_union_kernel, dim3(covis_parts(a.n_words)), dim3(VB), 0, st, a);
  hipLaunchKernelGGL(covis_stats_kernel, dim3(1), dim3(VB), 0, st, a, covis_parts(a.n_words));
  return hipGetLastError();
}

MapWindowWs map_window_layout(void* base, int n_frames, int n_words) {
  MapWindowWs w{};
  WsCarver c(base);
  w.cnt = c.take<int>(4 * (size_t)n_frames);
  w.order = c.take<int32_t>(4 * (size_t)n_frames);
  w.uni = c.take<uint32_t>(4 * (size_t)n_words);
  w.part = c.take<int>(4 * (size_t)covis_parts(n_words));
  w.ctl = c.take<int>(16);
  w.bytes = c.bytes;
  return w;
}

hipError_t launch_map_window(hipStream_t st, const MapWindowArgs& a) {
  hipLaunchKernelGGL(window_count_kernel, dim3(a.n_frames), dim3(VB), 0, st, a, 0);
  hipLaunchKernelGGL(window_free_kernel, dim3(1), dim3(VR), 0, st, a);
  hipLaunchKernelGGL(window_union_kernel, dim3(covis_parts(a.n_words)), dim3(VB), 0, st, a);
  hipLaunchKernelGGL(window_count_kernel, dim3(a.n_frames), dim3(VB), 0, st, a, 1);
  hipLaunchKernelGGL(window_fixed_kernel, dim3(1), dim3(VR), 0, st, a, covis_parts(a.n_words));
  return hipGetLastError();
}

}  // namespace vo
