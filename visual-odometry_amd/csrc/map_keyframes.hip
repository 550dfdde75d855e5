// map_keyframes.hip -- keyframes chosen from the covisibility bit rows (voe_map_keyframes*): the frames whose landmarks enough
// other frames see are dropped one at a time, the most redundant first.  The rules are those of include/vo_hip.h (KEYFRAMES); the
// bit-sliced counters, the candidate tests and the order of two candidates are the inline functions of keyframes_rules.h.
// Everything here is an integer: every sum is exact in any order, and the file forms no real number.
// How many live frames see an entry is kept BIT-SLICED: plane p of word w holds bit p of that count for the 32 entries of the
// word, so a row is added or taken out, and "count >= min_observers + 1" is answered, 32 entries per and / xor / or.
// Launches, a fixed sequence for (n_frames, n_words, max_dropped):
//   keyframes_frames_kernel   one workgroup per frame: the flag, seen[f] by an integer tree, the frame's state, its outputs' defaults
//   keyframes_planes_kernel   one thread per word: the planes, the rows of the frames that are not GONE added one after the other
//   max_dropped times, each pair returning at once behind the device's done flag:
//     keyframes_count_kernel  workgroups stride over chunks of KEYFRAMES_CHUNK words, one word per lane.  The row the step before
//                             dropped leaves the chunk's planes (this is the only writer of a chunk's planes in the launch); the
//                             chunk's masks go to LDS; then every wave takes frames of its own: popcount(row & mask) of the
//                             frames that can still be candidates, summed over the wave by shuffles and kept per frame in LDS.  A
//                             frame of the LDS array has one owning wave, so nothing is atomic there; at the end of the launch a
//                             workgroup issues one integer atomicAdd per frame it has a count for.
//     keyframes_select_kernel one workgroup: the candidate tests (a frame that fails one is never read again: the monotonicity of
//                             the header), the best candidate by a tree over (red, seen, frame) compared by int64 cross-products,
//                             the step's record, the live byte, the accumulator zeroed; done when there is no candidate
//   keyframes_count_kernel    once more over EVERY live frame: red at the final state, for the outputs and the verdicts
//   keyframes_finish_kernel   one workgroup: verdicts, row counts, keep bytes, seen / red of the frames not dropped, the statistics
// No launch waits for another workgroup.  The one atomic is the integer atomicAdd named above.
#include "vo_internal.h"
#include "covis_rules.h"
#include "keyframes_rules.h"

namespace vo {

constexpr int KB = KEYFRAMES_CHUNK;           // threads of a counting workgroup: one per word of a chunk
constexpr int KR = 1024;                      // threads of the selecting and the finishing workgroup
constexpr int KW = KB / 64;                   // waves of a counting workgroup
constexpr int KJ = KEYFRAMES_CHUNK / 64;      // words of a chunk per lane
constexpr int KU = 4;                         // frames a wave has in flight
constexpr int KMAX_F = 4096;                  // VOE_MAP_COVIS_MAX_FRAMES
constexpr int KMAX_GRID = 2048;               // counting workgroups at most; they stride over the chunks
static_assert(KB == 256 && KB % 64 == 0, "a chunk is a workgroup's width and whole waves");

// the header's numbers: the flags FREE 0, PROTECTED 1, GONE 2; a PROTECTED or GONE frame's verdict is its flag
enum { KF_FREE = 0, KF_PROTECTED = 1, KF_GONE = 2 };
enum { KV_LEFT = 0, KV_PROTECTED = 1, KV_GONE = 2, KV_DROPPED = 3, KV_EMPTY = 4, KV_NEEDED = 5, KV_GAP = 6 };

__device__ __forceinline__ int keyframes_flag(const MapKeyframesArgs& a, int f) {
  const int v = a.flags ? a.flags[f] : KF_FREE;
  return v > KF_GONE ? KF_PROTECTED : v;            // (the device form cannot refuse: such a frame is never dropped)
}

__global__ __launch_bounds__(KB) void keyframes_frames_kernel(MapKeyframesArgs a) {
  __shared__ int s_w[16];
  const int f = blockIdx.x;
  const int flag = keyframes_flag(a, f);
  int n = 0;
  if (flag != KF_GONE) {
    const uint32_t* row = a.bits + covis_row(f, a.n_words);
    for (int w = threadIdx.x; w < a.n_words; w += KB) n += __popc(row[w]);
  }
  n = block_sum(n, s_w);
  if (threadIdx.x == 0) {
    a.w.seen[f] = n;
    a.w.red[f] = 0;
    a.w.live[f] = flag != KF_GONE;
    a.w.poss[f] = flag == KF_FREE && n >= a.min_seen;
    a.step[f] = -1;
    a.order[f] = -1;
    if (f == 0) { a.w.ctl[0] = 0; a.w.ctl[1] = 0; a.w.ctl[2] = -1; }
  }
}

__global__ __launch_bounds__(KB) void keyframes_planes_kernel(MapKeyframesArgs a) {
  const int w = blockIdx.x * KB + threadIdx.x;
  if (w >= a.n_words) return;
  uint32_t pl[KEYFRAMES_MAX_PLANES];
#pragma unroll
  for (int p = 0; p < KEYFRAMES_MAX_PLANES; ++p) pl[p] = 0u;
#pragma unroll 8
  for (int f = 0; f < a.n_frames; ++f) {
    const uint32_t x = a.bits[covis_row(f, a.n_words) + w] & (a.w.live[f] ? ~0u : 0u);      // (a GONE frame's row is ignored)
    keyframes_add(pl, a.n_planes, x);
  }
#pragma unroll
  for (int p = 0; p < KEYFRAMES_MAX_PLANES; ++p)
    if (p < a.n_planes) a.w.planes[(size_t)p * a.n_words + w] = pl[p];
}

// all == 0: a step -- returns behind done, counts the frames that can still be candidates.  all != 0: the final state -- counts
// every live frame.  Both first take the row of ctl[2] out of the planes.
__global__ __launch_bounds__(KB) void keyframes_count_kernel(MapKeyframesArgs a, int all) {
  __shared__ int s_red[KMAX_F];
  __shared__ uint32_t s_mask[KEYFRAMES_CHUNK];
  if (!all && a.w.ctl[0]) return;
  const int last = a.w.ctl[2];
  const uint8_t* use = all ? a.w.live : a.w.poss;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t thr = keyframes_threshold(a.min_observers);
  const int n_chunks = (a.n_words + KEYFRAMES_CHUNK - 1) / KEYFRAMES_CHUNK;
  for (int f = threadIdx.x; f < a.n_frames; f += KB) s_red[f] = 0;      // (published by the barriers of the first chunk)
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int base = c * KEYFRAMES_CHUNK;
    const int w = base + threadIdx.x;
    uint32_t mask = 0u;
    if (w < a.n_words) {
      uint32_t pl[KEYFRAMES_MAX_PLANES];
#pragma unroll
      for (int p = 0; p < KEYFRAMES_MAX_PLANES; ++p) pl[p] = p < a.n_planes ? a.w.planes[(size_t)p * a.n_words + w] : 0u;
      const uint32_t x = last >= 0 ? a.bits[covis_row(last, a.n_words) + w] : 0u;
      if (x) {
        keyframes_sub(pl, a.n_planes, x);
#pragma unroll
        for (int p = 0; p < KEYFRAMES_MAX_PLANES; ++p)
          if (p < a.n_planes) a.w.planes[(size_t)p * a.n_words + w] = pl[p];
      }
      mask = keyframes_ge(pl, a.n_planes, thr);
    }
    __syncthreads();                                        // (the chunk before has read its masks)
    s_mask[threadIdx.x] = mask;
    __syncthreads();
    uint32_t m[KJ];
#pragma unroll
    for (int j = 0; j < KJ; ++j) m[j] = s_mask[lane + 64 * j];      // (0 behind the last word)
    // wave k owns the frames f with (f / KU) % KW == k
    for (int f0 = wave * KU; f0 < a.n_frames; f0 += KW * KU) {
      int n[KU];
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const int f = f0 + u;
        n[u] = 0;
        if (f < a.n_frames && use[f]) {
          const uint32_t* row = a.bits + covis_row(f, a.n_words) + base;
#pragma unroll
          for (int j = 0; j < KJ; ++j)
            if (base + lane + 64 * j < a.n_words) n[u] += __popc(row[lane + 64 * j] & m[j]);
        }
      }
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        int v = n[u];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        if (lane == 0 && f0 + u < a.n_frames) s_red[f0 + u] += v;
      }
    }
  }
  __syncthreads();
  for (int f = threadIdx.x; f < a.n_frames; f += KB) {
    const int v = s_red[f];
    if (v) atomicAdd(a.w.red + f, v);
  }
}

__global__ __launch_bounds__(KR) void keyframes_select_kernel(MapKeyframesArgs a) {
  __shared__ int s_r[KR], s_s[KR], s_f[KR];
  if (a.w.ctl[0]) return;
  int br = 0, bs = 1, bf = -1;
  for (int f = threadIdx.x; f < a.n_frames; f += KR) {
    const int r = a.w.red[f];
    a.w.red[f] = 0;                                         // the accumulator of the next step
    if (!a.w.poss[f]) continue;
    const int s = a.w.seen[f];
    const bool ok = keyframes_share_ok(r, s, a.share_permille) && (a.max_gap <= 0 || keyframes_gap_ok(a.w.live, a.n_frames, f, a.max_gap));
    if (!ok) { a.w.poss[f] = 0; continue; }                 // never a candidate again: red only falls, runs only grow
    if (keyframes_before(r, s, f, br, bs, bf)) { br = r; bs = s; bf = f; }
  }
  s_r[threadIdx.x] = br; s_s[threadIdx.x] = bs; s_f[threadIdx.x] = bf;
  __syncthreads();                                          // (also: every walk over the live bytes is behind us)
  for (int d = KR / 2; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) {
      const int o = threadIdx.x + d;
      if (keyframes_before(s_r[o], s_s[o], s_f[o], s_r[threadIdx.x], s_s[threadIdx.x], s_f[threadIdx.x])) {
        s_r[threadIdx.x] = s_r[o]; s_s[threadIdx.x] = s_s[o]; s_f[threadIdx.x] = s_f[o];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int f = s_f[0], k = a.w.ctl[1];
    if (f >= 0 && k < a.max_dropped) {
      a.step[f] = k; a.order[k] = f;
      a.seen_out[f] = s_s[0]; a.red_out[f] = s_r[0];
      a.w.live[f] = 0; a.w.poss[f] = 0;
      a.w.ctl[1] = k + 1; a.w.ctl[2] = f;
    } else {
      a.w.ctl[0] = 1; a.w.ctl[2] = -1;
    }
  }
}

// voe_map_keyframes_stats: int32 n_frames, n_kept, n_dropped, n_gone, n_protected, n_needed, n_blocked, n_empty
__global__ __launch_bounds__(KR) void keyframes_finish_kernel(MapKeyframesArgs a) {
  __shared__ int s_w[16];
  int n_dropped = 0, n_gone = 0, n_prot = 0, n_needed = 0, n_blocked = 0, n_empty = 0;
  for (int f = threadIdx.x; f < a.n_frames; f += KR) {
    const int flag = keyframes_flag(a, f);
    const int seen = a.w.seen[f], red = a.w.red[f];
    int v;
    if (flag == KF_GONE) { v = KV_GONE; ++n_gone; }
    else if (a.step[f] >= 0) { v = KV_DROPPED; ++n_dropped; }
    else if (flag == KF_PROTECTED) { v = KV_PROTECTED; ++n_prot; }
    else if (seen < a.min_seen) { v = KV_EMPTY; ++n_empty; }
    else if (!keyframes_share_ok(red, seen, a.share_permille)) { v = KV_NEEDED; ++n_needed; }
    else if (a.max_gap > 0 && !keyframes_gap_ok(a.w.live, a.n_frames, f, a.max_gap)) { v = KV_GAP; ++n_blocked; }
    else { v = KV_LEFT; ++n_blocked; }
    const bool out = v == KV_GONE || v == KV_DROPPED;
    a.verdict[f] = v;
    a.n_rows_out[f] = out ? 0 : (a.d_n ? a.d_n[f] : a.n_max);
    a.keep[f] = out ? 0 : 1;
    if (v != KV_DROPPED) { a.seen_out[f] = seen; a.red_out[f] = v == KV_GONE ? 0 : red; }      // (a dropped frame's: at its own step)
  }
  n_dropped = block_sum(n_dropped, s_w);
  n_gone = block_sum(n_gone, s_w);
  n_prot = block_sum(n_prot, s_w);
  n_needed = block_sum(n_needed, s_w);
  n_blocked = block_sum(n_blocked, s_w);
  n_empty = block_sum(n_empty, s_w);
  if (threadIdx.x == 0) {
    int* si = static_cast<int*>(a.stats);
    si[0] = a.n_frames; si[1] = a.n_frames - n_dropped - n_gone; si[2] = n_dropped; si[3] = n_gone;
    si[4] = n_prot; si[5] = n_needed; si[6] = n_blocked; si[7] = n_empty;
  }
}

MapKeyframesWs map_keyframes_layout(void* base, int n_frames, int n_words) {
  MapKeyframesWs w{};
  WsCarver c(base);
  const size_t F = (size_t)n_frames;
  w.planes = c.take<uint32_t>(4 * (size_t)keyframes_planes(n_frames) * (size_t)n_words);
  w.seen = c.take<int>(4 * F);
  w.red = c.take<int>(4 * F);
  w.live = c.take<uint8_t>(F);
  w.poss = c.take<uint8_t>(F);
  w.order = c.take<int32_t>(4 * F);
  w.ctl = c.take<int>(16);
  w.bytes = c.bytes;
  return w;
}

hipError_t launch_map_keyframes(hipStream_t st, const MapKeyframesArgs& a) {
  const int n_chunks = (a.n_words + KEYFRAMES_CHUNK - 1) / KEYFRAMES_CHUNK;
  const int grid = n_chunks < KMAX_GRID ? n_chunks : KMAX_GRID;
  hipLaunchKernelGGL(keyframes_frames_kernel, dim3(a.n_frames), dim3(KB), 0, st, a);
  hipLaunchKernelGGL(keyframes_planes_kernel, dim3((a.n_words + KB - 1) / KB), dim3(KB), 0, st, a);
  for (int k = 0; k < a.max_dropped; ++k) {
    hipLaunchKernelGGL(keyframes_count_kernel, dim3(grid), dim3(KB), 0, st, a, 0);
    hipLaunchKernelGGL(keyframes_select_kernel, dim3(1), dim3(KR), 0, st, a);
  }
  hipLaunchKernelGGL(keyframes_count_kernel, dim3(grid), dim3(KB), 0, st, a, 1);
  hipLaunchKernelGGL(keyframes_finish_kernel, dim3(1), dim3(KR), 0, st, a);
  return hipGetLastError();
}

}  // namespace vo
