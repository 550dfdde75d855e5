// map_loops.hip -- loop edges found and measured in the map (voe_map_loops*).  The rules are those of include/vo_map_loops.h.
// Everything up to the measurement is an integer: every sum is exact in any order.  The hits are the public lookup's, the
// reference frames come from the launches of voe_map_apply_correction (pose_graph.hip, a dry run), the bit rows from the
// covisibility's bit pass (map_covis.hip), the measurement from the two public batched calls; what lives here:
//   loops_hist_kernel     one workgroup per frame j: walks the words of row j, 64 words per wave and step.  A step deals its 64
//                         words two at a time over the wave -- lane l looks at bit l & 31 of word l >> 5 of the pair -- so the
//                         gather of ref[e] reads 2 x 128 contiguous bytes per instruction and only under a set bit.  The lanes
//                         whose entries share a reference frame (neighbours in the map usually do: it grew frame by frame) add
//                         their count with ONE integer LDS atomic.  Then the row is stored, summed to a prefix in LDS, and the
//                         frame's candidate is the maximum of a 64-bit key over i < j - gap.
//   loops_choose_kernel   one workgroup: the suppression within `separation`, the survivors ranked by counting the smaller keys
//                         (covis_rank_key: c descending, j ascending), the slots, three counts.
//   loops_pairs_kernel    one workgroup per slot: the band's rows of frame j in ascending row by count / scan / scatter, 1024
//                         rows a step with a running base; the points gathered, the frame's pixels copied.
//   loops_finish_kernel   one workgroup: status, edge, Z in double, record, statistics.
// No launch waits for another workgroup; no float atomics.
#include "vo_internal.h"
#include "covis_rules.h"
#include "sim3.h"
#include "../../include/vo_map_loops.h"

namespace vo {

constexpr int LB = 256;                   // threads of a histogram workgroup: 4 waves of 64 words each
constexpr int LR = 1024;                  // threads of the choosing and the gathering workgroups
constexpr int LF = MAP_LOOPS_MAX_FRAMES;
static_assert(LF == VOE_MAP_COVIS_MAX_FRAMES && LF % LB == 0, "a row of the histogram is LF ints of LDS, dealt in equal runs");
static_assert(sizeof(voe_map_loop_record) == 40 && sizeof(voe_map_loops_stats) == 32, "the finish writes these records word by word");

__global__ __launch_bounds__(LB) void loops_hist_kernel(MapLoopsArgs a) {
  __shared__ int s_hist[LF];
  __shared__ int s_w[LB / 64];
  __shared__ unsigned long long s_best[LB / 64];
  const int j = blockIdx.x, F = a.n_frames, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, half = lane >> 5, bit = lane & 31;
  for (int k = tid; k < LF; k += LB) s_hist[k] = 0;
  __syncthreads();
  const uint32_t* row = a.w.bits + covis_row(j, a.n_words);
  for (int w0 = wave * 64; w0 < a.n_words; w0 += LB) {        // (uniform in the wave)
    const int w = w0 + lane;
    const uint32_t mine = w < a.n_words ? row[w] : 0u;
    if (__ballot(mine != 0u) == 0ull) continue;
    for (int k = 0; k < 32; ++k) {
      const uint32_t word = __shfl(mine, 2 * k + half);
      bool on = (word >> bit) & 1u;
      int r = -1;
      if (on) {
        r = a.ref[32 * (size_t)(w0 + 2 * k + half) + bit];    // (a set bit lies below the size: inside every ref array)
        on = (unsigned)r < (unsigned)F;
      }
      unsigned long long todo = __ballot(on);
      while (todo) {                                          // one LDS atomic per distinct reference frame of the step
        const int leader = __ffsll((long long)todo) - 1;
        const int r0 = __shfl(r, leader);
        const unsigned long long same = __ballot(on && r == r0);
        if (lane == leader) atomicAdd(&s_hist[r0], __popcll(same));
        todo &= ~same;
      }
    }
  }
  __syncthreads();
  if (a.hist)
    for (int k = tid; k < F; k += LB) a.hist[(size_t)j * F + k] = s_hist[k];
  __syncthreads();
  // the inclusive prefix of the row, in place: every thread owns a run of LF / LB consecutive frames
  constexpr int PER = LF / LB;
  int run = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) run += s_hist[tid * PER + k];
  int total;
  int before = block_exclusive_scan<LB>(run, s_w, total);
#pragma unroll
  for (int k = 0; k < PER; ++k) { before += s_hist[tid * PER + k]; s_hist[tid * PER + k] = before; }
  __syncthreads();
  // the candidate: the largest (c, -i) over 0 <= i < j - gap with c >= min_shared
  unsigned long long best = 0ull;
  const long long end = (long long)j - a.gap;
  for (int i = tid; i < end && i < F; i += LB) {
    const int lo = i > a.ref_window ? i - a.ref_window : 0;
    const int c = s_hist[i] - (lo > 0 ? s_hist[lo - 1] : 0);
    if (c >= a.min_shared) {
      const unsigned long long key = ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(unsigned)(0x7fffffff - i);
      best = key > best ? key : best;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(best, d); best = o > best ? o : best; }
  if (lane == 0) s_best[wave] = best;
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < LB / 64; ++v) best = s_best[v] > best ? s_best[v] : best;
    a.w.cand[2 * j] = best ? 0x7fffffff - (int)(unsigned)(best & 0xffffffffull) : -1;
    a.w.cand[2 * j + 1] = (int)(best >> 32);
  }
}

__global__ __launch_bounds__(LR) void loops_choose_kernel(MapLoopsArgs a) {
  __shared__ int s_c[LF];
  __shared__ uint64_t s_key[LF];
  __shared__ int s_w[LR / 64];
  const int F = a.n_frames, tid = threadIdx.x;
  for (int j = tid; j < F; j += LR) s_c[j] = a.w.cand[2 * j] >= 0 ? a.w.cand[2 * j + 1] : 0;      // (a candidate has c >= min_shared >= 1)
  for (int l = tid; l < a.max_loops; l += LR) { int32_t* s = a.w.slots + 4 * l; s[0] = -1; s[1] = -1; s[2] = 0; s[3] = 0; }
  __syncthreads();
  int n_cand = 0, n_surv = 0;
  for (int j = tid; j < F; j += LR) {
    const int c = s_c[j];
    bool keep = c > 0;
    n_cand += keep;
    const int lo = j - (a.separation < j ? a.separation : j), hi = j + (a.separation < F - 1 - j ? a.separation : F - 1 - j);
    for (int o = lo; keep && o <= hi; ++o) {
      const int co = s_c[o];
      if (o != j && (co > c || (co == c && o < j))) keep = false;
    }
    s_key[j] = keep ? covis_rank_key(c, j) : ~0ull;
    n_surv += keep;
  }
  int tot_cand, tot_surv;
  (void)block_exclusive_scan<LR>(n_cand, s_w, tot_cand);
  __syncthreads();
  (void)block_exclusive_scan<LR>(n_surv, s_w, tot_surv);      // (its barrier also publishes the keys)
  for (int j = tid; j < F; j += LR) {
    const uint64_t key = s_key[j];
    if (key == ~0ull) continue;
    int rank = 0;
    for (int o = 0; o < F; ++o) rank += s_key[o] < key;
    if (rank < a.max_loops) { int32_t* s = a.w.slots + 4 * rank; s[0] = a.w.cand[2 * j]; s[1] = j; s[2] = s_c[j]; }
  }
  if (tid == 0) { a.w.ctl[0] = tot_cand; a.w.ctl[1] = tot_surv; a.w.ctl[2] = tot_surv < a.max_loops ? tot_surv : a.max_loops; }
}

__global__ __launch_bounds__(LR) void loops_pairs_kernel(MapLoopsArgs a) {
  __shared__ int s_w[LR / 64];
  const int l = blockIdx.x, tid = threadIdx.x;
  const int i = a.w.slots[4 * l], j = a.w.slots[4 * l + 1];
  if (i < 0) {                                                // EMPTY (uniform)
    if (tid == 0) a.w.n_pairs[l] = 0;
    return;
  }
  int M = a.hdr[0];
  M = M < a.cap ? M : a.cap;
  M = M < a.bound ? M : a.bound;
  const int n = live_rows(a.d_n ? a.d_n + j : nullptr, a.n_max);
  const int lo = i > a.ref_window ? i - a.ref_window : 0;
  const size_t slot = (size_t)l * a.n_max;
  const float2* uv_in = reinterpret_cast<const float2*>(a.uv) + (size_t)j * a.uv_stride;
  float2* uv_out = reinterpret_cast<float2*>(a.w.uv) + slot;
  int base = 0;
  for (int row0 = 0; row0 < a.n_max; row0 += LR) {
    const int row = row0 + tid;
    if (row < a.n_max) uv_out[row] = uv_in[row];
    bool take = false;
    int e = -1;
    if (row < n) {
      e = a.w.ent[(size_t)j * a.n_max + row];
      if (e >= 0 && e < M) { const int r = a.ref[e]; take = r >= lo && r <= i; }
    }
    int total;
    const int k = base + block_rank<LR>(take, s_w, total);
    if (take) {                                               // k < n_max: one pair per live row at most
      const float* p = a.pts + 3 * (size_t)e;
      float* q = a.w.world + 3 * (slot + k);
      q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
      reinterpret_cast<int2*>(a.w.lpairs)[slot + k] = make_int2(row, k);
    }
    base += total;
    __syncthreads();                                          // (s_w is written again by the next step)
  }
  if (tid == 0) a.w.n_pairs[l] = base;
}

// voe_map_loop_record: int32 i, j, c, n_pairs, ransac_status, ransac_inliers, num_inliers, status; float chi_inliers, chi_outliers
// voe_map_loops_stats: int32 n_frames, n_entries, n_candidates, n_survivors, n_slots, n_ok, two reserved words
__global__ __launch_bounds__(LB) void loops_finish_kernel(MapLoopsArgs a) {
  __shared__ int s_w[LB / 64];
  int n_ok = 0;
  for (int l = threadIdx.x; l < a.max_loops; l += LB) {
    const int i = a.w.slots[4 * l], j = a.w.slots[4 * l + 1], c = a.w.slots[4 * l + 2];
    const int n_pairs = a.w.n_pairs[l], rstat = a.w.rstat[l], handed = a.w.n_handed[l];
    const float* T = a.w.T_solved + 16 * (size_t)l;
    const float chi_in = a.w.stats4[4 * (size_t)l], chi_out = a.w.stats4[4 * (size_t)l + 1];
    const int n_in = (int)a.w.stats4[4 * (size_t)l + 2];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 16; ++k) finite &= fabsf(T[k]) <= 3.402823466e38f;      // false for NaN and +-inf
    float Z[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) Z[k] = (k % 5 == 0) ? 1.f : 0.f;
    int status = VOE_MAP_LOOP_OK;
    if (i < 0) status = VOE_MAP_LOOP_EMPTY;
    else if (n_pairs < 6) status = VOE_MAP_LOOP_FEW_MATCHES;
    else if (rstat != 0) status = VOE_MAP_LOOP_NO_CONSENSUS;
    else if (!finite) status = VOE_MAP_LOOP_NOT_FINITE;
    else if (n_in < a.min_inliers) status = VOE_MAP_LOOP_FEW_INLIERS;
    else {
      // Z = S'_j S_i^-1, S'_j = [c_i R | c_i t], S_i^-1 = [M_i^-1 | -M_i^-1 t_i]: in double, rounded once
      const float* S = a.S16 + 16 * (size_t)i;
      double Mi[9], ti[3], Minv[9], A[9], at[3], Zm[9], u[3], v[3];
#pragma unroll
      for (int k = 0; k < 9; ++k) Mi[k] = (double)S[(k % 3) + 4 * (k / 3)];
#pragma unroll
      for (int k = 0; k < 3; ++k) ti[k] = (double)S[12 + k];
      const double ci = cbrt(pg_det3(Mi));
      pg_inv3(Mi, Minv);
#pragma unroll
      for (int k = 0; k < 9; ++k) A[k] = ci * (double)T[(k % 3) + 4 * (k / 3)];
#pragma unroll
      for (int k = 0; k < 3; ++k) at[k] = ci * (double)T[12 + k];
#pragma unroll
      for (int col = 0; col < 3; ++col) pg_mv(A, Minv + 3 * col, Zm + 3 * col);
      pg_mv(Minv, ti, u);
      pg_mv(A, u, v);
      bool zf = true;
#pragma unroll
      for (int k = 0; k < 9; ++k) { Z[(k % 3) + 4 * (k / 3)] = (float)Zm[k]; zf &= refine_finite(Zm[k]); }
#pragma unroll
      for (int k = 0; k < 3; ++k) { Z[12 + k] = (float)(at[k] - v[k]); zf &= refine_finite(at[k] - v[k]); }
      if (!zf) {
        status = VOE_MAP_LOOP_NOT_FINITE;
#pragma unroll
        for (int k = 0; k < 16; ++k) Z[k] = (k % 5 == 0) ? 1.f : 0.f;
      }
    }
    const bool ok = status == VOE_MAP_LOOP_OK;
    n_ok += ok;
    a.edges[2 * l] = i; a.edges[2 * l + 1] = j;
#pragma unroll
    for (int k = 0; k < 16; ++k) a.Z16[16 * (size_t)l + k] = Z[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) a.weights[3 * (size_t)l + k] = ok ? a.w_loop[k] : 0.f;
    int* rec = static_cast<int*>(a.loops) + 10 * (size_t)l;
    rec[0] = i; rec[1] = j; rec[2] = c; rec[3] = n_pairs; rec[4] = rstat; rec[5] = handed; rec[6] = n_in; rec[7] = status;
    rec[8] = __float_as_int(chi_in); rec[9] = __float_as_int(chi_out);
  }
  int tot;
  (void)block_exclusive_scan<LB>(n_ok, s_w, tot);
  if (threadIdx.x == 0) {
    int M = a.hdr[0];
    M = M < a.cap ? M : a.cap;
    M = M < a.bound ? M : a.bound;
    int* si = static_cast<int*>(a.stats);
    si[0] = a.n_frames; si[1] = M; si[2] = a.w.ctl[0]; si[3] = a.w.ctl[1]; si[4] = a.w.ctl[2]; si[5] = tot; si[6] = 0; si[7] = 0;
  }
}

MapLoopsWs map_loops_layout(void* base, int n_frames, int n_max, int bound, int max_loops) {
  MapLoopsWs w{};
  WsCarver c(base);
  const size_t F = (size_t)n_frames, N = (size_t)(n_max > 0 ? n_max : 1), B = (size_t)(bound > 0 ? bound : 1), L = (size_t)max_loops;
  const size_t W = (size_t)covis_words_for((long long)B);
  w.pairs = c.take<int32_t>(8 * F * N);
  w.ent = c.take<int32_t>(4 * F * N);
  w.n_hits = c.take<int>(4 * F);
  w.key = c.take<int>(4 * B);
  w.ref = c.take<int32_t>(4 * 32 * W);
  w.apply_stats = c.take<int>(16);
  w.bits = c.take<uint32_t>(4 * F * W);
  w.cand = c.take<int32_t>(8 * F);
  w.slots = c.take<int32_t>(16 * L);
  w.ctl = c.take<int>(16);
  w.world = c.take<float>(12 * L * N);
  w.uv = c.take<float>(8 * L * N);
  w.lpairs = c.take<int32_t>(8 * L * N);
  w.n_pairs = c.take<int>(4 * L);
  w.handed = c.take<int32_t>(8 * L * N);
  w.n_handed = c.take<int>(4 * L);
  w.rstat = c.take<int>(4 * L);
  w.T_start = c.take<float>(64 * L);
  w.T_solved = c.take<float>(64 * L);
  w.stats4 = c.take<float>(16 * L);
  w.bytes = c.bytes;
  return w;
}

hipError_t launch_map_loops_find(hipStream_t st, const MapLoopsArgs& a) {
  hipLaunchKernelGGL(loops_hist_kernel, dim3(a.n_frames), dim3(LB), 0, st, a);
  hipLaunchKernelGGL(loops_choose_kernel, dim3(1), dim3(LR), 0, st, a);
  hipLaunchKernelGGL(loops_pairs_kernel, dim3(a.max_loops), dim3(LR), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_loops_finish(hipStream_t st, const MapLoopsArgs& a) {
  hipLaunchKernelGGL(loops_finish_kernel, dim3(1), dim3(LB), 0, st, a);
  return hipGetLastError();
}

}  // namespace vo
