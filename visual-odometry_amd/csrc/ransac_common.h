// ransac_common.h -- the device skeleton shared by the two RANSAC front ends: ransac.hip (epipolar initialisation, DESIGN.md
// section 4.9) and pose_ransac.hip (P3P tracking, section 4.10).  Here: the sample rule (the splitmix64 draws of vo_hip.h), the
// scoring tile, the selection of the winner, the tail of the mask kernel and the scatter of the compaction (count / scan /
// scatter).  In each front end's file: its gather and hypothesis kernels, its per-pair predicate, and a model type.
//
// A model M is a compile-time description of one front end, built from that problem's arguments (no function pointers, no
// run-time choice between front ends).  ransac_score_body<M> asks it for
//   M::NT, M::PTS                      threads per workgroup and pairs per thread of the scoring tile (256 and 4);
//   M::Pair, m.load_pair(i),           what a thread keeps in registers for pair i, and the value of a slot past the live
//   M::zero_pair()                     count (never scored);
//   M::Hyp, m.valid(h), m.load(h)      hypothesis h, loaded when valid; both must read the same addresses in every lane
//                                      (wave-uniform loads);
//   m.inlier(hyp, pair)                the predicate, in the front end's own arithmetic and operand order.
#pragma once

#include <hip/hip_runtime.h>

#include "vo_math.h"

namespace vo {

constexpr int RANSAC_HB = 64;      // hypotheses per scoring workgroup: one per lane of the count register

// the sample rule of vo_hip.h, bit for bit
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  unsigned long long z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// draw(h, j) = ((splitmix64(seed ^ ((h << 20) | j)) >> 32) * n) >> 32
__device__ __forceinline__ int ransac_draw(unsigned long long seed, int h, unsigned j, int n) {
  const unsigned long long r = splitmix64(seed ^ (((unsigned long long)h << 20) | j)) >> 32;
  return (int)((r * (unsigned long long)n) >> 32);
}

// The selection, in a workgroup of 1024 threads: hypothesis h is invalid when flag[h * stride] == 0 (its count becomes -1);
// returns, in thread 0, the maximum of (count << 32) | (0xFFFFFFFF - h) over the valid ones -- the most inliers, ties to
// the lowest h -- and 0 when none is valid (a valid key is > 0: h < 2^16)
__device__ __forceinline__ unsigned long long ransac_select_best(int n_hyp, const float* flag, int stride, int* counts) {
  __shared__ unsigned long long s_best[1024 / 64];
  unsigned long long best = 0;
  for (int h = threadIdx.x; h < n_hyp; h += 1024) {
    if (flag[(size_t)h * stride] == 0.f) { counts[h] = -1; continue; }
    const unsigned long long key = ((unsigned long long)(unsigned)counts[h] << 32) | (0xFFFFFFFFull - (unsigned)h);
    if (key > best) best = key;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(best, d);
    if (o > best) best = o;
  }
  if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 0; w < 1024 / 64; ++w) if (s_best[w] > best) best = s_best[w];
  return best;
}

// The scoring tile, the hot path: workgroup (bx, by) holds pairs [bx * NT * PTS, ...) in registers, PTS per thread, and walks
// the block of RANSAC_HB hypotheses from by * RANSAC_HB on.  Per wave one ballot + popcount per hypothesis and pair slot, the
// count parked in the lane of that hypothesis; the waves' counts are summed through LDS and added to counts[] with one
// atomicAdd per (workgroup, hypothesis).  n: the live pairs.
template <class M>
__device__ __forceinline__ void ransac_score_body(const M& m, unsigned bx, unsigned by, int n, int n_hyp, int* counts) {
  __shared__ int s_cnt[M::NT / 64][RANSAC_HB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  typename M::Pair p[M::PTS];
  bool live[M::PTS];
#pragma unroll
  for (int q = 0; q < M::PTS; ++q) {
    const int i = (bx * M::PTS + q) * M::NT + threadIdx.x;
    live[q] = i < n;
    p[q] = live[q] ? m.load_pair(i) : M::zero_pair();
  }
  const int h0 = by * RANSAC_HB;
  const int hn = n_hyp - h0 < RANSAC_HB ? n_hyp - h0 : RANSAC_HB;
  int mine = 0;                                  // the count of hypothesis h0 + lane over this wave's pairs
  for (int k = 0; k < hn; ++k) {
    if (!m.valid(h0 + k)) continue;              // the same addresses in every lane
    const typename M::Hyp hyp = m.load(h0 + k);
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < M::PTS; ++q) cnt += __popcll(__ballot(live[q] && m.inlier(hyp, p[q])));
    if (lane == k) mine = cnt;
  }
  s_cnt[wave][lane] = mine;
  __syncthreads();
  if (threadIdx.x < hn) {
    int v = 0;
#pragma unroll
    for (int w = 0; w < M::NT / 64; ++w) v += s_cnt[w][threadIdx.x];
    if (v) atomicAdd(&counts[h0 + threadIdx.x], v);
  }
}

// The tail of a mask kernel of NT threads: `in` is this thread's predicate for pair bx * NT + threadIdx.x (false past the live
// count); writes the mask byte and the workgroup's count, which the scan turns into the scatter's offset.
template <int NT>
__device__ __forceinline__ void ransac_mask_tail(bool in, unsigned bx, int n_max, uint8_t* mask, int* blk) {
  __shared__ int s_wave[NT / 64];
  const int i = bx * NT + threadIdx.x;
  if (i < n_max) mask[i] = in ? 1 : 0;
  int total;
  block_rank<NT>(in, s_wave, total);
  if (threadIdx.x == 0) blk[bx] = total;
}

// The scatter: the masked pairs in their original order, behind the workgroup's scanned offset
template <int NT>
__device__ __forceinline__ void ransac_scatter_body(unsigned bx, int n_max, const uint8_t* mask, const int* blk, const int32_t* pairs,
                                                    int32_t* out_pairs) {
  __shared__ int s_wave[NT / 64];
  const int i = bx * NT + threadIdx.x;
  const bool in = i < n_max && mask[i];
  int total;
  const int r = block_rank<NT>(in, s_wave, total);
  if (in) reinterpret_cast<int2*>(out_pairs)[blk[bx] + r] = reinterpret_cast<const int2*>(pairs)[i];
}

}  // namespace vo
