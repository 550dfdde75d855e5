// ransac_common.h -- device pieces shared by the two RANSAC front ends: ransac.hip (epipolar initialisation, DESIGN.md
// section 4.9) and pose_ransac.hip (P3P tracking, section 4.10).  Both draw their samples by the splitmix64 rule of
// vo_hip.h, select the winner by the same key and compact the winner's inliers by count / scan / scatter.
#pragma once

#include <hip/hip_runtime.h>

namespace vo {

// live rows: *d_n clamped to [0, n_max], or n_max when d_n is null
__device__ __forceinline__ int ransac_rows(const int* d_n, int n_max) {
  int n = n_max;
  if (d_n) { const int m = *d_n; n = m < n ? (m < 0 ? 0 : m) : n; }
  return n;
}

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

// exclusive rank of `flag` inside a workgroup of NT threads (as geom.hip's block_rank); total = flags set
template <int NT>
__device__ __forceinline__ int ransac_rank(bool flag, int* s_wave, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int before = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) s_wave[wave] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const int c = s_wave[w];
    if (w < wave) off += c;
    tot += c;
  }
  total = tot;
  return off + before;
}

}  // namespace vo
