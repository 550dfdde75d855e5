// covis_rules.h -- the small integer rules of map_covis.hip (include/vo_map_covis.h), as inline functions that the kernels and
// a host check (tests/hostcheck/covis_check.cpp) compile from this one text: where an entry's bit lies, how the tiles of the
// upper triangle of the frame-pair matrix are numbered, and the key the window's two rankings sort by.  No floating point.
#ifndef VO_COVIS_RULES_H
#define VO_COVIS_RULES_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define COVIS_HD __host__ __device__ inline
#else
#define COVIS_HD inline
#endif

namespace vo {

constexpr int COVIS_TILE = 32;            // frames along one edge of a tile of frame pairs
constexpr int COVIS_CHUNK = 64;           // 32-bit words of a row staged in LDS per step

// entry e lives in bit covis_bit(e) of word covis_word(e) of its frame's row
COVIS_HD int covis_word(int e) { return e >> 5; }
COVIS_HD uint32_t covis_bit(int e) { return 1u << (e & 31); }
// the words a map of `size` entries needs
COVIS_HD int covis_words_for(long long size) { return (int)((size + 31) / 32); }
// row f of a bit matrix of n_words words per row
COVIS_HD size_t covis_row(int f, int n_words) { return (size_t)f * (size_t)n_words; }

// the tiles along one edge, and the tiles on or above the diagonal
COVIS_HD int covis_tiles_edge(int n_frames) { return (n_frames + COVIS_TILE - 1) / COVIS_TILE; }
COVIS_HD int covis_tiles(int n_frames) { const int T = covis_tiles_edge(n_frames); return T * (T + 1) / 2; }
// tile t of the upper triangle, row by row: (0,0) (0,1) ... (0,T-1) (1,1) ... (T-1,T-1).  ti <= tj.  T <= 128: the walk is short.
COVIS_HD void covis_tile(int t, int T, int* ti, int* tj) {
  int i = 0;
  while (t >= T - i) { t -= T - i; ++i; }
  *ti = i; *tj = i + t;
}

// The rankings of the window: a larger count first, among equal counts the smaller frame first.  One 64-bit key, ascending.
COVIS_HD uint64_t covis_rank_key(int count, int frame) {
  return ((uint64_t)(uint32_t)(0x7fffffff - count) << 32) | (uint64_t)(uint32_t)frame;
}

}  // namespace vo
#endif
