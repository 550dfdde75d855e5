// map.hip -- the map of vo_complete on the device: PointCloudVector<3>::update (PointCloud.h:52-66) and the `history`
// chain that moves every frame's triangulated cloud into the first camera's frame (vo_complete.cpp:145-147,175-176).
//
// The reference's update is a sequential double loop: for every point of the cloud, in order, the FIRST map entry whose
// appearance compares equal (operator== on ten floats: -0 == +0, a NaN equals nothing) gets the point; with no such entry
// the (point, appearance) pair is appended -- and is itself found by later points of the same cloud.  What that leaves:
//   * one entry per class of equal appearances, holding the appearance BITS of the class's first occurrence ever
//     and the point of its LAST occurrence so far;
//   * new classes appended in the order of their first occurrence in the cloud;
//   * rows with a NaN always appended, each one, never found.
// Here the classes live in an open-addressing table in device memory keyed by a hash of the canonical row (-0 -> +0), one
// 64-bit word per slot: (tag << 32) | entry.  One update = four launches over the cloud, no host round trip:
//   map_probe_kernel   every cloud row finds or claims its class's slot.  A row that claims writes (tag, M + i) -- M the
//                      map's size, i its index in the cloud -- and equal rows lower that to the smallest i by atomicMin
//                      (an entry < M, i.e. a class the map already holds, is smaller than any of them); the class's last
//                      occurrence is kept beside it by atomicMax.  Slot per row -> scratch.
//   map_flag_kernel    "am I the first occurrence of a new class?" per row; per-workgroup counts and in-group ranks.
//   map_scan_kernel    one workgroup: offsets of the workgroups, new size.
//   map_commit_kernel  first occurrences write their appearance at M + rank; last occurrences write the (moved) point
//                      into the class's entry and turn the slot's provisional M + i into the entry's index.
// The result does not depend on the order in which rows reach the table: min / max over cloud indices decide.
#include "vo_internal.h"

namespace vo {

constexpr int MB = 256;                                   // rows per workgroup
constexpr unsigned long long MAP_EMPTY = ~0ull;
// A class that found no room in the arrays (its entry would have been >= cap) leaves this word in its slot.  A free word there
// would cut the probe chains that run over the slot, and an entry index >= cap would be read as a row of the NEXT update's
// cloud; the marker is neither: probe, lookup and re-hash step over it, nothing claims it, and it goes away when the table is
// rebuilt (growth, vo_map_clear).  No slot's word equals it: entries and provisional indices stay below 2^30.
constexpr unsigned long long MAP_DROPPED = ~0ull - 1ull;

struct MapArgs {
  float* pts;                  // [cap][3]
  float* app;                  // [cap][10]
  unsigned long long* table;   // [tcap] (tag << 32) | entry, MAP_EMPTY when free, MAP_DROPPED where a class found no room
  int* last;                   // [tcap] last cloud index of the slot's class in the running update, -1 otherwise
  unsigned tmask;              // tcap - 1 (a power of two)
  int cap;                     // entries the arrays hold
  int* hdr;                    // [0] size  [1] base of the running update  [2] rows of the running update  [3] rows dropped for lack of room
  const float* c_xyz;          // the cloud
  const float* c_app;
  int n_max;
  const int* d_n;              // or null
  const float* T16;            // isometry applied to every cloud point (device, column-major 4x4) or null
  int* slot;                   // [n_max] scratch: slot of row i, -1 for a NaN row
  int* rank;                   // [n_max] scratch: rank of a first occurrence inside its workgroup
  int* counts;                 // [nb + 1] scratch: per-workgroup counts -> offsets
  int nb;
  const int* guard;            // or null.  A device flag read when the update's launches RUN: where it is 0 all four return at once
                               // and the map, its table and its header keep every byte (voe_map_grow: a fixed sequence of launches)
  __device__ __forceinline__ bool off() const { return guard && *guard == 0; }      // (the same in every thread of a launch)
};

__device__ __forceinline__ Row map_load_row(const float* app, size_t i) {
  const float2* p = reinterpret_cast<const float2*>(app) + 5 * i;
  Row r;
#pragma unroll
  for (int k = 0; k < 5; ++k) { const float2 t = p[k]; r.v[2 * k] = t.x; r.v[2 * k + 1] = t.y; }
  return r;
}
// Row, map_row_has_nan, map_rows_equal, map_hash and map_home_slot: vo_math.h (the host build of the tests runs them too)

__global__ __launch_bounds__(MB) void map_probe_kernel(MapArgs a) {
  if (a.off()) return;
  const int n = live_rows(a.d_n, a.n_max);
  const int M = a.hdr[0];
  const int i = blockIdx.x * MB + threadIdx.x;
  if (i >= n) return;
  const Row r = map_load_row(a.c_app, (size_t)i);
  if (map_row_has_nan(r)) { a.slot[i] = -1; return; }
  const unsigned h = map_hash(r);
  const unsigned long long mine = ((unsigned long long)h << 32) | (unsigned)(M + i);
  unsigned s = map_home_slot(h, a.tmask);
  int found = -2;
  for (unsigned probes = 0; probes <= a.tmask; ++probes, s = (s + 1) & a.tmask) {
    unsigned long long w = a.table[s];
    if (w == MAP_EMPTY) {
      w = atomicCAS(&a.table[s], MAP_EMPTY, mine);
      if (w == MAP_EMPTY) { found = (int)s; break; }        // claimed
    }
    if (w == MAP_DROPPED || (unsigned)(w >> 32) != h) continue;      // a class that was dropped, or another class, lives here
    // w names an entry (< M: commit leaves nothing else behind) or a row of THIS cloud (M + i', i' < n: written above by a
    // thread of this launch)
    const unsigned e = (unsigned)w;
    const Row o = e < (unsigned)M ? map_load_row(a.app, (size_t)e) : map_load_row(a.c_app, (size_t)(e - (unsigned)M));
    if (!map_rows_equal(r, o)) continue;                    // same tag, another row
    // my class: from here on the slot only ever holds members of it, so the minimum keeps the map's entry if there is
    // one and the first occurrence in the cloud otherwise
    atomicMin(&a.table[s], mine);
    found = (int)s;
    break;
  }
  a.slot[i] = found;                                        // (-2: the table is full -- the host keeps it at most half full)
  if (found >= 0) atomicMax(&a.last[found], i);
  else atomicAdd(&a.hdr[3], 1);                             // a row without a slot is a row dropped (hdr[3] is read by no launch of the update)
}

__global__ __launch_bounds__(MB) void map_flag_kernel(MapArgs a) {
  __shared__ int s_wave[MB / 64];
  if (a.off()) return;
  const int n = live_rows(a.d_n, a.n_max);
  const int M = a.hdr[0];
  const int i = blockIdx.x * MB + threadIdx.x;
  bool first = false;
  if (i < n) {
    const int s = a.slot[i];
    first = s == -1 || (s >= 0 && (unsigned)a.table[s] == (unsigned)(M + i));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(first);
  if (lane == 0) s_wave[wave] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < MB / 64; ++w) { const int c = s_wave[w]; if (w < wave) off += c; tot += c; }
  if (i < a.n_max) a.rank[i] = first ? off + __popcll(m & ((1ull << lane) - 1ull)) : -1;
  if (threadIdx.x == 0) a.counts[blockIdx.x] = tot;
}

__global__ __launch_bounds__(1024) void map_scan_kernel(MapArgs a) {
  __shared__ int s_w[16];
  __shared__ int s_carry;
  if (a.off()) return;
  const int sum = scan_with_carry<1024>(a.counts, a.nb, s_w, &s_carry);
  if (threadIdx.x == 0) {
    const int M = a.hdr[0];
    int add = sum;
    int dropped = 0;
    if (M + add > a.cap) { dropped = M + add - a.cap; add = a.cap - M; }      // (the host grows the arrays before this can happen)
    a.hdr[1] = M;
    a.hdr[2] = live_rows(a.d_n, a.n_max);
    a.hdr[3] += dropped;
    a.hdr[0] = M + add;
  }
}

__global__ __launch_bounds__(MB) void map_commit_kernel(MapArgs a) {
  if (a.off()) return;
  const int n = a.hdr[2];
  const int M = a.hdr[1];
  const int i = blockIdx.x * MB + threadIdx.x;
  if (i >= n) return;
  const int s = a.slot[i];
  if (s == -2) return;
  const int rk = a.rank[i];
  if (rk >= 0) {                                            // first occurrence of a new class (or a NaN row): its appearance, bit for bit
    const int e = M + a.counts[blockIdx.x] + rk;
    if (e < a.cap) {
      const float2* src = reinterpret_cast<const float2*>(a.c_app) + 5 * (size_t)i;
      float2* dst = reinterpret_cast<float2*>(a.app) + 5 * (size_t)e;
#pragma unroll
      for (int k = 0; k < 5; ++k) dst[k] = src[k];
    }
  }
  int e;                                                    // the entry this row's point goes to, if it is its class's last occurrence
  if (s == -1) {
    e = M + a.counts[blockIdx.x] + rk;
  } else {
    if (a.last[s] != i) return;
    const unsigned idx = (unsigned)a.table[s];
    if (idx < (unsigned)M) {
      e = (int)idx;
    } else {
      const int f = (int)(idx - (unsigned)M);               // the class's first occurrence in this cloud
      e = M + a.counts[f / MB] + a.rank[f];
      // the slot now names the entry, or says that the class was dropped (only this thread touches the slot in this launch)
      a.table[s] = e < a.cap ? ((a.table[s] & 0xffffffff00000000ull) | (unsigned)e) : MAP_DROPPED;
    }
    a.last[s] = -1;
  }
  if (e >= a.cap) return;
  float x = a.c_xyz[3 * (size_t)i], y = a.c_xyz[3 * (size_t)i + 1], z = a.c_xyz[3 * (size_t)i + 2];
  if (a.T16) {                                              // history * triangulated_pc (vo_complete.cpp:175, PointCloud.h:80)
    float t[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) t[k] = a.T16[k];
    const Pose X = pose_from_T16(t);
    const float px = x, py = y, pz = z;
    pose_apply(X, px, py, pz, x, y, z);
  }
  a.pts[3 * (size_t)e] = x; a.pts[3 * (size_t)e + 1] = y; a.pts[3 * (size_t)e + 2] = z;
}

// rebuilds the table from the entries (after the arrays grew): entry j claims or joins its class's slot; the smallest j stays
// (guard: launch_map_rehash)
__global__ __launch_bounds__(MB) void map_rehash_kernel(MapArgs a, const int* guard) {
  if (guard && *guard == 0) return;
  const int M = a.hdr[0];
  const int j = blockIdx.x * MB + threadIdx.x;
  if (j >= M) return;
  const Row r = map_load_row(a.app, (size_t)j);
  if (map_row_has_nan(r)) return;
  const unsigned h = map_hash(r);
  const unsigned long long mine = ((unsigned long long)h << 32) | (unsigned)j;
  unsigned s = map_home_slot(h, a.tmask);
  for (unsigned probes = 0; probes <= a.tmask; ++probes, s = (s + 1) & a.tmask) {
    unsigned long long w = a.table[s];
    if (w == MAP_EMPTY) {
      w = atomicCAS(&a.table[s], MAP_EMPTY, mine);
      if (w == MAP_EMPTY) return;
    }
    if (w == MAP_DROPPED || (unsigned)(w >> 32) != h) continue;
    if (!map_rows_equal(r, map_load_row(a.app, (size_t)(unsigned)w))) continue;
    atomicMin(&a.table[s], mine);
    return;
  }
}

// history <- X^-1 (reset != 0, vo_complete.cpp:146) or history * X^-1 (vo_complete.cpp:176): Isometry3f arithmetic in float,
// Eigen's order (vo_math.h: pose_inverse, pose_mul), one thread
__global__ void map_history_kernel(float* hist16, const float* X16, int reset) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float t[16];
  for (int k = 0; k < 16; ++k) t[k] = X16[k];
  const Pose Xi = pose_inverse(pose_from_T16(t));
  Pose H = Xi;
  if (!reset) {
    for (int k = 0; k < 16; ++k) t[k] = hist16[k];
    H = pose_mul(pose_from_T16(t), Xi);
  }
  pose_to_T16(H, t);
  for (int k = 0; k < 16; ++k) hist16[k] = t[k];
}

// map <- T * map (vo_complete.cpp:183), in place
__global__ __launch_bounds__(256) void map_transform_kernel(MapArgs a, Pose T) {
  const int M = a.hdr[0];
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < M; j += gridDim.x * blockDim.x) {
    float* p = a.pts + 3 * (size_t)j;
    float x, y, z;
    pose_apply(T, p[0], p[1], p[2], x, y, z);
    p[0] = x; p[1] = y; p[2] = z;
  }
}

// ---- the read-only side: which entry would update() have found for this row? ---------------------------------------------
// map_lookup_probe_kernel walks the table exactly as map_probe_kernel does (same hash, same home slot, same linear step) but
// only reads: it stops at the first free word, skips words of another tag or of another row, and takes the entry of the first
// word whose row compares equal -- the class's entry, since a class owns one slot.  No atomics, no store to the table or the
// entries.  Then count / scan / scatter compact the hits by QUERY index: the result is a function of the data alone.
__global__ __launch_bounds__(MB) void map_lookup_probe_kernel(MapLookupArgs a) {
  __shared__ int s_wave[MB / 64];
  const FrameBlock fb = frame_block(a.nb, a.n_frames);
  if (!fb.live) return;                                     // (the whole workgroup)
  const int n = live_rows(a.d_n ? a.d_n + fb.f : nullptr, a.n_max);      // (a null d_n stays null: every frame holds n_max)
  int M = a.hdr[0];
  M = M < a.cap ? M : a.cap;
  const int i = fb.b * MB + threadIdx.x;
  int found = -1;
  if (i < n) {
    const Row r = map_load_row(a.q_app + (size_t)fb.f * a.q_stride, (size_t)i);
    if (!map_row_has_nan(r)) {
      const unsigned h = map_hash(r);
      unsigned s = map_home_slot(h, a.tmask);               // the home slot of map_probe_kernel
      for (unsigned probes = 0; probes <= a.tmask; ++probes, s = (s + 1) & a.tmask) {
        const unsigned long long w = a.table[s];
        if (w == MAP_EMPTY) break;                          // the class was never entered
        if (w == MAP_DROPPED || (unsigned)(w >> 32) != h) continue;      // a dropped class, or another class, lives here
        const unsigned e = (unsigned)w;
        if (e >= (unsigned)M) continue;                     // (never, between updates: a slot names an entry)
        if (!map_rows_equal(r, map_load_row(a.app, (size_t)e))) continue;   // same tag, another row
        found = (int)e;
        break;
      }
    }
  }
  if (i < a.n_max) a.ent[(size_t)fb.f * a.n_max + i] = found;
  const unsigned long long m = __ballot(found >= 0);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
#pragma unroll
    for (int w = 0; w < MB / 64; ++w) tot += s_wave[w];
    a.counts[(size_t)fb.f * a.counts_stride + fb.b] = tot;
  }
}

__global__ __launch_bounds__(MB) void map_lookup_scatter_kernel(MapLookupArgs a) {
  __shared__ int s_wave[MB / 64];
  const FrameBlock fb = frame_block(a.nb, a.n_frames);
  if (!fb.live) return;
  const int i = fb.b * MB + threadIdx.x;
  const int e = i < a.n_max ? a.ent[(size_t)fb.f * a.n_max + i] : -1;      // (-1 beyond the live rows)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(e >= 0);
  if (lane == 0) s_wave[wave] = __popcll(m);
  __syncthreads();
  if (e < 0) return;
  int off = a.counts[(size_t)fb.f * a.counts_stride + fb.b];
#pragma unroll
  for (int w = 0; w < MB / 64; ++w) if (w < wave) off += s_wave[w];
  const size_t k = (size_t)(off + __popcll(m & ((1ull << lane) - 1ull)));      // < n_max: one hit per live row at most
  const size_t o = (size_t)fb.f * a.n_max + k;
  if (a.pairs) reinterpret_cast<int2*>(a.pairs)[o] = make_int2(i, e);
  if (a.local_pairs) reinterpret_cast<int2*>(a.local_pairs)[o] = make_int2(i, (int)k);
  if (a.xyz) {
    const float* p = a.pts + 3 * (size_t)e;
    float* q = a.xyz + 3 * o;
    q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
  }
}

// one thread per frame: the status of vo_map_localise*_dev, the pose handed out and the statistics (8 words per frame:
// status, live rows, hits, RANSAC status, pairs handed to the solver, the solver's inliers, chi^2 of inliers / outliers)
__global__ __launch_bounds__(64) void map_localise_finish_kernel(MapLocaliseFinish a) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= a.n_frames) return;
  int rows = a.n_max;
  if (a.d_n) { const int m = a.d_n[f]; rows = m < rows ? (m < 0 ? 0 : m) : rows; }
  const int hits = a.n_hits[f];
  const int rstat = a.ransac_status ? a.ransac_status[f] : 0;
  const int handed = a.n_handed[f];
  float T[16];
  int n_in;
  float chi_in, chi_out;
  if (a.state) {                                            // the single solver: its pose as vo_picp_get_pose_dev writes it
    const float* p = a.state->pose[0];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int r = k & 3, c = k >> 2;
      T[k] = r == 3 ? (c == 3 ? 1.f : 0.f) : (c == 3 ? p[9 + r] : p[r + 3 * c]);
    }
    n_in = a.state->n_in; chi_in = a.state->chi_in; chi_out = a.state->chi_out;
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) T[k] = a.T_solved[16 * (size_t)f + k];
    chi_in = a.stats4[4 * (size_t)f]; chi_out = a.stats4[4 * (size_t)f + 1]; n_in = (int)a.stats4[4 * (size_t)f + 2];
  }
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 16; ++k) finite &= fabsf(T[k]) <= 3.402823466e38f;      // false for NaN and +-inf
  int status = 0;
  if (hits < 6) status = 1;
  else if (rstat != 0) status = 2;
  else if (!finite) status = 4;
  else if (n_in < a.min_inliers) status = 3;
  float* out = a.T_out + 16 * (size_t)f;
  if (status == 0) {
#pragma unroll
    for (int k = 0; k < 16; ++k) out[k] = T[k];
  } else if (a.T0) {
    const unsigned* src = reinterpret_cast<const unsigned*>(a.T0) + 16 * (size_t)f;      // T0's bits, whatever they are
    unsigned* dst = reinterpret_cast<unsigned*>(out);
#pragma unroll
    for (int k = 0; k < 16; ++k) dst[k] = src[k];
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) out[k] = (k % 5 == 0) ? 1.f : 0.f;
  }
  int* s = a.stats + 8 * (size_t)f;
  s[0] = status; s[1] = rows; s[2] = hits; s[3] = rstat; s[4] = handed; s[5] = n_in;
  s[6] = __float_as_int(chi_in); s[7] = __float_as_int(chi_out);
}

size_t map_scratch_ints(int n_max) { return 2 * (size_t)n_max + (size_t)((n_max + MB - 1) / MB) + 8; }

static size_t lookup_counts_stride(int n_max) { const size_t nb = (size_t)((n_max + MB - 1) / MB); return ((nb ? nb : 1) + 3) & ~(size_t)3; }
size_t map_lookup_scratch_ints(int n_max, int n_frames, bool with_entries) {
  return (size_t)n_frames * (lookup_counts_stride(n_max) + (with_entries ? (size_t)n_max : 0)) + 8;
}

hipError_t launch_map_lookup(hipStream_t st, const MapDev& m, const float* d_app, size_t app_stride_rows, int n_max, const int* d_n,
                             int n_frames, int32_t* d_pairs, int* d_n_out, float* d_xyz, int32_t* d_local_pairs, int32_t* d_entries,
                             int* d_scratch) {
  if (n_max <= 0) return hipMemsetAsync(d_n_out, 0, sizeof(int) * (size_t)n_frames, st);
  MapLookupArgs a;
  a.app = m.app; a.pts = m.pts; a.table = m.table; a.hdr = m.hdr; a.tmask = m.tcap - 1u; a.cap = m.cap;
  a.q_app = d_app; a.q_stride = 10 * app_stride_rows; a.n_max = n_max; a.d_n = d_n; a.n_frames = n_frames;
  a.nb = (n_max + MB - 1) / MB;
  a.counts_stride = lookup_counts_stride(n_max);
  a.counts = d_scratch;
  a.ent = d_entries ? d_entries : d_scratch + (size_t)n_frames * a.counts_stride;
  a.pairs = d_pairs; a.local_pairs = d_local_pairs; a.xyz = d_xyz;
  hipLaunchKernelGGL(map_lookup_probe_kernel, frame_grid(a.nb, n_frames), dim3(MB), 0, st, a);
  hipError_t e = launch_scan(st, a.counts, a.nb, d_n_out, nullptr, n_frames, a.counts_stride);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(map_lookup_scatter_kernel, frame_grid(a.nb, n_frames), dim3(MB), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_localise_finish(hipStream_t st, const MapLocaliseFinish& a) {
  hipLaunchKernelGGL(map_localise_finish_kernel, dim3((a.n_frames + 63) / 64), dim3(64), 0, st, a);
  return hipGetLastError();
}

static MapArgs map_args(const MapDev& m, const float* c_xyz, const float* c_app, int n_max, const int* d_n, const float* T16,
                        int* scratch) {
  MapArgs a;
  a.pts = m.pts; a.app = m.app; a.table = m.table; a.last = m.last; a.tmask = m.tcap - 1u; a.cap = m.cap; a.hdr = m.hdr;
  a.c_xyz = c_xyz; a.c_app = c_app; a.n_max = n_max; a.d_n = d_n; a.T16 = T16;
  a.nb = (n_max + MB - 1) / MB;
  a.slot = scratch; a.rank = scratch + n_max; a.counts = scratch + 2 * (size_t)n_max;
  a.guard = nullptr;
  return a;
}

hipError_t launch_map_update(hipStream_t st, const MapDev& m, const float* c_xyz, const float* c_app, int n_max, const int* d_n,
                             const float* d_T16, int* d_scratch, const int* d_guard) {
  if (n_max <= 0) return hipSuccess;
  MapArgs a = map_args(m, c_xyz, c_app, n_max, d_n, d_T16, d_scratch);
  a.guard = d_guard;
  hipLaunchKernelGGL(map_probe_kernel, dim3(a.nb), dim3(MB), 0, st, a);
  hipLaunchKernelGGL(map_flag_kernel, dim3(a.nb), dim3(MB), 0, st, a);
  hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(1024), 0, st, a);
  hipLaunchKernelGGL(map_commit_kernel, dim3(a.nb), dim3(MB), 0, st, a);
  return hipGetLastError();
}

// the guarded form's clear of table and last: what the two memsets of the unguarded form write, where the flag is not 0
__global__ __launch_bounds__(MB) void map_table_clear_kernel(MapArgs a, const int* guard) {
  if (*guard == 0) return;
  for (size_t s = (size_t)blockIdx.x * MB + threadIdx.x; s <= (size_t)a.tmask; s += (size_t)gridDim.x * MB) {
    a.table[s] = MAP_EMPTY;
    a.last[s] = -1;
  }
}

hipError_t launch_map_rehash(hipStream_t st, const MapDev& m, int size_bound, const int* d_guard) {
  const MapArgs a = map_args(m, nullptr, nullptr, 0, nullptr, nullptr, nullptr);
  if (d_guard) {
    const unsigned want = (m.tcap + MB - 1) / MB;
    hipLaunchKernelGGL(map_table_clear_kernel, dim3(want < 4096u ? want : 4096u), dim3(MB), 0, st, a, d_guard);
  } else {
    hipError_t e = hipMemsetAsync(m.table, 0xff, sizeof(unsigned long long) * (size_t)m.tcap, st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(m.last, 0xff, sizeof(int) * (size_t)m.tcap, st);
    if (e != hipSuccess) return e;
  }
  if (size_bound <= 0) return hipGetLastError();
  hipLaunchKernelGGL(map_rehash_kernel, dim3((size_bound + MB - 1) / MB), dim3(MB), 0, st, a, d_guard);
  return hipGetLastError();
}

hipError_t launch_map_history(hipStream_t st, float* d_hist16, const float* d_X16, int reset) {
  hipLaunchKernelGGL(map_history_kernel, dim3(1), dim3(64), 0, st, d_hist16, d_X16, reset);
  return hipGetLastError();
}

hipError_t launch_map_transform(hipStream_t st, const MapDev& m, const Pose& T, int size_bound) {
  if (size_bound <= 0) return hipSuccess;
  const MapArgs a = map_args(m, nullptr, nullptr, 0, nullptr, nullptr, nullptr);
  int grid = (size_bound + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(map_transform_kernel, dim3(grid), dim3(256), 0, st, a, T);
  return hipGetLastError();
}

}  // namespace vo
