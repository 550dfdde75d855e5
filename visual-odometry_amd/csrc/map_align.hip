// map_align.hip -- two maps (voe_map_align* / voe_map_merge*, include/vo_map_align.h holds the rules).
// The alignment is the third front end of ransac_common.h, a 3-point similarity:
//   align_gather_kernel   one float4 + one float2 per match: src's point a and dst's point b;
//   align_hyp_kernel      one thread per hypothesis, in double: the sample (first 3 distinct draws), Umeyama's closed form on
//                         the three pairs with the facade's 3x3 SVD (linalg::svd3), rounded to float;
//   align_score_kernel    the hot path, ransac_common.h's scoring tile on AlignModel: |M a + t - b|^2 in float, fixed FMA order;
//   align_select_kernel   one workgroup: the winner (ransac_common.h) and the number of valid hypotheses;
//   per refit round       align_sums_kernel (the inliers of the current model: count, sum a, sum b per block of 256 pairs),
//                         align_moments_kernel (every block reduces the blocks' sums to the centroids, then its centred moments),
//                         align_solve_kernel (one workgroup: the moments, Umeyama, the new model);
//   align_decide_kernel   one workgroup: refit or winner, the status;
//   align_out_kernel      the mask and the squared residuals of the final inliers per block, in double;
//   align_finish_kernel   one workgroup: rms, S and the statistics.
// Every floating-point sum is a tree of fixed shape over LDS (block_tree_sum, lm_pcg.h), per block and then over the blocks: no float
// atomics, the same bytes from every call.  The merge's own kernels (the misses of a lookup compacted in order: count / scan /
// scatter) are at the end; lookup and update are map.hip's, through their public entry points (capi_map.hip).
#include "vo_internal.h"
#include "ransac_common.h"
#include "../../include/vo_hip.h"
#include "../../include/vo/linalg.hpp"

namespace vo {

namespace {

constexpr int AB = 256;            // threads per workgroup = pairs per block of every sum
constexpr int ALIGN_PTS = 4;       // pairs per thread of the scoring pass

// the blocks' rows summed: thread t adds rows t, t + AB, ... in ascending order, then the tree
template <int K>
__device__ __forceinline__ void rows_sum(const double* rows, int nb, double (&v)[K], double* s) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0.0;
  for (int j = threadIdx.x; j < nb; j += AB) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += rows[(size_t)j * K + k];
  }
  block_tree_sum<K>(v, s);
}

// the sum of the blocks' inlier counts (integers: any order), in every thread
__device__ __forceinline__ int counts_sum(const int* blk, int nb) {
  __shared__ int s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  int c = 0;
  for (int j = threadIdx.x; j < nb; j += AB) c += blk[j];
  if (c) atomicAdd(&s_cnt, c);
  __syncthreads();
  const int total = s_cnt;
  __syncthreads();
  return total;
}

struct Sim { double M[9], t[3], c; };      // M = c R column-major

// Umeyama's closed form from the moments: Sg row-major, Sg[3 i + j] = mean db_i da_j; false: invalid
__device__ bool umeyama(const double Sg[9], double var_a, const double ca[3], const double cb[3], int with_scale, Sim& o) {
  if (!(var_a > 0.0) || !isfinite(var_a)) return false;
  linalg::Mat3d S, U, V;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) S.m[i][j] = Sg[3 * i + j];
  double s[3];
  linalg::svd3(S, U, s, V);
  if (!(s[1] > 1e-9 * s[0])) return false;                     // rank < 2 (a NaN fails too)
  const double d = U.det() * V.det() < 0.0 ? -1.0 : 1.0;
  const double c = with_scale ? (s[0] + s[1] + d * s[2]) / var_a : 1.0;
  if (!(c > 0.0)) return false;
  bool finite = isfinite(c);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double r = U.m[i][0] * V.m[j][0] + U.m[i][1] * V.m[j][1] + d * (U.m[i][2] * V.m[j][2]);
      o.M[i + 3 * j] = c * r;
      finite &= isfinite(o.M[i + 3 * j]);
    }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    o.t[i] = cb[i] - (o.M[i] * ca[0] + o.M[i + 3] * ca[1] + o.M[i + 6] * ca[2]);
    finite &= isfinite(o.t[i]);
  }
  o.c = c;
  return finite;
}

__device__ __forceinline__ void sim_to_floats(const Sim& s, float* out) {
#pragma unroll
  for (int k = 0; k < 9; ++k) out[k] = (float)s.M[k];
  out[9] = (float)s.t[0]; out[10] = (float)s.t[1]; out[11] = (float)s.t[2];
  out[12] = 1.f; out[13] = out[14] = out[15] = 0.f;
}

struct AlignHyp { float M[9], t[3]; };
struct AlignPair { float4 p; float2 q; };       // (a0, a1, a2, b0), (b1, b2)

__device__ __forceinline__ AlignHyp load_hyp(const float* g) {
  AlignHyp m;
#pragma unroll
  for (int k = 0; k < 9; ++k) m.M[k] = g[k];
  m.t[0] = g[9]; m.t[1] = g[10]; m.t[2] = g[11];
  return m;
}

// the float32 predicate of the header, in its FMA order; strict, a NaN never passes
__device__ __forceinline__ bool align_inlier(const AlignHyp& m, const AlignPair& x, float thr2) {
  const float r0 = __builtin_fmaf(m.M[0], x.p.x, __builtin_fmaf(m.M[3], x.p.y, __builtin_fmaf(m.M[6], x.p.z, m.t[0]))) - x.p.w;
  const float r1 = __builtin_fmaf(m.M[1], x.p.x, __builtin_fmaf(m.M[4], x.p.y, __builtin_fmaf(m.M[7], x.p.z, m.t[1]))) - x.q.x;
  const float r2 = __builtin_fmaf(m.M[2], x.p.x, __builtin_fmaf(m.M[5], x.p.y, __builtin_fmaf(m.M[8], x.p.z, m.t[2]))) - x.q.y;
  return __builtin_fmaf(r0, r0, __builtin_fmaf(r1, r1, r2 * r2)) < thr2;
}

// the squared residual of the statistics: double, from the float32 model and points widened, left to right
__device__ __forceinline__ double align_d2(const AlignHyp& m, const AlignPair& x) {
  const double a0 = x.p.x, a1 = x.p.y, a2 = x.p.z;
  const double r0 = (((double)m.M[0] * a0 + (double)m.M[3] * a1) + (double)m.M[6] * a2 + (double)m.t[0]) - (double)x.p.w;
  const double r1 = (((double)m.M[1] * a0 + (double)m.M[4] * a1) + (double)m.M[7] * a2 + (double)m.t[1]) - (double)x.q.x;
  const double r2 = (((double)m.M[2] * a0 + (double)m.M[5] * a1) + (double)m.M[8] * a2 + (double)m.t[2]) - (double)x.q.y;
  return (r0 * r0 + r1 * r1) + r2 * r2;
}

struct AlignModel {
  static constexpr int NT = AB, PTS = ALIGN_PTS;
  using Pair = AlignPair;
  using Hyp = AlignHyp;
  const MapAlignArgs& a;
  __device__ __forceinline__ Pair load_pair(int i) const { return Pair{a.pa[i], a.pb[i]}; }
  static __device__ __forceinline__ Pair zero_pair() { return Pair{make_float4(0.f, 0.f, 0.f, 0.f), make_float2(0.f, 0.f)}; }
  __device__ __forceinline__ bool valid(int h) const { return !(a.hyp[(size_t)h * ALIGN_FS + 12] == 0.f); }
  __device__ __forceinline__ Hyp load(int h) const { return load_hyp(a.hyp + (size_t)h * ALIGN_FS); }
  __device__ __forceinline__ bool inlier(const Hyp& m, const Pair& p) const { return align_inlier(m, p, a.thr2); }
};

}  // namespace

__global__ __launch_bounds__(AB) void align_gather_kernel(MapAlignArgs a) {
  const int n = live_rows(a.d_n, a.n_max);
  for (int i = blockIdx.x * AB + threadIdx.x; i < n; i += gridDim.x * AB) {
    const int2 pr = reinterpret_cast<const int2*>(a.pairs)[i];            // (src entry < n_max, dst entry): the lookup's
    const float qnan = __int_as_float(0x7fc00000);
    float4 p = make_float4(qnan, qnan, qnan, qnan);
    if (pr.x >= 0 && pr.x < a.n_max) {
      const float* s = a.src_pts + 3 * (size_t)pr.x;
      p = make_float4(s[0], s[1], s[2], a.bxyz[3 * (size_t)i]);
    }
    a.pa[i] = p;
    a.pb[i] = make_float2(a.bxyz[3 * (size_t)i + 1], a.bxyz[3 * (size_t)i + 2]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl->n = n;
}

__global__ __launch_bounds__(64) void align_hyp_kernel(MapAlignArgs a) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= a.n_hyp) return;
  const int n = live_rows(a.d_n, a.n_max);
  int i0 = 0, i1 = 0, i2 = 0, k = 0;                       // the first 3 distinct draws, in registers
  if (n >= 3)
    for (unsigned j = 0; j < 64 && k < 3; ++j) {
      const int v = ransac_draw(a.seed, h, j, n);
      if ((k < 1 || v != i0) && (k < 2 || v != i1)) {
        i0 = k == 0 ? v : i0; i1 = k == 1 ? v : i1; i2 = k == 2 ? v : i2;
        ++k;
      }
    }
  float out[ALIGN_FS];
#pragma unroll
  for (int c = 0; c < ALIGN_FS; ++c) out[c] = 0.f;
  double scale = 0.0;
  if (k == 3) {
    const float4 p0 = a.pa[i0], p1 = a.pa[i1], p2 = a.pa[i2];
    const float2 q0 = a.pb[i0], q1 = a.pb[i1], q2 = a.pb[i2];
    const double A[3][3] = {{p0.x, p0.y, p0.z}, {p1.x, p1.y, p1.z}, {p2.x, p2.y, p2.z}};
    const double B[3][3] = {{p0.w, q0.x, q0.y}, {p1.w, q1.x, q1.y}, {p2.w, q2.x, q2.y}};
    double ca[3], cb[3], Sg[9], var_a = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) { ca[i] = (A[0][i] + A[1][i] + A[2][i]) / 3.0; cb[i] = (B[0][i] + B[1][i] + B[2][i]) / 3.0; }
#pragma unroll
    for (int c = 0; c < 9; ++c) Sg[c] = 0.0;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      double da[3], db[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) { da[i] = A[p][i] - ca[i]; db[i] = B[p][i] - cb[i]; }
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Sg[3 * i + j] += db[i] * da[j];
      var_a += da[0] * da[0] + da[1] * da[1] + da[2] * da[2];
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) Sg[c] /= 3.0;
    var_a /= 3.0;
    Sim s;
    if (umeyama(Sg, var_a, ca, cb, a.with_scale, s)) { sim_to_floats(s, out); scale = s.c; }
  }
  float4* dst = reinterpret_cast<float4*>(a.hyp + (size_t)h * ALIGN_FS);
  dst[0] = make_float4(out[0], out[1], out[2], out[3]);
  dst[1] = make_float4(out[4], out[5], out[6], out[7]);
  dst[2] = make_float4(out[8], out[9], out[10], out[11]);
  dst[3] = make_float4(out[12], out[13], out[14], out[15]);
  a.hyp_scale[h] = scale;
}

__global__ __launch_bounds__(AB) void align_score_kernel(MapAlignArgs a) {
  ransac_score_body(AlignModel{a}, blockIdx.x, blockIdx.y, live_rows(a.d_n, a.n_max), a.n_hyp, a.counts);
}

__global__ __launch_bounds__(1024) void align_select_kernel(MapAlignArgs a) {
  __shared__ int s_valid;
  if (threadIdx.x == 0) s_valid = 0;
  __syncthreads();
  int nv = 0;
  for (int h = threadIdx.x; h < a.n_hyp; h += 1024) nv += a.hyp[(size_t)h * ALIGN_FS + 12] != 0.f;
  if (nv) atomicAdd(&s_valid, nv);
  const unsigned long long best = ransac_select_best(a.n_hyp, a.hyp + 12, ALIGN_FS, a.counts);      // (synchronises)
  if (threadIdx.x == 0) {
    MapAlignCtl* c = a.ctl;
    const int win = best ? (int)(0xFFFFFFFFull - (best & 0xFFFFFFFFull)) : -1;
    c->win_h = win; c->win_cnt = best ? (int)(best >> 32) : 0; c->n_valid = s_valid;
    for (int k = 0; k < ALIGN_FS; ++k) {
      const float v = win >= 0 ? a.hyp[(size_t)win * ALIGN_FS + k] : 0.f;
      c->win[k] = v; c->cur[k] = v; c->ref[k] = 0.f;
    }
    c->scale_win = c->scale_cur = win >= 0 ? a.hyp_scale[win] : 0.0;
    c->scale_ref = 0.0;
    c->alive = win >= 0 && a.n_refits > 0;
    c->have_ref = 0; c->cnt_cur = 0;
  }
}

// the inliers of the current model: per block of AB pairs their count and the sums of a and of b
__global__ __launch_bounds__(AB) void align_sums_kernel(MapAlignArgs a) {
  __shared__ double s[ALIGN_SUMS * AB];
  __shared__ int s_wave[AB / 64];
  if (!a.ctl->alive) return;                                // (the whole grid)
  const int n = live_rows(a.d_n, a.n_max);
  const int i = blockIdx.x * AB + threadIdx.x;
  const AlignHyp m = load_hyp(a.ctl->cur);
  double v[ALIGN_SUMS] = {0, 0, 0, 0, 0, 0};
  bool in = false;
  if (i < n) {
    const AlignPair x{a.pa[i], a.pb[i]};
    in = align_inlier(m, x, a.thr2);
    if (in) { v[0] = x.p.x; v[1] = x.p.y; v[2] = x.p.z; v[3] = x.p.w; v[4] = x.q.x; v[5] = x.q.y; }
  }
  int total;
  block_rank<AB>(in, s_wave, total);
  block_tree_sum<ALIGN_SUMS>(v, s);
  if (threadIdx.x == 0) {
    a.blk[blockIdx.x] = total;
#pragma unroll
    for (int k = 0; k < ALIGN_SUMS; ++k) a.sums[(size_t)blockIdx.x * ALIGN_SUMS + k] = v[k];
  }
}

__global__ __launch_bounds__(AB) void align_moments_kernel(MapAlignArgs a) {
  __shared__ double s[ALIGN_MOMS * AB];
  if (!a.ctl->alive) return;
  const int cnt = counts_sum(a.blk, a.nb);
  double c6[ALIGN_SUMS];
  rows_sum<ALIGN_SUMS>(a.sums, a.nb, c6, s);
  double v[ALIGN_MOMS];
#pragma unroll
  for (int k = 0; k < ALIGN_MOMS; ++k) v[k] = 0.0;
  const int n = live_rows(a.d_n, a.n_max);
  const int i = blockIdx.x * AB + threadIdx.x;
  if (cnt >= 3 && i < n) {
    const AlignPair x{a.pa[i], a.pb[i]};
    if (align_inlier(load_hyp(a.ctl->cur), x, a.thr2)) {
      const double m = (double)cnt;
      const double da[3] = {x.p.x - c6[0] / m, x.p.y - c6[1] / m, x.p.z - c6[2] / m};
      const double db[3] = {x.p.w - c6[3] / m, x.q.x - c6[4] / m, x.q.y - c6[5] / m};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * r + c] = db[r] * da[c];
      v[9] = da[0] * da[0] + da[1] * da[1] + da[2] * da[2];
    }
  }
  block_tree_sum<ALIGN_MOMS>(v, s);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < ALIGN_MOMS; ++k) a.moms[(size_t)blockIdx.x * ALIGN_MOMS + k] = v[k];
  }
}

// one workgroup: the inlier count of the current model, and -- `last` == 0 -- the refit over them.  `last`: the pass behind the
// last round, which only counts.
__global__ __launch_bounds__(AB) void align_solve_kernel(MapAlignArgs a, int last) {
  __shared__ double s[ALIGN_MOMS * AB];
  MapAlignCtl* c = a.ctl;
  if (!c->alive) return;
  const int cnt = counts_sum(a.blk, a.nb);
  if (last) {
    if (threadIdx.x == 0) { c->cnt_cur = cnt; c->alive = 0; }
    return;
  }
  double c6[ALIGN_SUMS], mo[ALIGN_MOMS];
  rows_sum<ALIGN_SUMS>(a.sums, a.nb, c6, s);
  rows_sum<ALIGN_MOMS>(a.moms, a.nb, mo, s);
  if (threadIdx.x != 0) return;
  c->cnt_cur = cnt;                                         // of c->cur: the winner's in round 0, the last refit's afterwards
  bool ok = cnt >= 3;
  Sim sim;
  if (ok) {
    const double m = (double)cnt;
    const double ca[3] = {c6[0] / m, c6[1] / m, c6[2] / m}, cb[3] = {c6[3] / m, c6[4] / m, c6[5] / m};
    double Sg[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Sg[k] = mo[k] / m;
    ok = umeyama(Sg, mo[9] / m, ca, cb, a.with_scale, sim);
  }
  if (!ok) { c->alive = 0; return; }
  float f[ALIGN_FS];
  sim_to_floats(sim, f);
  for (int k = 0; k < ALIGN_FS; ++k) { c->ref[k] = f[k]; c->cur[k] = f[k]; }
  c->scale_ref = c->scale_cur = sim.c;
  c->have_ref = 1;
}

__global__ __launch_bounds__(64) void align_decide_kernel(MapAlignArgs a) {
  if (threadIdx.x != 0) return;
  MapAlignCtl* c = a.ctl;
  // with a valid refit, cnt_cur is the count of c->ref: every pass behind the solve that made it ran on it
  const bool kept = c->have_ref && c->cnt_cur >= c->win_cnt;
  int n_fin = kept ? c->cnt_cur : c->win_cnt;
  const int need = a.min_inliers > 3 ? a.min_inliers : 3;
  const int st = c->n < 3 ? VOE_MAP_ALIGN_FEW_MATCHES : c->win_h < 0 ? VOE_MAP_ALIGN_NO_HYPOTHESIS
               : n_fin < need ? VOE_MAP_ALIGN_FEW_INLIERS : VOE_MAP_ALIGN_OK;
  const bool ok = st == VOE_MAP_ALIGN_OK;
  for (int k = 0; k < ALIGN_FS; ++k) c->fin[k] = ok ? (kept ? c->ref[k] : c->win[k]) : (k < 12 && k % 4 == 0 ? 1.f : 0.f);
  c->scale_fin = ok ? (kept ? c->scale_ref : c->scale_win) : 1.0;
  c->status = st; c->kept = ok && kept; c->n_fin = ok ? n_fin : 0;
}

__global__ __launch_bounds__(AB) void align_out_kernel(MapAlignArgs a) {
  __shared__ double s[AB];
  const MapAlignCtl* c = a.ctl;
  const int n = live_rows(a.d_n, a.n_max);
  const int i = blockIdx.x * AB + threadIdx.x;
  double v[1] = {0.0};
  bool in = false;
  if (c->status == VOE_MAP_ALIGN_OK && i < n) {
    const AlignHyp m = load_hyp(c->fin);
    const AlignPair x{a.pa[i], a.pb[i]};
    in = align_inlier(m, x, a.thr2);
    if (in) v[0] = align_d2(m, x);
  }
  if (a.mask_out && i < a.n_max) a.mask_out[i] = in ? 1 : 0;
  block_tree_sum<1>(v, s);
  if (threadIdx.x == 0) a.rms[blockIdx.x] = v[0];
}

__global__ __launch_bounds__(AB) void align_finish_kernel(MapAlignArgs a) {
  __shared__ double s[AB];
  const MapAlignCtl* c = a.ctl;
  double v[1];
  rows_sum<1>(a.rms, a.nb, v, s);
  if (threadIdx.x != 0) return;
  float T[16];
  for (int col = 0; col < 3; ++col) {
    for (int r = 0; r < 3; ++r) T[r + 4 * col] = c->fin[r + 3 * col];
    T[3 + 4 * col] = 0.f;
  }
  T[12] = c->fin[9]; T[13] = c->fin[10]; T[14] = c->fin[11]; T[15] = 1.f;
  for (int k = 0; k < 16; ++k) a.S16_out[k] = T[k];
  voe_map_align_stats* st = static_cast<voe_map_align_stats*>(a.stats);
  st->status = c->status; st->n_matches = c->n; st->n_inliers = c->n_fin; st->best_hypothesis = c->win_h;
  st->best_count = c->win_cnt; st->n_valid = c->n_valid; st->refit_kept = c->kept; st->reserved = 0;
  st->scale = c->scale_fin;
  st->rms = c->n_fin > 0 ? sqrt(v[0] / (double)c->n_fin) : 0.0;
}

static int align_nb(int n_max) { const int nb = (n_max + AB - 1) / AB; return nb > 0 ? nb : 1; }

// The workspace, block by block (each 256-aligned); ws may be null (the walk then only measures)
MapAlignArgs map_align_layout(void* ws, int n_max, int n_hyp, size_t* bytes) {
  MapAlignArgs a{};
  const size_t n = (size_t)(n_max > 0 ? n_max : 1), H = (size_t)n_hyp, nb = (size_t)align_nb(n_max);
  WsCarver w(ws);
  a.ctl = w.take<MapAlignCtl>(sizeof(MapAlignCtl));
  a.pa = w.take<float4>(16 * n);
  a.pb = w.take<float2>(8 * n);
  a.hyp = w.take<float>(4 * ALIGN_FS * H);
  a.hyp_scale = w.take<double>(8 * H);
  a.counts = w.take<int>(4 * H);
  a.blk = w.take<int>(4 * nb);
  a.sums = w.take<double>(8 * ALIGN_SUMS * nb);
  a.moms = w.take<double>(8 * ALIGN_MOMS * nb);
  a.rms = w.take<double>(8 * nb);
  a.bxyz = w.take<float>(12 * n);
  a.n_max = n_max; a.n_hyp = n_hyp; a.nb = (int)nb;
  if (bytes) *bytes = w.bytes;
  return a;
}

hipError_t launch_map_align(hipStream_t st, const MapAlignArgs& a) {
  hipError_t e = hipMemsetAsync(a.ctl, 0, sizeof(MapAlignCtl), st);
  if (e == hipSuccess) e = hipMemsetAsync(a.counts, 0, sizeof(int) * (size_t)a.n_hyp, st);
  if (e != hipSuccess) return e;
  const int nb = a.nb;
  hipLaunchKernelGGL(align_gather_kernel, dim3(nb < 1024 ? nb : 1024), dim3(AB), 0, st, a);
  hipLaunchKernelGGL(align_hyp_kernel, dim3((a.n_hyp + 63) / 64), dim3(64), 0, st, a);
  const int nsb = (a.n_max + AB * ALIGN_PTS - 1) / (AB * ALIGN_PTS);
  hipLaunchKernelGGL(align_score_kernel, dim3(nsb > 0 ? nsb : 1, (a.n_hyp + RANSAC_HB - 1) / RANSAC_HB), dim3(AB), 0, st, a);
  hipLaunchKernelGGL(align_select_kernel, dim3(1), dim3(1024), 0, st, a);
  for (int r = 0; r <= a.n_refits && a.n_refits > 0; ++r) {
    const int last = r == a.n_refits;                          // the pass behind the last round: the count of its refit
    hipLaunchKernelGGL(align_sums_kernel, dim3(nb), dim3(AB), 0, st, a);
    if (!last) hipLaunchKernelGGL(align_moments_kernel, dim3(nb), dim3(AB), 0, st, a);
    hipLaunchKernelGGL(align_solve_kernel, dim3(1), dim3(AB), 0, st, a, last);
  }
  hipLaunchKernelGGL(align_decide_kernel, dim3(1), dim3(64), 0, st, a);
  hipLaunchKernelGGL(align_out_kernel, dim3(nb), dim3(AB), 0, st, a);
  hipLaunchKernelGGL(align_finish_kernel, dim3(1), dim3(AB), 0, st, a);
  return hipGetLastError();
}

// ---- the merge's own kernels: the misses of the lookup, compacted in src order ------------------------------------------------
__global__ void merge_begin_kernel(int* ctl, const int* dst_hdr) {
  if (threadIdx.x == 0 && blockIdx.x == 0) ctl[0] = dst_hdr[0];
}

__global__ __launch_bounds__(AB) void merge_count_kernel(const int32_t* ent, const int* src_hdr, int n_max, int* blk) {
  __shared__ int s_wave[AB / 64];
  const int n = live_rows(src_hdr, n_max);
  const int i = blockIdx.x * AB + threadIdx.x;
  int total;
  block_rank<AB>(i < n && ent[i] < 0, s_wave, total);
  if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

__global__ __launch_bounds__(AB) void merge_scatter_kernel(const int32_t* ent, const int* src_hdr, int n_max, const int* blk,
                                                           const float* src_pts, const float* src_app, float* out_pts, float* out_app) {
  __shared__ int s_wave[AB / 64];
  const int n = live_rows(src_hdr, n_max);
  const int i = blockIdx.x * AB + threadIdx.x;
  const bool miss = i < n && ent[i] < 0;
  int total;
  const int r = block_rank<AB>(miss, s_wave, total);
  if (!miss) return;
  const size_t o = (size_t)(blk[blockIdx.x] + r);              // < n <= n_max: one slot per miss at most
  out_pts[3 * o] = src_pts[3 * (size_t)i]; out_pts[3 * o + 1] = src_pts[3 * (size_t)i + 1]; out_pts[3 * o + 2] = src_pts[3 * (size_t)i + 2];
  const float2* s = reinterpret_cast<const float2*>(src_app) + 5 * (size_t)i;      // the appearance's bits
  float2* d = reinterpret_cast<float2*>(out_app) + 5 * o;
#pragma unroll
  for (int k = 0; k < 5; ++k) d[k] = s[k];
}

__global__ void merge_stats_kernel(const int* ctl, const int* src_hdr, const int* dst_hdr, int n_max, voe_map_merge_stats* st) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  st->n_src = live_rows(src_hdr, n_max);
  st->n_shared = ctl[1];
  st->n_dst_after = dst_hdr[0];
  st->n_appended = dst_hdr[0] - ctl[0];
}

MapMergeWs map_merge_layout(void* ws, int n_max) {
  MapMergeWs m{};
  const size_t n = (size_t)(n_max > 0 ? n_max : 1);
  WsCarver w(ws);
  m.ctl = w.take<int>(64);
  m.ent = w.take<int32_t>(4 * n);
  m.pairs = w.take<int32_t>(8 * n);
  m.blk = w.take<int>(4 * (size_t)align_nb(n_max));
  m.stage_pts = w.take<float>(12 * n);
  m.stage_app = w.take<float>(40 * n);
  m.bytes = w.bytes;
  return m;
}

hipError_t launch_map_merge_begin(hipStream_t st, const MapMergeWs& w, const int* dst_hdr) {
  hipLaunchKernelGGL(merge_begin_kernel, dim3(1), dim3(64), 0, st, w.ctl, dst_hdr);
  return hipGetLastError();
}

hipError_t launch_map_merge_misses(hipStream_t st, const MapMergeWs& w, const float* src_pts, const float* src_app, const int* src_hdr,
                                   int n_max) {
  if (n_max <= 0) return hipMemsetAsync(w.ctl + 2, 0, sizeof(int), st);
  const int nb = align_nb(n_max);
  hipLaunchKernelGGL(merge_count_kernel, dim3(nb), dim3(AB), 0, st, w.ent, src_hdr, n_max, w.blk);
  hipError_t e = launch_scan(st, w.blk, nb, w.ctl + 2);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(merge_scatter_kernel, dim3(nb), dim3(AB), 0, st, w.ent, src_hdr, n_max, w.blk, src_pts, src_app, w.stage_pts,
                     w.stage_app);
  return hipGetLastError();
}

hipError_t launch_map_merge_stats(hipStream_t st, const MapMergeWs& w, const int* src_hdr, const int* dst_hdr, int n_max, void* stats) {
  hipLaunchKernelGGL(merge_stats_kernel, dim3(1), dim3(64), 0, st, w.ctl, src_hdr, dst_hdr, n_max, static_cast<voe_map_merge_stats*>(stats));
  return hipGetLastError();
}

}  // namespace vo
