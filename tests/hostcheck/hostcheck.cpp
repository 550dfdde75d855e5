// hostcheck.cpp -- compiles the __host__ __device__ functors of
// visual-odometry_amd/csrc/vo_math.h with g++ so that the per-element logic the
// kernels run (projection gates, PICP term, pivoted LDLT, pose update,
// triangulate_point) can be compared with the oracle in the GPU-less
// container.  TEST INFRASTRUCTURE: not part of libvo_hip.so, never shipped.
#include "../../visual-odometry_amd/csrc/vo_math.h"

using namespace vo;

static CamK mk(int rows, int cols, int zn, int zf, const float* K) {
  CamK c; for (int i = 0; i < 9; ++i) c.K[i] = K[i];
  c.rows = rows; c.cols = cols; c.z_near = zn; c.z_far = zf; return c;
}

extern "C" {

int hc_project_point(int rows, int cols, int zn, int zf, const float* K, const float* T16,
                     const float* p, float* uv) {
  float pc[3], ph[3], inv;
  return project_point(mk(rows, cols, zn, zf, K), pose_from_T16(T16), p[0], p[1], p[2], uv[0], uv[1], pc, ph, inv) ? 1 : 0;
}

// accumulates n correspondences sequentially into acc[30] (zeroed here)
void hc_picp_accumulate(int rows, int cols, int zn, int zf, const float* K, const float* T16, float thr,
                        int keep, const float* world, const float* meas, const int* corr, int n, float* acc) {
  const CamK cam = mk(rows, cols, zn, zf, K);
  const Pose T = pose_from_T16(T16);
  for (int k = 0; k < NACC; ++k) acc[k] = 0.f;
  for (int i = 0; i < n; ++i) {
    const float* w = world + 3 * corr[2 * i + 1];
    const float* z = meas + 2 * corr[2 * i];
    picp_accumulate(cam, T, thr, keep != 0, w[0], w[1], w[2], z[0], z[1], acc);
  }
}

// PINHOLE instantiation (structural zeros of K removed): must equal the general one bit for bit
void hc_picp_accumulate_pinhole(int rows, int cols, int zn, int zf, const float* K, const float* T16, float thr,
                                int keep, const float* world, const float* meas, const int* corr, int n, float* acc) {
  const CamK cam = mk(rows, cols, zn, zf, K);
  const Pose T = pose_from_T16(T16);
  for (int k = 0; k < NACC; ++k) acc[k] = 0.f;
  for (int i = 0; i < n; ++i) {
    const float* w = world + 3 * corr[2 * i + 1];
    const float* z = meas + 2 * corr[2 * i];
    if (keep) picp_accumulate_t<true, true>(cam, T, thr, w[0], w[1], w[2], z[0], z[1], acc);
    else picp_accumulate_t<true, false>(cam, T, thr, w[0], w[1], w[2], z[0], z[1], acc);
  }
}

// the batched solver's instantiations (MUL0: a rejected term is zeroed through vo_mul0 -- on the host the same rule spelled out):
// `general` != 0 takes the 3x3-K form.  Contributing terms must get the bits of the forms above; rejected ones exact zeros.
void hc_picp_accumulate_mul0(int rows, int cols, int zn, int zf, const float* K, const float* T16, float thr, int keep, int general,
                             const float* world, const float* meas, const int* corr, int n, float* acc) {
  const CamK cam = mk(rows, cols, zn, zf, K);
  const Pose T = pose_from_T16(T16);
  for (int k = 0; k < NACC; ++k) acc[k] = 0.f;
  for (int i = 0; i < n; ++i) {
    const float* w = world + 3 * corr[2 * i + 1];
    const float* z = meas + 2 * corr[2 * i];
    if (general) {
      if (keep) picp_accumulate_t<false, true, true, true>(cam, T, thr, w[0], w[1], w[2], z[0], z[1], acc);
      else picp_accumulate_t<false, false, true, true>(cam, T, thr, w[0], w[1], w[2], z[0], z[1], acc);
    } else {
      if (keep) picp_accumulate_t<true, true, true, true>(cam, T, thr, w[0], w[1], w[2], z[0], z[1], acc);
      else picp_accumulate_t<true, false, true, true>(cam, T, thr, w[0], w[1], w[2], z[0], z[1], acc);
    }
  }
}

int hc_is_pinhole(const float* K) { return is_pinhole(K) ? 1 : 0; }

void hc_picp_update(const float* acc, float damping, const float* T16, float* T16_out, float* H, float* b) {
  const Pose Tn = picp_update(acc, damping, pose_from_T16(T16), H, b);
  pose_to_T16(Tn, T16_out);
}

void hc_ldlt6(const float* A_colmajor, const float* rhs, float* x) {
  float a[6][6];
  for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) a[r][c] = A_colmajor[r + 6 * c];
  ldlt6_solve(a, rhs, x);
}

// latency-optimised variant used by the kernels: permutation up front
void hc_ldlt6_perm(const float* A_colmajor, const float* rhs, float* x) {
  float full[36], scratch[6];
  for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) full[6 * r + c] = A_colmajor[r + 6 * c];
  ldlt6_solve_perm(full, rhs, scratch, x);
}

// the round kernels' solve since round 3: natural elimination order (H is positive definite)
void hc_ldlt6_ordered(const float* A_colmajor, const float* rhs, float* x) {
  float B[6][6], y[6];
  for (int r = 0; r < 6; ++r) { y[r] = rhs[r]; for (int c = 0; c < 6; ++c) B[r][c] = A_colmajor[r + 6 * c]; }
  ldlt6_solve_ordered(B, y);
  for (int r = 0; r < 6; ++r) x[r] = y[r];
}
void hc_sincos_small(float v, float* s, float* c) { sincos_small(v, *s, *c); }

// The pieces of the round kernels' tail (picp.hip, picp_tail_direct) put together as that function puts them together:
// ldlt6_solve_ordered on H itself with -b, ONE branch for the three angles (sincosf when any exceeds 0.5 rad, the polynomial
// otherwise), v2t_from_sincos, T <- dT * T.  H col-major with the damping on its diagonal.
void hc_picp_tail_fast(const float* H_colmajor, const float* b, const float* T16, float* T16_out) {
  float B[6][6], y[6];
  for (int r = 0; r < 6; ++r) { y[r] = -b[r]; for (int c = 0; c < 6; ++c) B[r][c] = c <= r ? H_colmajor[r + 6 * c] : 0.f; }
  ldlt6_solve_ordered(B, y);
  float sn[3], cs[3];
  const bool big = !(fabsf(y[3]) <= 0.5f && fabsf(y[4]) <= 0.5f && fabsf(y[5]) <= 0.5f);
  for (int m = 0; m < 3; ++m) {
    if (big) sincosf(y[3 + m], &sn[m], &cs[m]);
    else sincos_small(y[3 + m], sn[m], cs[m]);
  }
  const Pose dT = v2t_from_sincos(y, sn[0], cs[0], sn[1], cs[1], sn[2], cs[2]);
  pose_to_T16(pose_mul(dT, pose_from_T16(T16)), T16_out);
}

void hc_ldlt2(const float* m, const float* rhs, float* x) { ldlt2_solve(m[0], m[1], m[3], rhs[0], rhs[1], x[0], x[1]); }

int hc_triangulate_point(const float* d1, const float* d2, const float* p2, float* p) {
  return triangulate_point(d1, d2, p2, p) ? 1 : 0;
}

void hc_tri_constants(const float* K, const float* X16, float* iK, float* iRiK, float* t) {
  const TriConst c = tri_constants(K, pose_from_T16(X16));
  for (int i = 0; i < 9; ++i) { iK[i] = c.iK[i]; iRiK[i] = c.iRiK[i]; }
  for (int i = 0; i < 3; ++i) t[i] = c.t[i];
}

void hc_v2t(const float* v, float* T16) { pose_to_T16(v2t_euler(v), T16); }

// the map's key functions (map.hip runs these very definitions): n rows of ten floats -> hash, NaN flag; hashes -> home slots
void hc_map_hash(const float* app, int n, uint32_t* h, int* has_nan) {
  for (int i = 0; i < n; ++i) {
    Row r;
    for (int k = 0; k < 10; ++k) r.v[k] = app[10 * (size_t)i + k];
    h[i] = map_hash(r);
    if (has_nan) has_nan[i] = map_row_has_nan(r) ? 1 : 0;
  }
}
void hc_map_home_slot(const uint32_t* h, int n, uint32_t tmask, uint32_t* slot) {
  for (int i = 0; i < n; ++i) slot[i] = map_home_slot(h[i], tmask);
}
int hc_map_rows_equal(const float* a, const float* b) {
  Row x, y;
  for (int k = 0; k < 10; ++k) { x.v[k] = a[k]; y.v[k] = b[k]; }
  return map_rows_equal(x, y) ? 1 : 0;
}

// The arithmetic of picp_exact_kernel on the host: terms by picp_term_exact, entry k summed sequentially in
// correspondence order, tail picp_update_t<true>.  Records per round H (damping included, col-major), b,
// (chi_in, chi_out, n_in), pose -- must equal the oracle's picp_solve_raw bit for bit.
void hc_picp_exact(int rows, int cols, int zn, int zf, const float* K, const float* T16, float thr, int keep,
                   const float* world, const float* meas, const int* corr, int n, int n_iters, float* tH, float* tb,
                   float* ts, float* tT) {
  const CamK cam = mk(rows, cols, zn, zf, K);
  Pose T = pose_from_T16(T16);
  for (int it = 0; it < n_iters; ++it) {
    float acc[NACC];
    for (int k = 0; k < NACC; ++k) acc[k] = 0.f;
    for (int i = 0; i < n; ++i) {
      const float* w = world + 3 * corr[2 * i + 1];
      const float* z = meas + 2 * corr[2 * i];
      float term[NTERM];
      const int f = picp_term_exact(cam, T, thr, w[0], w[1], w[2], z[0], z[1], term);
      if (!f) continue;
      if (f == 1 || keep) for (int k = 0; k < 27; ++k) acc[k] += term[k];
      if (f == 1) { acc[27] += term[27]; acc[29] += 1.f; } else acc[28] += term[27];
    }
    T = picp_update_t<true>(acc, 1.f, T, tH + 36 * it, tb + 6 * it);
    ts[3 * it] = acc[27]; ts[3 * it + 1] = acc[28]; ts[3 * it + 2] = acc[29];
    pose_to_T16(T, tT + 16 * it);
  }
}
}
