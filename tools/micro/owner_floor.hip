// Floor of a round of the "32 row-group owners" form of the single-problem solver: 32 workgroups of
// 1024 threads, each four virtual blocks of 256 threads that linearise and reduce the tiles g, g + 32, ... of one row group
// exactly as a 256-thread workgroup of picp_round_kernel does (same picp_accumulate_t, same quad reduction, tile sums added
// in tile order), correspondences held in registers, then the group sum, the staged 32-way sum and the tail in every wave.
// What is LEFT OUT is the exchange of the 32 group rows between the workgroups (each workgroup stages its own row 32 times
// through LDS instead): the time per round printed here is what the owner form cannot go below, before any hand-off.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -mllvm -amdgpu-kernarg-preload-count=16
//        -o tools/micro/bin/owner_floor tools/micro/owner_floor.hip ; run on the GPU box: owner_floor [n]
#include "../../visual-odometry_amd/csrc/picp.hip"

#include <cstdio>
#include <vector>

namespace vo {

constexpr int OWN_VB = 4;                         // virtual blocks per workgroup
constexpr int OWN_GROUPS = 32;

// block_reduce_quad up to the part sums, for virtual block `vb` (its own s_acc / s_part regions); the barriers are the workgroup's
__device__ __forceinline__ void owner_reduce_parts(float acc[NACC], float* s_acc, float* s_part, int tid) {
#pragma unroll
  for (int k = 0; k < NACC; ++k) {
    acc[k] += dpp_mov<0xB1>(acc[k]);
    acc[k] += dpp_mov<0x4E>(acc[k]);
  }
  const int q = tid & 3;
  const bool q1 = q == 1, q2 = q == 2, q3 = q == 3;
  float w[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float a0 = acc[j], a1 = acc[8 + j], a2 = acc[16 + j], a3 = 24 + j < NACC ? acc[24 + j < NACC ? 24 + j : 0] : 0.f;
    asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));
    float v = a0;
    v = q1 ? a1 : v;
    v = q2 ? a2 : v;
    v = q3 ? a3 : v;
    w[j] = v;
  }
  float4* row = reinterpret_cast<float4*>(s_acc + (tid >> 2) * ACC_STRIDE + 8 * q);
  row[0] = make_float4(w[0], w[1], w[2], w[3]);
  row[1] = make_float4(w[4], w[5], w[6], w[7]);
  __syncthreads();
  constexpr int ROWS_PER_PART = (PICP_BLOCK / 4) / PICP_PARTS;
  const int slot = tid & 31, part = tid >> 5;
  const float* src = s_acc + (part * ROWS_PER_PART) * ACC_STRIDE + slot;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < ROWS_PER_PART; ++j) s += src[j * ACC_STRIDE];
  s_part[part * 32 + slot] = s;
  __syncthreads();
}

template <bool PINHOLE, bool KEEP>
__global__ __launch_bounds__(OWN_VB* PICP_BLOCK) void owner_floor_kernel(const PicpParams* __restrict__ P, const float* pk_base,
                                                                         size_t pk_cap, int n, int nb, int n_iters, float* out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* s_acc_all = smem;                                    // OWN_VB x PICP_BLOCK * ACC_STRIDE
  float* s_part_all = s_acc_all + OWN_VB * PICP_BLOCK * ACC_STRIDE;   // OWN_VB x PICP_PARTS * 32
  float* s_stage = s_part_all + OWN_VB * PICP_PARTS * 32;     // 32 * STG_STRIDE
  float* s_own = s_stage + 32 * STG_STRIDE;                   // 32
  const PackedCorr pk{const_cast<float*>(pk_base), pk_cap};
  const int tid = threadIdx.x, vb = tid >> 8, vt = tid & 255, lane = tid & 63;
  const int g = blockIdx.x;
  float* s_acc = s_acc_all + vb * PICP_BLOCK * ACC_STRIDE;
  float* s_part = s_part_all + vb * PICP_PARTS * 32;
  const CamK cam = P->cam;
  const float thr = P->thr, damping = P->damping;
  float cx[2], cy[2], cz[2], cu[2], cv[2];
  bool have[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int b = g + OWN_GROUPS * (OWN_VB * k + vb), i = b * PICP_BLOCK + vt;
    have[k] = b < nb && i < n;
    cx[k] = cy[k] = cz[k] = cu[k] = cv[k] = 0.f;
    if (have[k]) { cx[k] = pk.arr(0)[i]; cy[k] = pk.arr(1)[i]; cz[k] = pk.arr(2)[i]; cu[k] = pk.arr(3)[i]; cv[k] = pk.arr(4)[i]; }
  }
  Pose T;
#pragma unroll
  for (int k = 0; k < 9; ++k) T.R[k] = (k % 4 == 0) ? 1.f : 0.f;
  T.t[0] = T.t[1] = T.t[2] = 0.f;
  T = uniform_pose(T);
  for (int it = 0; it < n_iters; ++it) {
    float gsum = 0.f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      float acc[NACC];
#pragma unroll
      for (int j = 0; j < NACC; ++j) acc[j] = 0.f;
      if (have[k]) picp_accumulate_t<PINHOLE, KEEP>(cam, T, thr, cx[k], cy[k], cz[k], cu[k], cv[k], acc);
      owner_reduce_parts(acc, s_acc, s_part, vt);
      if (tid < 32) {                                          // the four tiles' rows, in tile order, onto the group sum
#pragma unroll
        for (int v2 = 0; v2 < OWN_VB; ++v2) {
          float o = 0.f;
#pragma unroll
          for (int p = 0; p < PICP_PARTS; ++p) o += s_part_all[(v2 * PICP_PARTS + p) * 32 + tid];
          gsum += tid < NACC ? o : 0.f;
        }
      }
    }
    if (tid < 32) s_own[tid] = gsum * (1.f / OWN_GROUPS);      // (stand-in for the exchange: 32 copies of a 32nd)
    __syncthreads();
    s_stage[(tid & 31) * STG_STRIDE + (tid >> 5)] = s_own[tid & 31];
    __syncthreads();
    float val = 0.f;
    if (lane < 45) {
      int slot;
      bool diag = false;
      if (lane < 36) {
        const int r = lane / 6, c = lane - 6 * r;
        const int lo = r < c ? r : c, hi = r < c ? c : r;
        slot = (13 * lo - lo * lo) / 2 + (hi - lo);
        diag = r == c;
      } else {
        slot = 21 + (lane - 36);
      }
      const float4* row = reinterpret_cast<const float4*>(s_stage + slot * STG_STRIDE);
      float tsum = 0.f;
#pragma unroll
      for (int k = 0; k < PICP_GROUPS / 4; ++k) { const float4 t4 = row[k]; tsum += t4.x; tsum += t4.y; tsum += t4.z; tsum += t4.w; }
      if (lane < 36) val = diag ? tsum + 1.f * damping : tsum;
      else if (lane < 42) val = -tsum;
    }
    float b0, b1, b2;
    pose_lane_operands(T, b0, b1, b2);
    T = uniform_pose(picp_tail_direct(val, b0, b1, b2));
    __syncthreads();
  }
  if (tid == 0) out[g] = T.t[0] + T.R[0];
}

}  // namespace vo

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
  using namespace vo;
  const int n = argc > 1 ? atoi(argv[1]) : 50000;
  const int nb = (n + PICP_BLOCK - 1) / PICP_BLOCK;
  if (nb > OWN_GROUPS * OWN_VB * 2) { printf("n too large for two batches\n"); return 1; }
  const size_t cap = ((size_t)n + 3) & ~(size_t)3;
  // a synthetic pair: points in front of a 640 x 480 pinhole camera, measurements = their projections moved by a pixel
  std::vector<float> pkh(5 * cap, 0.f);
  unsigned s = 12345u;
  auto rnd = [&] { s = s * 1664525u + 1013904223u; return (s >> 8) * (1.f / 16777216.f); };
  for (int i = 0; i < n; ++i) {
    const float z = 1.f + 8.f * rnd(), x = (rnd() - 0.5f) * 1.5f * z, y = (rnd() - 0.5f) * 1.1f * z;
    pkh[i] = x; pkh[cap + i] = y; pkh[2 * cap + i] = z;
    pkh[3 * cap + i] = 180.f * x / z + 320.f + (rnd() - 0.5f) * 2.f;
    pkh[4 * cap + i] = 180.f * y / z + 240.f + (rnd() - 0.5f) * 2.f;
  }
  PicpParams hp{};
  const float K[9] = {180.f, 0.f, 0.f, 0.f, 180.f, 0.f, 320.f, 240.f, 1.f};      // column-major
  for (int k = 0; k < 9; ++k) hp.cam.K[k] = K[k];
  hp.cam.rows = 480; hp.cam.cols = 640; hp.cam.z_near = 0; hp.cam.z_far = 10;
  hp.thr = 10000.f; hp.damping = 1.f; hp.keep_outliers = 0; hp.n_corr = n;
  PicpParams* dP; float *dpk, *dout;
  CK(hipMalloc(&dP, sizeof(hp))); CK(hipMalloc(&dpk, sizeof(float) * 5 * cap)); CK(hipMalloc(&dout, sizeof(float) * OWN_GROUPS));
  CK(hipMemcpy(dP, &hp, sizeof(hp), hipMemcpyHostToDevice));
  CK(hipMemcpy(dpk, pkh.data(), sizeof(float) * 5 * cap, hipMemcpyHostToDevice));
  const size_t lds = sizeof(float) * (OWN_VB * PICP_BLOCK * ACC_STRIDE + OWN_VB * PICP_PARTS * 32 + 32 * STG_STRIDE + 32);
  auto kern = owner_floor_kernel<true, false>;
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  double ms[2] = {0, 0};
  const int iters[2] = {50, 150}, reps = 50;
  for (int pass = 0; pass < 2; ++pass)            // pass 0 warms up
    for (int w = 0; w < 2; ++w) {
      CK(hipEventRecord(e0));
      for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(kern, dim3(OWN_GROUPS), dim3(OWN_VB * PICP_BLOCK), lds, 0, dP, dpk, cap, n, nb, iters[w], dout);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      CK(hipGetLastError());
      float t; CK(hipEventElapsedTime(&t, e0, e1));
      ms[w] = t / reps;
    }
  float o[OWN_GROUPS];
  CK(hipMemcpy(o, dout, sizeof(o), hipMemcpyDeviceToHost));
  printf("n %d tiles %d lds %zu B: launch of 50 rounds %.2f us, of 150 rounds %.2f us -> %.3f us per round without the exchange (check %g)\n",
         n, nb, lds, ms[0] * 1e3, ms[1] * 1e3, (ms[1] - ms[0]) * 1e3 / 100.0, o[0]);
  return 0;
}
