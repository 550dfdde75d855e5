// step_gap.hip -- what lies between two steps of the headline ("Between two steps"): the submission
// shape of one 50-round solve, 11 launches of the round's geometry (197 x 256 threads), replayed by a C++ loop with
// kernels that do nothing but read one word their predecessor wrote and write the next.  Four patterns:
//   a  one plain launch, then hipGraphLaunch of a graph of 10 kernels        (how a solve is submitted)
//   b  hipGraphLaunch of a graph of 11 kernels
//   c  11 plain launches
//   d  pattern a, the graph's last kernel also storing one word to pinned host memory (the tail launch's report)
// Per pattern: device us per step (two events around the whole timed loop) and host us per step (the enqueue calls
// alone).  200 untimed steps, then 2000 timed.  With empty kernels the host is the limit of pattern c (a plain launch takes
// it longer than an empty kernel takes the device), so the tool takes a third argument: every kernel then lasts at least
// `work_ticks` ticks of the 100 MHz wall clock (345: a round's 3.45 us), a bounded wait of one thread on the clock alone,
// and the patterns are compared where the device is the limit, as in a solve.
//   build: hipcc --offload-arch=gfx950 -O2 -o bin/step_gap step_gap.hip
//   usage: step_gap [steps=2000] [untimed=200] [work_ticks=0]
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>

using clk = std::chrono::steady_clock;
static double us(clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); }

constexpr int LAUNCHES = 11, GRID = 197, BLOCK = 256;

// words[k + 1] = words[k] + 1 by one thread; `report`: pinned host memory or null
__global__ void link_kernel(int* words, int k, int* report, unsigned work_ticks) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int v = words[k] + 1;
    if (work_ticks) { const unsigned long long t0 = wall_clock64(); while (wall_clock64() - t0 < work_ticks) {} }
    words[k + 1] = v;
    if (report) __hip_atomic_store(report, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

#define CHECK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static unsigned g_work = 0;
static hipError_t plain(hipStream_t st, int* words, int from, int to, int* report) {
  for (int k = from; k < to; ++k) hipLaunchKernelGGL(link_kernel, dim3(GRID), dim3(BLOCK), 0, st, words, k, k == LAUNCHES - 1 ? report : nullptr, g_work);
  return hipGetLastError();
}

static hipError_t capture(hipStream_t st, int* words, int from, int* report, hipGraphExec_t* out) {
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) return e;
  const hipError_t el = plain(st, words, from, LAUNCHES, report);
  e = hipStreamEndCapture(st, &g);
  if (e == hipSuccess && el != hipSuccess) e = el;
  if (e == hipSuccess) e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
  if (g) (void)hipGraphDestroy(g);
  return e;
}

int main(int argc, char** argv) {
  const int steps = argc > 1 ? atoi(argv[1]) : 2000, untimed = argc > 2 ? atoi(argv[2]) : 200;
  const int work = argc > 3 ? atoi(argv[3]) : 0;
  if (steps < 1 || untimed < 0 || work < 0 || work > 100000) return 2;
  g_work = (unsigned)work;
  hipStream_t st;
  CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  int *words = nullptr, *report = nullptr;
  CHECK(hipMalloc(&words, (LAUNCHES + 1) * sizeof(int)));
  CHECK(hipMemset(words, 0, (LAUNCHES + 1) * sizeof(int)));
  CHECK(hipHostMalloc(&report, sizeof(int), hipHostMallocDefault));
  *report = 0;
  hipGraphExec_t g10 = nullptr, g11 = nullptr, g10r = nullptr;
  CHECK(capture(st, words, 1, nullptr, &g10));
  CHECK(capture(st, words, 0, nullptr, &g11));
  CHECK(capture(st, words, 1, report, &g10r));
  hipEvent_t ev0, ev1;
  CHECK(hipEventCreate(&ev0));
  CHECK(hipEventCreate(&ev1));
  std::printf("{\"grid\": %d, \"block\": %d, \"launches_per_step\": %d, \"steps\": %d, \"untimed\": %d, \"work_ticks\": %d", GRID, BLOCK, LAUNCHES, steps, untimed, work);
  const char* names[4] = {"a_plain_plus_graph10", "b_graph11", "c_plain11", "d_plain_plus_graph10_report"};
  for (int rep = 0; rep < 2; ++rep) {             // (every pattern twice, the order kept: the second pass is the record's check on the first)
    for (int p = 0; p < 4; ++p) {
      double host = 0;
      hipError_t e = hipSuccess;
      for (int s = -untimed; s < steps && e == hipSuccess; ++s) {
        if (s == 0) { CHECK(hipStreamSynchronize(st)); CHECK(hipEventRecord(ev0, st)); }
        const auto t0 = clk::now();
        if (p == 0) { e = plain(st, words, 0, 1, nullptr); if (e == hipSuccess) e = hipGraphLaunch(g10, st); }
        else if (p == 1) e = hipGraphLaunch(g11, st);
        else if (p == 2) e = plain(st, words, 0, LAUNCHES, nullptr);
        else { e = plain(st, words, 0, 1, nullptr); if (e == hipSuccess) e = hipGraphLaunch(g10r, st); }
        const auto t1 = clk::now();
        if (s >= 0) host += us(t0, t1);
      }
      CHECK(e);
      CHECK(hipEventRecord(ev1, st));
      CHECK(hipEventSynchronize(ev1));
      float ms = 0;
      CHECK(hipEventElapsedTime(&ms, ev0, ev1));
      std::printf(", \"%s%s\": {\"device_us_per_step\": %.3f, \"host_us_per_step\": %.3f}", names[p], rep ? "_again" : "", ms * 1e3 / steps, host / steps);
    }
  }
  int last = 0;
  CHECK(hipMemcpy(&last, words + LAUNCHES, sizeof(int), hipMemcpyDeviceToHost));
  std::printf(", \"chain_word\": %d, \"report_word\": %d}\n", last, *report);
  (void)hipGraphExecDestroy(g10); (void)hipGraphExecDestroy(g11); (void)hipGraphExecDestroy(g10r);
  (void)hipEventDestroy(ev0); (void)hipEventDestroy(ev1);
  (void)hipHostFree(report); (void)hipFree(words);
  (void)hipStreamDestroy(st);
  return last == LAUNCHES ? 0 : 1;
}
